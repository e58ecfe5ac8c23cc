// track_candidates.hpp — which observation slot is a candidate of which image: the two launches that
// misift_refine_cameras_batch (kernels_refine.hip) and misift_resect_cameras_batch (kernels_resect.hip) start with.  The
// rule (T, O, valid tracks, the owner of a slot, the candidates of an image) is stated once, in include/misift.h under
// misift_refine_cameras_batch.  Each file that includes this compiles its own copy of the kernels.
//   cand_owner_kernel  256-thread workgroups, one lane per track, the grid sized from max_tracks.  T and O are read from
//                      the export summary on the device.  A lane whose track is valid walks its range with
//                      atomicMax(owner[o], t), so a slot ends with the largest valid track that holds it (owner[] is
//                      memset to -1 before).
//   cand_key_kernel    one lane per slot, the grid sized from max_obs: key[o] = the observation's frame when slot o is a
//                      candidate of that image (it has an owner of status 0 with a finite point, its position is finite
//                      and its frame lies in [0, nimages)), otherwise -1.
#pragma once
#include "common.hpp"
#include "triangulate_core.hpp"

namespace {

constexpr int CAND_THREADS = FUND_SLOTS;

struct alignas(16) CandObs {                   // misift_track_obs, read with one 16-byte load
  int frame, record;
  float xpos, ypos;
};
static_assert(sizeof(CandObs) == sizeof(misift_track_obs), "CandObs mirrors misift_track_obs");

struct CandArgs {
  int max_tracks, max_obs, nimages;
  const int *track_offsets;
  const CandObs *obs;
  const int *export_summary;
  const float *points;                         // max_tracks x 4
  const int *point_status;
  int *owner, *key;                            // temp: max_obs each
};

__device__ __forceinline__ int cand_T(const CandArgs &A) { return min(max(A.export_summary[2], 0), A.max_tracks); }
__device__ __forceinline__ int cand_O(const CandArgs &A) { return min(max(A.export_summary[3], 0), A.max_obs); }

__global__ __launch_bounds__(CAND_THREADS) void cand_owner_kernel(CandArgs A)
{
  const int t = blockIdx.x * CAND_THREADS + threadIdx.x;     // below max_tracks + 256: no overflow
  if (t >= cand_T(A)) return;
  const int off = A.track_offsets[t], end = A.track_offsets[t + 1];
  if (!tri_range_ok(off, end, cand_O(A))) return;            // before it addresses anything
  for (int o = off; o < end; o++) atomicMax(&A.owner[o], t);
}

__global__ __launch_bounds__(CAND_THREADS) void cand_key_kernel(CandArgs A)
{
  const int o = blockIdx.x * CAND_THREADS + threadIdx.x;
  if (o >= cand_O(A)) return;
  const int t = A.owner[o];
  int key = -1;
  if (t >= 0 && A.point_status[t] == TRI_OK) {
    const float *X = A.points + 4 * (size_t)t;
    const CandObs ob = A.obs[o];
    if (fundamental_finite(X[0]) && fundamental_finite(X[1]) && fundamental_finite(X[2]) && fundamental_finite(ob.xpos) &&
        fundamental_finite(ob.ypos) && ob.frame >= 0 && ob.frame < A.nimages)
      key = ob.frame;
  }
  A.key[o] = key;
}

inline dim3 cand_blocks(int n) { return dim3((unsigned)(((long long)n + CAND_THREADS - 1) / CAND_THREADS)); }

}  // namespace

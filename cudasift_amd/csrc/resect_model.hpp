// resect_model.hpp — what misift_resect_cameras_batch (kernels_resect.hip) and misift_localize_frames_batch
// (kernels_localize.hip) share of their searches: the ransac_batch.hpp model over candidates (x, y, X, Y, Z) under the
// intrinsics of the entry's image, the six-point solve of one lane, and the entry's results as the pick kernels write
// them.  The arithmetic is resect_core.hpp (the draw, the solve) and refine_core.hpp (the inlier test).
//
// Args is the search's argument struct.  Beside rs it holds s (a TrackScene: intrinsics is the pinned host copy), images
// (the pinned host copy, one image per entry, checked on the host to lie in [0, nimages)), min_inliers, install, cam,
// cam_pair, res_cam, res_cand, res_inliers, res_status and summary.  INDEX: whether an index per candidate follows the
// coordinates in the temp.
#pragma once
#include "ransac_batch.hpp"
#include "resect_core.hpp"

template <class ArgsT, bool WITH_INDEX>
struct ResectModelOf {
  typedef ArgsT Args;
  static constexpr int SAMPLE = RESECT_SAMPLE, PARAMS = 12, COORDS = 5;
  static constexpr bool INDEX = WITH_INDEX, COUNT_ALL = true;
  template <class Ring>
  static __device__ __forceinline__ void draw(LibcRand<Ring> &g, const FastMod31 &fm, int (&p)[RESECT_SAMPLE])
  {
    resect_draw6(g, fm, p);
  }
  struct Lane {
    float k[4];                                // the image's intrinsics
  };
  static __device__ __forceinline__ Lane lane(const ArgsT &A, int e)
  {
    const float *kp = A.s.intrinsics + 4 * (size_t)A.images[e];
    return Lane{{kp[0], kp[1], kp[2], kp[3]}};
  }
  static __device__ __forceinline__ bool inlier(const float (&cam)[12], const Lane &ln, const float (&q)[5],
                                                float thresh2)
  {
    const float X[3] = {q[2], q[3], q[4]};
    return refine_member(cam, ln.k, X, q[0], q[1], thresh2);
  }
  static __device__ __forceinline__ float invalid() { return 0.0f; }
};

// a lane's 11 x 12 system in LDS: word (r, c) at (12 r + c) * 64 from the lane's base
struct ResectLdsMat {
  float *base;
  __device__ float get(int r, int c) const { return base[(RESECT_COLS * r + c) * 64]; }
  __device__ void set(int r, int c, float v) { base[(RESECT_COLS * r + c) * 64] = v; }
};

constexpr int RESECT_SOLVE_LDS = RESECT_ROWS * RESECT_COLS * 64;             // floats of a solve workgroup: 33 KiB

// The body of a solve kernel on 64-lane workgroups: s_m is the workgroup's RESECT_SOLVE_LDS floats.
template <class Model>
__device__ __forceinline__ void resect_solve_lane(const typename Model::Args &A, int hblocks, float *s_m)
{
  const RansacSearch &S = A.rs;
  int e, idx, n;
  if (!ransac_solve_begin(S, hblocks, e, idx, n)) return;
  const int mc = S.cap16;
  const float *coord = S.coord + (size_t)e * 5 * mc;
  float x[6], y[6], X[6], Y[6], Z[6];
  bool in_range = true;
#pragma unroll
  for (int k = 0; k < RESECT_SAMPLE; k++) {
    const int i = ransac_sample_position<Model>(S, e, idx, k, n, in_range);
    x[k] = coord[i]; y[k] = coord[mc + i]; X[k] = coord[2 * mc + i]; Y[k] = coord[3 * mc + i]; Z[k] = coord[4 * mc + i];
  }
  const typename Model::Lane ln = Model::lane(A, e);
  ResectLdsMat m{s_m + threadIdx.x};
  float cam[12];
  resect_solve6(m, x, y, X, Y, Z, ln.k, cam);
  ransac_store_hyp<Model>(S, e, idx, in_range, cam);
}

// Thread 0 of entry e's pick workgroup, behind ransac_pick: the entry's results, the install and the summary.  Returns the
// status; *picked gets the index of the picked hypothesis (status RESECT_OK only).
template <class Args>
__device__ __forceinline__ int resect_entry_results(const Args &A, int e, bool searched, unsigned long long best,
                                                    int *picked)
{
  const RansacSearch &S = A.rs;
  const int *meta = S.meta + (size_t)RANSAC_META * e;
  int status = meta[1], inliers = 0;
  float cam[12];
#pragma unroll
  for (int j = 0; j < 12; j++) cam[j] = 0.0f;
  if (searched) {
    inliers = ransac_pick_count(best);
    status = inliers < A.min_inliers ? RESECT_NO_MODEL : RESECT_OK;
    if (status == RESECT_OK) {
      const int idx = min(max(ransac_pick_index(best), 0), S.num_loops - 1);
      const float *hyp = S.hyp + (size_t)e * 12 * S.lp;
#pragma unroll
      for (int j = 0; j < 12; j++) cam[j] = pose_one_nan(hyp[j * S.lp + idx]);
      *picked = idx;
    }
  }
  float *out = A.res_cam + 12 * (size_t)e;
#pragma unroll
  for (int j = 0; j < 12; j++) out[j] = cam[j];
  A.res_cand[e] = meta[2];
  A.res_inliers[e] = inliers;
  A.res_status[e] = status;
  if (A.install && status == RESECT_OK) {
    const int img = A.images[e];
    float *dst = A.cam + 12 * (size_t)img;
#pragma unroll
    for (int j = 0; j < 12; j++) dst[j] = cam[j];
    A.cam_pair[img] = POSEGRAPH_RESECTED;
  }
  atomicAdd(&A.summary[status == RESECT_OK ? 1 : status + 2], 1);
  if (status == RESECT_OK) atomicAdd(&A.summary[2], inliers);
  return status;
}

// kernels_track_candidates.hip — the owner of every observation slot and the image it is a candidate of: the two
// launches of track_candidates.hpp, compiled here once for the calls that start with them.  Each kernel hands one work
// item to the function of triangulate_core.hpp that the host hooks run in loops.
#include "track_candidates.hpp"

namespace {

constexpr int CAND_THREADS = FUND_SLOTS;

__global__ __launch_bounds__(CAND_THREADS) void cand_owner_kernel(TrackScene S, int *owner)
{
  const int t = blockIdx.x * CAND_THREADS + threadIdx.x;     // below max_tracks + 256: no overflow
  if (t < scene_T(S)) scene_track_owns(S, owner, t);
}

__global__ __launch_bounds__(CAND_THREADS) void cand_key_kernel(TrackScene S, const int *owner, int *key)
{
  const int o = blockIdx.x * CAND_THREADS + threadIdx.x;
  if (o < scene_O(S)) key[o] = scene_slot_key(S, owner, o);
}

inline dim3 cand_blocks(int n) { return dim3((unsigned)(((long long)n + CAND_THREADS - 1) / CAND_THREADS)); }

}  // namespace

void launch_track_candidates(misift_ctx *ctx, const TrackScene &scene, int *owner, int *key)
{
  hipLaunchKernelGGL(cand_owner_kernel, cand_blocks(scene.max_tracks), dim3(CAND_THREADS), 0, ctx->stream, scene, owner);
  if (key)
    hipLaunchKernelGGL(cand_key_kernel, cand_blocks(scene.max_obs), dim3(CAND_THREADS), 0, ctx->stream, scene, owner, key);
}

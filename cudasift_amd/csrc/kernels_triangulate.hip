// kernels_triangulate.hip — misift_triangulate_tracks_batch: one N-view world point per exported track under the linked
// cameras, refined on reprojection error, and each observation's residual.  It joins the track chain (the observation
// lists of misift_export_tracks_batch) to the pose chain (the cameras of misift_link_poses_batch).  No reference
// counterpart.  The arithmetic is triangulate_core.hpp, shared with the host-only test hook at the end of this file.
//
// One memset (the summary) and one launch, whatever the data:
//   triangulate_tracks_kernel   256-thread workgroups, one lane per track, the grid sized from max_tracks.  T is read
//                               from the export summary on the device; a workgroup whose first track is at or beyond T
//                               leaves at once.  The others stage the cameras and intrinsics in LDS, 17 words per image
//                               (twelve of the camera, fx fy cx cy, and whether the image has a finite camera: the odd
//                               stride keeps neighbouring images on different banks), when nimages <= TRI_CAPACITY;
//                               beyond it every view reads d_cam, d_cam_pair and a device copy of the intrinsics from
//                               global memory.  A lane then runs tri_track on its track: the linear pass, the residual
//                               pass num_loops + 1 times at the most, and one more pass for d_obs_error.  A track's
//                               16-byte observations are read with one load each, the next one issued before the current
//                               view is worked on, and lie next to its neighbours', so the lanes of a wavefront share
//                               cache lines and the later passes find them in the L1 / L2.
//                               The summary is integer sums: a wavefront shuffle reduction, then one atomic per
//                               wavefront and non-zero entry.
// A several-lanes-per-track form for long tracks was not built: a track of the window chain has a handful of
// observations, and the summation order k ascending would force such a form into a serial combine anyway.
#include <stdint.h>
#include "common.hpp"
#include "triangulate_core.hpp"

namespace {

constexpr int TRI_THREADS = 256;
constexpr int TRI_CAPACITY = 512;              // images whose cameras and intrinsics are staged in LDS
constexpr int TRI_WORDS = 17;                  // per staged image

struct TriArgs {
  TrackScene s;                                // no points yet; intrinsics: the pinned host copy (staged) or its device
                                               // copy (beyond the capacity)
  int min_views, num_loops;
  float *points;
  int *point_views, *point_status;
  float *obs_error;                            // may be NULL
  int *summary;
};

// the LDS copy: 17 words per image
struct TriCamsStaged {
  const float *s;
  __device__ __forceinline__ const float *cam(int i) const { return s + TRI_WORDS * i; }
  __device__ __forceinline__ const float *k(int i) const { return s + TRI_WORDS * i + 12; }
  __device__ __forceinline__ bool set(int i) const { return s[TRI_WORDS * i + 16] != 0.0f; }
};

template <class Cams>
__device__ __forceinline__ int tri_lane(const TriArgs &A, const Cams &C, int t, int *views, int *kept)
{
  const int off = A.s.track_offsets[t], end = A.s.track_offsets[t + 1];
  float *point = A.points + 4 * (size_t)t;
  if (!tri_range_ok(off, end, A.s.max_obs)) {
    const float nan = pose_one_nan(NAN);
    point[0] = point[1] = point[2] = point[3] = nan;
    *views = 0;
    *kept = 0;
    return TRI_BAD_RANGE;
  }
  return tri_track(C, A.s.nimages, A.s.obs + off, end - off, A.min_views, A.num_loops, point, views,
                   A.obs_error ? A.obs_error + off : nullptr, kept);
}

__global__ __launch_bounds__(TRI_THREADS) void triangulate_tracks_kernel(TriArgs A)
{
  extern __shared__ __attribute__((aligned(16))) float s_cams[];
  const int tid = threadIdx.x;
  const int T = scene_T(A.s);
  if (blockIdx.x == 0 && tid == 0) A.summary[0] = T;
  const int first = blockIdx.x * TRI_THREADS;  // at most max_tracks - 1: no overflow
  if (first >= T) return;                      // the same in every thread
  const int nimages = A.s.nimages;
  const bool staged = nimages <= TRI_CAPACITY;
  if (staged) {
    for (int i = tid; i < 12 * nimages; i += TRI_THREADS) s_cams[TRI_WORDS * (i / 12) + i % 12] = A.s.cam[i];
    for (int i = tid; i < 4 * nimages; i += TRI_THREADS) s_cams[TRI_WORDS * (i >> 2) + 12 + (i & 3)] = A.s.intrinsics[i];
    __syncthreads();
    for (int i = tid; i < nimages; i += TRI_THREADS) {         // TriCamsPlain::set, once per image
      bool ok = A.s.cam_pair[i] != POSEGRAPH_UNSET;
      for (int j = 0; j < 12; j++) ok = ok && fundamental_finite(s_cams[TRI_WORDS * i + j]);
      s_cams[TRI_WORDS * i + 16] = ok ? 1.0f : 0.0f;
    }
    __syncthreads();
  }
  const int t = first + tid;
  int status = -1, views = 0, kept = 0;
  if (t < T) {
    // the two calls differ in nothing but where the cameras are read, and are kept apart so that the staged one compiles
    // to LDS instructions and not to flat ones
    if (staged) status = tri_lane(A, TriCamsStaged{s_cams}, t, &views, &kept);
    else status = tri_lane(A, TriCamsPlain{A.s.cam, A.s.cam_pair, A.s.intrinsics}, t, &views, &kept);
    A.point_views[t] = views;
    A.point_status[t] = status;
  }
  int v[7] = {status == TRI_OK, status == TRI_OK ? views : 0, status == TRI_FEW_VIEWS, status == TRI_SINGULAR,
              status == TRI_BEHIND, kept, status == TRI_BAD_RANGE};
#pragma unroll
  for (int j = 0; j < 7; j++) {
    for (int off = 32; off > 0; off >>= 1) v[j] += __shfl_xor(v[j], off, 64);
    if ((tid & 63) == 0 && v[j]) atomicAdd(&A.summary[1 + j], v[j]);
  }
}

}  // namespace

size_t triangulate_tracks_batch_tmp_bytes(int nimages)
{
  return nimages > TRI_CAPACITY ? sizeof(float) * 4 * (size_t)nimages : 0;
}

// Enqueue misift_triangulate_tracks_batch on the context stream (common.hpp): a memset and one launch; beyond the
// staging capacity a copy of the intrinsics into temp memory goes first.  scene.intrinsics: the pinned copy.
int launch_triangulate_tracks_batch(misift_ctx *ctx, const TrackScene &scene, int min_views, int num_loops,
                                    float *d_points, int *d_point_views, int *d_point_status, float *d_obs_error,
                                    int *d_summary)
{
  TriArgs A{scene, min_views, num_loops, d_points, d_point_views, d_point_status, d_obs_error, d_summary};
  const size_t tmp = triangulate_tracks_batch_tmp_bytes(scene.nimages);
  if (tmp) {
    const int rc = misift_ensure_tmp(ctx, tmp);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->d_match_tmp, scene.intrinsics, tmp, hipMemcpyHostToDevice, ctx->stream));
    A.s.intrinsics = reinterpret_cast<const float *>(ctx->d_match_tmp);
  }
  HIP_TRY(hipMemsetAsync(d_summary, 0, 8 * sizeof(int), ctx->stream));
  const size_t lds = tmp ? 0 : sizeof(float) * TRI_WORDS * (size_t)scene.nimages;
  const unsigned blocks = (unsigned)(((long long)scene.max_tracks + TRI_THREADS - 1) / TRI_THREADS);
  LaunchScope ls(ctx, "triangulate_tracks");
  hipLaunchKernelGGL(triangulate_tracks_kernel, dim3(blocks), dim3(TRI_THREADS), lds, ctx->stream, A);
  return ls.finish();
}

// Test-only, host-only: one track as a lane of the kernel computes it (triangulate_core.hpp), and the staging capacity.
extern "C" int misift_test_triangulate_capacity(void) { return TRI_CAPACITY; }

extern "C" int misift_test_triangulate_track(const float *cams, const int *cam_pair, const float *intrinsics,
                                             int nimages, const misift_track_obs *obs, int nobs, int min_views,
                                             int num_loops, float *point4, int *views, int *status, float *obs_error,
                                             int *gn_accepted)
{
  if (!cams || !cam_pair || !intrinsics || nimages < 1 || nobs < 0 || (nobs > 0 && !obs) || min_views < 2 ||
      num_loops < 0 || !point4 || !views || !status || !gn_accepted) {
    misift_set_error("misift_test_triangulate_track: invalid argument");
    return MISIFT_EINVAL;
  }
  *status = tri_track(TriCamsPlain{cams, cam_pair, intrinsics}, nimages, reinterpret_cast<const TrackObs *>(obs), nobs,
                      min_views, num_loops, point4, views, obs_error, gn_accepted);
  return MISIFT_OK;
}

// kernels_refine.hip — misift_refine_cameras_batch: every linked camera moved to minimise the reprojection error of the
// observations its image makes of the triangulated track points, the points held (motion-only bundle adjustment).  It
// is the other half of misift_triangulate_tracks_batch's minimisation; the two alternated are block-coordinate bundle
// adjustment.  No reference counterpart.  The arithmetic is refine_core.hpp, shared with the host-only test hook at the
// end of this file.
//
// Two memsets (the owners, the summary) and three launches, whatever the data:
//   cand_owner_kernel      the owner of every slot and
//   cand_key_kernel        the image every slot is a candidate of: launch_track_candidates (track_candidates.hpp).
//   refine_cameras_kernel  one 256-thread workgroup per image, thread s being slot s of the call's sum.  A pass walks the
//                          keys o = s, s + 256, ... < O with coalesced 4-byte loads, eight ahead; for a key that names its
//                          image the lane loads the owner, the 16-byte observation and the point, decides membership under
//                          the camera of step 1 (recomputed in every pass: some twenty operations, and no member list
//                          has to be kept anywhere), and adds the 28 terms in registers.  The tree runs through 28 KiB of
//                          LDS.  The solve and the update are a few hundred operations that every lane runs on the
//                          same values.  num_loops + 1 passes at the most; a workgroup reads O x 4 bytes of keys per
//                          pass, from the L2 after the first image has read them.
// Not built: member lists kept in LDS after the first pass, and a form that spreads the terms of an image
// whose slots fall into a few lanes over all lanes before they are added in the order of the sum.
#include <stdint.h>
#include <string.h>
#include "common.hpp"
#include "refine_core.hpp"
#include "track_candidates.hpp"

namespace {

constexpr int REFINE_THREADS = FUND_SLOTS;
constexpr int REFINE_AHEAD = 8;                // slot keys a lane loads before it looks at the first

struct RefineArgs {
  int min_obs, num_loops, orthonormalise;
  float thresh2;
  TrackScene s;                                // intrinsics: the pinned host copy
  const int *owner, *key;                      // temp: max_obs each
  const int *held;                             // the pinned host copy: nimages flags
  float *cam_out;
  int *cam_obs;
  float *cam_rms;
  int *cam_steps, *cam_status, *summary;
};

// the workgroup as the Exec of refine_camera
struct RefineBlockExec {
  const RefineArgs &A;
  float *p;                                    // LDS: REFINE_SUMS x FUND_SLOTS
  int *cnt;                                    // LDS: 8 ints
  int image, O;
  const float *k;                              // fx fy cx cy in registers

  // slot o, known to be a candidate of this image: false when it is no member; its terms, or `behind`
  __device__ __forceinline__ bool terms(int o, const float (&cam1)[12], const float (&cam)[12], float thresh2,
                                        float (&x)[REFINE_SUMS], int &n, bool &behind) const
  {
    const float *P = A.s.points + 4 * (size_t)A.owner[o];
    const TrackObs ob = track_obs_load(A.s.obs + o);
    const float X[3] = {P[0], P[1], P[2]};
    if (!refine_member(cam1, k, X, ob.xpos, ob.ypos, thresh2)) return false;
    n++;
    if (refine_terms(cam, k, X, ob.xpos, ob.ypos, x)) return true;
    behind = true;
    return false;
  }

  __device__ void pass(const float (&cam1)[12], const float (&cam)[12], float thresh2, float (&S)[REFINE_SUMS], int &n,
                       bool &behind)
  {
    const int t = threadIdx.x;
    int mine = 0;
    bool back = false;
    // slot t's partial sums as fundamental_slot_partial forms them: the members o = t, t + 256, ... in ascending order
    // from +0.  The keys of REFINE_AHEAD slots are loaded before the first is looked at: a load per iteration left the
    // walk waiting on each in turn.
    float acc[REFINE_SUMS];
#pragma unroll
    for (int j = 0; j < REFINE_SUMS; j++) acc[j] = 0.0f;
    for (long long base = t; base < O; base += (long long)REFINE_AHEAD * FUND_SLOTS) {
      int key[REFINE_AHEAD];
#pragma unroll
      for (int u = 0; u < REFINE_AHEAD; u++) {
        const long long o = base + u * FUND_SLOTS;
        key[u] = o < O ? A.key[o] : -1;
      }
#pragma unroll
      for (int u = 0; u < REFINE_AHEAD; u++) {
        if (key[u] != image) continue;
        float x[REFINE_SUMS];
        if (!terms((int)(base + u * FUND_SLOTS), cam1, cam, thresh2, x, mine, back)) continue;
#pragma unroll
        for (int j = 0; j < REFINE_SUMS; j++) acc[j] = acc[j] + x[j];
      }
    }
#pragma unroll
    for (int j = 0; j < REFINE_SUMS; j++) p[j * FUND_SLOTS + t] = acc[j];
    int c = mine, b = back ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) {
      c += __shfl_xor(c, off, 64);
      b |= __shfl_xor(b, off, 64);
    }
    if ((t & 63) == 0) {
      cnt[t >> 6] = c;
      cnt[4 + (t >> 6)] = b;
    }
    for (int off = FUND_SLOTS / 2; off > 0; off >>= 1) {
      __syncthreads();
      if (t < off) fundamental_tree_step<REFINE_SUMS>(p, t, off);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < REFINE_SUMS; j++) S[j] = p[j * FUND_SLOTS];
    n = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    behind = (cnt[4] | cnt[5] | cnt[6] | cnt[7]) != 0;
    __syncthreads();                           // p and cnt are free again
  }
};

__global__ __launch_bounds__(REFINE_THREADS) void refine_cameras_kernel(RefineArgs A)
{
  __shared__ float s_p[REFINE_SUMS * FUND_SLOTS];
  __shared__ int s_cnt[8];
  const int i = blockIdx.x, tid = threadIdx.x;
  if (i == 0 && tid == 0) A.summary[0] = scene_T(A.s);
  const unsigned *bits = reinterpret_cast<const unsigned *>(A.s.cam) + 12 * (size_t)i;
  unsigned given[12];
  float cam_in[12];
#pragma unroll
  for (int j = 0; j < 12; j++) {
    given[j] = bits[j];
    cam_in[j] = __uint_as_float(given[j]);
  }
  const int pair = A.s.cam_pair[i];
  const float *kp = A.s.intrinsics + 4 * (size_t)i;
  const float k[4] = {kp[0], kp[1], kp[2], kp[3]};
  const bool fixed = pair == POSEGRAPH_ROOT || A.held[i] != 0;
  RefineBlockExec ex{A, s_p, s_cnt, i, scene_O(A.s), k};
  RefineResult r;
  refine_camera(ex, cam_in, pair == POSEGRAPH_UNSET, fixed, k, A.orthonormalise, A.min_obs, A.num_loops, A.thresh2, r);
  if (tid != 0) return;                        // every thread holds the same result; the input was read above
  unsigned *out = reinterpret_cast<unsigned *>(A.cam_out) + 12 * (size_t)i;
#pragma unroll
  for (int j = 0; j < 12; j++) out[j] = r.as_given ? given[j] : __float_as_uint(r.cam[j]);
  A.cam_obs[i] = r.nobs;
  A.cam_rms[2 * (size_t)i] = r.rms0;
  A.cam_rms[2 * (size_t)i + 1] = r.rms1;
  A.cam_steps[i] = r.steps;
  A.cam_status[i] = r.status;
  atomicAdd(&A.summary[r.status == REFINE_OK ? 1 : r.status == REFINE_NO_CAMERA ? 7 : r.status + 2], 1);
  if (r.status == REFINE_OK && r.nobs) atomicAdd(&A.summary[2], r.nobs);
  if (r.steps) atomicAdd(&A.summary[6], r.steps);
}

}  // namespace

size_t refine_cameras_batch_tmp_bytes(int max_obs) { return 2 * sizeof(int) * (size_t)max_obs; }

// Enqueue misift_refine_cameras_batch on the context stream (common.hpp): two memsets and three launches.
int launch_refine_cameras_batch(misift_ctx *ctx, const TrackScene &scene, const int *h_held, int min_obs, int num_loops,
                                float thresh2, int orthonormalise, float *d_cam_out, int *d_cam_obs, float *d_cam_rms,
                                int *d_cam_steps, int *d_cam_status, int *d_summary)
{
  const int rc = misift_ensure_tmp(ctx, refine_cameras_batch_tmp_bytes(scene.max_obs));
  if (rc) return rc;
  int *owner = reinterpret_cast<int *>(ctx->d_match_tmp), *key = owner + scene.max_obs;
  const RefineArgs A{min_obs, num_loops, orthonormalise, thresh2, scene, owner, key, h_held, d_cam_out, d_cam_obs,
                     d_cam_rms, d_cam_steps, d_cam_status, d_summary};
  HIP_TRY(hipMemsetAsync(owner, 0xff, sizeof(int) * (size_t)scene.max_obs, ctx->stream));
  HIP_TRY(hipMemsetAsync(d_summary, 0, 8 * sizeof(int), ctx->stream));
  LaunchScope ls(ctx, "refine_cameras");
  launch_track_candidates(ctx, scene, owner, key);
  hipLaunchKernelGGL(refine_cameras_kernel, dim3(scene.nimages), dim3(REFINE_THREADS), 0, ctx->stream, A);
  return ls.finish();
}

// Test-only, host-only: one image as its workgroup computes it (refine_core.hpp).
extern "C" int misift_test_refine_camera(const float *cam12, int cam_pair, int held, const float *intrinsics4, int ncand,
                                         const int *slot, const float *X, const float *xy, int min_obs, int num_loops,
                                         float max_error, int orthonormalise, float *cam_out12, int *nobs, float *rms2,
                                         int *steps, int *status)
{
  bool ok = cam12 && intrinsics4 && ncand >= 0 && (ncand == 0 || (slot && X && xy)) && min_obs >= 3 && num_loops >= 0 &&
            max_error > 0.0f && (orthonormalise == 0 || orthonormalise == 1) && cam_out12 && nobs && rms2 && steps && status;
  for (int i = 0; ok && i < ncand; i++) ok = slot[i] >= 0 && (i == 0 || slot[i] > slot[i - 1]);
  if (!ok) {
    misift_set_error("misift_test_refine_camera: invalid argument");
    return MISIFT_EINVAL;
  }
  float cam_in[12];
  memcpy(cam_in, cam12, sizeof cam_in);
  RefineHostExec ex;
  ex.ncand = ncand; ex.slot = slot; ex.X = X; ex.xy = xy; ex.k = intrinsics4;
  RefineResult r;
  refine_camera(ex, cam_in, cam_pair == POSEGRAPH_UNSET, cam_pair == POSEGRAPH_ROOT || held != 0, intrinsics4,
                orthonormalise, min_obs, num_loops, max_error * max_error, r);
  if (r.as_given) memmove(cam_out12, cam12, 12 * sizeof(float));
  else memcpy(cam_out12, r.cam, 12 * sizeof(float));
  *nobs = r.nobs;
  rms2[0] = r.rms0; rms2[1] = r.rms1;
  *steps = r.steps;
  *status = r.status;
  return MISIFT_OK;
}

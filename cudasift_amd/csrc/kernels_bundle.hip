// kernels_bundle.hip — misift_adjust_bundle_batch: Levenberg-Marquardt over all free cameras and all active track points
// at once.  Each step eliminates the points (Schur complement), solves the reduced camera system matrix-free by a fixed
// number of block-Jacobi preconditioned conjugate-gradient iterations, back-substitutes the points and is kept or turned
// away on the device.  No reference counterpart.  The arithmetic is bundle_core.hpp: every kernel here is a few lines
// that hand one work item to the function of its phase, the same function the host-only test hook (bundle_host.hpp,
// wrapped at the end of this file) runs in a loop.
//
// Three memsets (the owners, the control words, the summary) and 11 + num_loops * (8 + 3 * cg_iters) launches, whatever
// the data.  A dispatch boundary is the only barrier between workgroups: nothing in here waits for another workgroup.
//   cand_owner_kernel, cand_key_kernel     launch_track_candidates: the owner of every slot, the image it is a candidate of
//   bundle_image_init_kernel    lane per image: usable / held / free, the camera of refine's step 1 into both buffers
//   bundle_premember_kernel     lane per slot: refine's member test under that camera
//   bundle_activate_kernel      lane per track: its pre-members counted; an inactive track's leave the keys
//   bundle_gather_kernel        256-thread workgroup per image, two walks over the keys: the members of lower images
//                               counted (the start of its list), then its members listed in ascending slot (ballot and
//                               popcount keep the order, as resect's gather); demotion
//   bundle_eval_kernel          lane per slot: a member's squared residual under a state buffer
//   bundle_cost_kernel          workgroup per image: its cost by the position rule
//   bundle_start_kernel         the scalar workgroup: the cost of the start, lambda0
//   per LM step:
//   bundle_track_normal_kernel  lane per track: Jc, Jp, r of its members into temp, V, gp, V', V'^-1 gp
//   bundle_image_normal_kernel  workgroup per image: U, gc, sum W y (33 sums, 33 KiB of LDS), U', b, the LDL^T checked
//   bundle_cg_start_kernel      the scalar workgroup: x, r, z, p, rho
//   per CG iteration: bundle_cg_track_kernel (lane per track), bundle_cg_image_kernel (workgroup per image, 6 sums),
//                     bundle_cg_scalar_kernel (the scalar workgroup)
//   bundle_track_trial_kernel, bundle_image_trial_kernel   lane per track / per image: the trial state
//   bundle_eval_kernel, bundle_cost_kernel                 under the trial state
//   bundle_decide_kernel        the scalar workgroup: kept or not, lambda, the history
//   then bundle_image_out_kernel and bundle_track_out_kernel write the outputs.
// misift_adjust_bundle_robust_batch is the same sequence with a loss (bundle_loss): bundle_track_normal_kernel<true>
// scales a member's 20 values by sqrt(w) where it writes them and bundle_eval_kernel<true> stores rho; the plain call
// launches the <false> instances, which hold no trace of the loss.  With d_obs_weight one launch more at the end,
//   bundle_weight_out_kernel    lane per slot: w of a member under the final state, -1 for any other slot
// misift_adjust_bundle_focal_batch adds one focal scale per camera group to the unknowns.  Without a grouped image it
// is the sequence above and one launch more at the end (bundle_focal_out_kernel: d_intrinsics_out and d_focal).  With
// one, every phase that reads the scale has a FOCAL instance beside the plain one, which holds no trace of it:
//   bundle_focal_init_kernel          the scalar workgroup, behind the gather: s_g = 1, the members of every group
//   bundle_eval_kernel<.., true>, bundle_weight_out_focal_kernel   the member projected with fx*s_g, fy*s_g
//   bundle_track_normal_focal_kernel  Juf, Jvf of every member beside the 20 values; per group w_gt . V'^-1 w_gt
//   bundle_image_normal_focal_kernel  42 sums (42 KiB of LDS): the 33, U_cf, Uff, gf, wf . y_t
//   bundle_cg_start_focal_kernel      per group the cross-image sums U_gg, g_g and the cross-track sum of the Schur
//                                     scalar S_gg, in the scalar workgroup one group after another
//   bundle_cg_track/_image/_scalar_focal_kernel   the focal terms of the gather, of y_i, and y_g; 7 sums per image
//   bundle_track_trial_focal_kernel, bundle_image_trial_focal_kernel   the trial point; the trial camera and scale
// so 13 + num_loops * (8 + 3 * cg_iters) launches: the two more are the groups' members and the two new outputs.
// misift_adjust_bundle_radial_batch adds one radial coefficient per camera group, applied to the observation.  With
// nothing radial (no grouped image, or no unknown coefficient and every start zero) it is the focal call's sequence and
// one launch more at the end (bundle_radial_out_kernel: d_radial).  Otherwise a RADIAL instance stands where the FOCAL
// one stood, launch for launch:
//   bundle_premember_radial_kernel, bundle_eval_kernel<.., true, true>, bundle_weight_out_radial_kernel
//                                      the observation enters as (x', y') under k_g (the member test: under k0)
//   bundle_radial_init_kernel          bundle_focal_init_kernel, and k_g = k0_g in both state buffers
//   bundle_track_normal_radial_kernel  the column Juk, Jvk of every member beside Juf, Jvf; per group wk_gt . V'^-1 wk_gt,
//                                      the wk_gt from a walk of their own in the registers of the w_gt (no scratch)
//   bundle_image_normal_radial_kernel  52 sums (52 KiB of LDS): the 42, U_ck, Ukk, gk, wk . y_t, Ufk
//   bundle_cg_start/_track/_image/_scalar_radial_kernel   S_kk and U_fk per group; the terms of k_g in the gather, in
//                                      y_i, y_g and y_k; 8 sums per image
//   bundle_track_trial_radial_kernel, bundle_image_trial_radial_kernel   the trial point; the trial camera, scale and k_g
// so 14 + num_loops * (8 + 3 * cg_iters) launches.  misift_undistort_obs_batch is undistort_obs_kernel alone.
// The host's side (the temp layout and the test hooks' body) is bundle_host.hpp.
// Jc, Jp and r are written once per LM step and read by both views: recomputing them in each CG pass instead gives the
// same bits and measured 10 to 13 % slower.
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "common.hpp"
#include "bundle_core.hpp"
#include "bundle_host.hpp"
#include "track_candidates.hpp"

namespace {

constexpr int BUNDLE_THREADS = FUND_SLOTS;

// the workgroup as the Sum of bundle_core.hpp: thread s is slot s, the tree runs through LDS
struct BundleBlockSum {
  float *p;                                    // LDS: K x FUND_SLOTS
  __device__ void fence() { __syncthreads(); }
  template <int K, class V>
  __device__ void sum(int n, V &v, float (&out)[K])
  {
    const int t = threadIdx.x;
    float acc[K];
    fundamental_slot_partial<K>(t, n, v, acc);
#pragma unroll
    for (int k = 0; k < K; k++) p[k * FUND_SLOTS + t] = acc[k];
    for (int off = FUND_SLOTS / 2; off > 0; off >>= 1) {
      __syncthreads();
      if (t < off) fundamental_tree_step<K>(p, t, off);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) out[k] = p[k * FUND_SLOTS];
    __syncthreads();                           // p is free again
  }
};

inline dim3 bundle_blocks(int n) { return dim3((unsigned)(((long long)n + BUNDLE_THREADS - 1) / BUNDLE_THREADS)); }

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_image_init_kernel(BundleData D)
{
  const int i = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (i < D.s.nimages) bundle_image_init(D, i);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_premember_kernel(BundleData D)
{
  const int o = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (o < scene_O(D.s)) bundle_slot_premember(D, o);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_activate_kernel(BundleData D)
{
  const int t = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (t < scene_T(D.s)) bundle_track_activate(D, t);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_gather_kernel(BundleData D)
{
  __shared__ int wave_cnt[2][4];
  __shared__ int base_s[2];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int O = scene_O(D.s);
  // first walk: the members of lower images come first in `list`, so count them, and this image's own
  int mine = 0, lower = 0;
  for (long long o = tid; o < O; o += BUNDLE_THREADS) {
    const int key = D.key[o];
    mine += key == i ? 1 : 0;
    lower += (key >= 0 && key < i) ? 1 : 0;
  }
  for (int off = 32; off > 0; off >>= 1) {
    mine += __shfl_xor(mine, off, 64);
    lower += __shfl_xor(lower, off, 64);
  }
  if (lane == 0) {
    wave_cnt[0][wave] = mine;
    wave_cnt[1][wave] = lower;
  }
  __syncthreads();
  const int n = wave_cnt[0][0] + wave_cnt[0][1] + wave_cnt[0][2] + wave_cnt[0][3];
  const int start = wave_cnt[1][0] + wave_cnt[1][1] + wave_cnt[1][2] + wave_cnt[1][3];   // start + n <= O
  if (tid == 0) base_s[0] = 0;
  __syncthreads();
  // second walk: the image's members in ascending slot; ballot and popcount keep the order
  for (long long o0 = 0; o0 < O; o0 += BUNDLE_THREADS) {
    const long long o = o0 + tid;
    const bool ok = o < O && D.key[o] == i;
    const unsigned long long m = __ballot(ok);
    if (lane == 0) wave_cnt[0][wave] = __popcll(m);
    __syncthreads();
    int pos = base_s[0];
    for (int w = 0; w < wave; w++) pos += wave_cnt[0][w];
    pos += __popcll(m & ((1ull << lane) - 1ull));
    if (ok && pos < n) D.list[start + pos] = (int)o;
    __syncthreads();
    if (tid == 0) base_s[0] += wave_cnt[0][0] + wave_cnt[0][1] + wave_cnt[0][2] + wave_cnt[0][3];
    __syncthreads();
  }
  if (tid == 0) {
    D.icount[i] = n;
    D.istart[i] = start;
    if (D.istate[i] == BUNDLE_ADJUSTED && n < D.min_obs) D.istate[i] = BUNDLE_FEW_OBS;
  }
}

template <bool ROBUST, bool FOCAL = false, bool RADIAL = false>
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_eval_kernel(BundleData D, int trial)
{
  const int o = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (o < scene_O(D.s)) bundle_eval_slot<ROBUST, FOCAL, RADIAL>(D, o, trial != 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_cost_kernel(BundleData D, int trial)
{
  __shared__ float s_p[FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_image_cost(D, S, blockIdx.x, trial != 0, threadIdx.x == 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_start_kernel(BundleData D)
{
  __shared__ float s_p[FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_scalar_init(D, S, threadIdx.x == 0);
}

template <bool ROBUST>
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_track_normal_kernel(BundleData D)
{
  const int t = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (t < scene_T(D.s)) bundle_track_normal<ROBUST>(D, t);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_image_normal_kernel(BundleData D)
{
  __shared__ float s_p[BUNDLE_NORMAL * FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_image_normal(D, S, blockIdx.x, threadIdx.x == 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_cg_start_kernel(BundleData D)
{
  __shared__ float s_p[FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_cg_start(D, S, threadIdx.x, BUNDLE_THREADS, threadIdx.x == 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_cg_track_kernel(BundleData D)
{
  const int t = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (t < scene_T(D.s)) bundle_cg_track(D, t);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_cg_image_kernel(BundleData D)
{
  __shared__ float s_p[6 * FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_cg_image(D, S, blockIdx.x, threadIdx.x == 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_cg_scalar_kernel(BundleData D)
{
  __shared__ float s_p[FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_cg_scalar(D, S, threadIdx.x, BUNDLE_THREADS, threadIdx.x == 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_track_trial_kernel(BundleData D)
{
  const int t = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (t < scene_T(D.s)) bundle_track_trial(D, t);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_image_trial_kernel(BundleData D)
{
  const int i = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (i < D.s.nimages) bundle_image_trial(D, i);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_decide_kernel(BundleData D)
{
  __shared__ float s_p[FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_decide(D, S, threadIdx.x, BUNDLE_THREADS, threadIdx.x == 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_image_out_kernel(BundleData D)
{
  const int i = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (i < D.s.nimages) bundle_image_out(D, i);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_track_out_kernel(BundleData D)
{
  const int t = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (t < scene_T(D.s)) bundle_track_out(D, t);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_weight_out_kernel(BundleData D)
{
  const int o = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (o < scene_O(D.s)) bundle_weight_slot(D, o);
}

// ---- misift_adjust_bundle_focal_batch: the FOCAL instances of the phases that read the focal scale, and the few
// kernels of its own

template <bool ROBUST>
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_track_normal_focal_kernel(BundleData D)
{
  const int t = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (t < scene_T(D.s)) bundle_track_normal_focal<ROBUST>(D, t);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_focal_init_kernel(BundleData D)
{
  BundleBlockSum S{nullptr};
  bundle_focal_init(D, S, threadIdx.x, BUNDLE_THREADS);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_image_normal_focal_kernel(BundleData D)
{
  __shared__ float s_p[BUNDLE_NORMAL_FOCAL * FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_image_normal_focal(D, S, blockIdx.x, threadIdx.x == 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_cg_start_focal_kernel(BundleData D)
{
  __shared__ float s_p[3 * FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_cg_start<true>(D, S, threadIdx.x, BUNDLE_THREADS, threadIdx.x == 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_cg_track_focal_kernel(BundleData D)
{
  const int t = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (t < scene_T(D.s)) bundle_cg_track<true>(D, t);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_cg_image_focal_kernel(BundleData D)
{
  __shared__ float s_p[7 * FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_cg_image_focal(D, S, blockIdx.x, threadIdx.x == 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_cg_scalar_focal_kernel(BundleData D)
{
  __shared__ float s_p[2 * FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_cg_scalar<true>(D, S, threadIdx.x, BUNDLE_THREADS, threadIdx.x == 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_track_trial_focal_kernel(BundleData D)
{
  const int t = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (t < scene_T(D.s)) bundle_track_trial<true>(D, t);
}

// lane per image: its trial camera; the first BUNDLE_MAX_GROUPS lanes of the launch: the trial scale of a group
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_image_trial_focal_kernel(BundleData D)
{
  const int i = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (i < D.s.nimages) bundle_image_trial(D, i);
  if (i < BUNDLE_MAX_GROUPS) bundle_focal_trial(D, i);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_weight_out_focal_kernel(BundleData D)
{
  const int o = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (o < scene_O(D.s)) bundle_weight_slot<true>(D, o);
}

// lane per image: d_intrinsics_out; the first ngroups lanes of the launch: d_focal
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_focal_out_kernel(BundleData D, int refined)
{
  const int i = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (i < D.s.nimages) bundle_intrinsics_out(D, i, refined != 0);
  if (i < D.ngroups) bundle_focal_out(D, i, refined != 0);
}

// ---- misift_adjust_bundle_radial_batch: the RADIAL instances of the phases that read an observation or carry a
// scalar, beside the plain and the FOCAL ones, which hold no trace of the coefficient

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_premember_radial_kernel(BundleData D)
{
  const int o = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (o < scene_O(D.s)) bundle_slot_premember<true>(D, o);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_radial_init_kernel(BundleData D)
{
  BundleBlockSum S{nullptr};
  bundle_focal_init<true>(D, S, threadIdx.x, BUNDLE_THREADS);
}

template <bool ROBUST>
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_track_normal_radial_kernel(BundleData D)
{
  const int t = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (t < scene_T(D.s)) bundle_track_normal_focal<ROBUST, true>(D, t);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_image_normal_radial_kernel(BundleData D)
{
  __shared__ float s_p[BUNDLE_NORMAL_RADIAL * FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_image_normal_radial(D, S, blockIdx.x, threadIdx.x == 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_cg_start_radial_kernel(BundleData D)
{
  __shared__ float s_p[4 * FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_cg_start<true, true>(D, S, threadIdx.x, BUNDLE_THREADS, threadIdx.x == 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_cg_track_radial_kernel(BundleData D)
{
  const int t = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (t < scene_T(D.s)) bundle_cg_track<true, true>(D, t);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_cg_image_radial_kernel(BundleData D)
{
  __shared__ float s_p[8 * FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_cg_image_radial(D, S, blockIdx.x, threadIdx.x == 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_cg_scalar_radial_kernel(BundleData D)
{
  __shared__ float s_p[2 * FUND_SLOTS];
  BundleBlockSum S{s_p};
  bundle_cg_scalar<true, true>(D, S, threadIdx.x, BUNDLE_THREADS, threadIdx.x == 0);
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_track_trial_radial_kernel(BundleData D)
{
  const int t = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (t < scene_T(D.s)) bundle_track_trial<true, true>(D, t);
}

// lane per image: its trial camera; the first BUNDLE_MAX_GROUPS lanes: the trial scale and coefficient of a group
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_image_trial_radial_kernel(BundleData D)
{
  const int i = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (i < D.s.nimages) bundle_image_trial(D, i);
  if (i < BUNDLE_MAX_GROUPS) {
    bundle_focal_trial(D, i);
    bundle_radial_trial(D, i);
  }
}

__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_weight_out_radial_kernel(BundleData D)
{
  const int o = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (o < scene_O(D.s)) bundle_weight_slot<true, true>(D, o);
}

// the first ngroups lanes: d_radial
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_radial_out_kernel(BundleData D, int refined, int radial)
{
  const int g = threadIdx.x;
  if (g < D.ngroups) bundle_radial_out(D, g, refined != 0, radial != 0);
}

// misift_undistort_obs_batch: lane per slot, one 16-byte load and one 16-byte store
__global__ __launch_bounds__(BUNDLE_THREADS) void undistort_obs_kernel(int max_obs, const TrackObs *obs,
                                                                       const int *export_summary, int nimages,
                                                                       const float *intrinsics, const int *group,
                                                                       const int *radial, TrackObs *out)
{
  const long long o = (long long)blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  const int O = scene_clamp(export_summary[3], max_obs);
  if (o >= O) return;
  const TrackObs ob = bundle_undistort_obs(track_obs_load(obs + o), nimages, intrinsics, group, radial);
  reinterpret_cast<int4 *>(out)[o] = make_int4(ob.frame, ob.record, __float_as_int(ob.xpos), __float_as_int(ob.ypos));
}

}  // namespace

size_t adjust_bundle_batch_tmp_bytes(int max_tracks, int max_obs, int nimages)
{
  BundleData D;
  D.s.max_tracks = max_tracks; D.s.max_obs = max_obs; D.s.nimages = nimages;
  return bundle_layout(D, nullptr);
}

size_t adjust_bundle_focal_batch_tmp_bytes(int max_tracks, int max_obs, int nimages)
{
  BundleData D;
  D.s.max_tracks = max_tracks; D.s.max_obs = max_obs; D.s.nimages = nimages;
  return bundle_layout(D, nullptr, true);
}

size_t adjust_bundle_radial_batch_tmp_bytes(int max_tracks, int max_obs, int nimages)
{
  BundleData D;
  D.s.max_tracks = max_tracks; D.s.max_obs = max_obs; D.s.nimages = nimages;
  return bundle_layout(D, nullptr, true, true);
}

// Enqueue misift_adjust_bundle_robust_batch on the context stream (common.hpp); misift_adjust_bundle_batch is loss 0 and
// no d_obs_weight.
int launch_adjust_bundle_batch(misift_ctx *ctx, const TrackScene &scene, const int *h_held, int min_views, int min_obs,
                               int num_loops, int cg_iters, float thresh2, float lambda0, int orthonormalise, int loss,
                               float loss_scale, float loss_scale2, float *d_cam_out, float *d_points_out, int *d_cam_obs,
                               int *d_cam_status, float *d_cam_rms, int *d_point_obs, float *d_history, float *d_cost,
                               float *d_obs_weight, int *d_summary)
{
  return launch_adjust_bundle_focal_batch(ctx, scene, h_held, min_views, min_obs, num_loops, cg_iters, thresh2, lambda0,
                                          orthonormalise, loss, loss_scale, loss_scale2, 0, nullptr, false, d_cam_out,
                                          d_points_out, d_cam_obs, d_cam_status, d_cam_rms, d_point_obs, d_history, d_cost,
                                          d_obs_weight, d_summary, nullptr, nullptr);
}

// Enqueue misift_adjust_bundle_focal_batch.  focal: an image has a group, so the FOCAL instances run, with one launch
// more in the setup (the groups' members) and the wider temp; otherwise the launches are those of the robust call.  With
// d_intrinsics_out one launch more at the end writes it and d_focal; the two existing calls pass NULL.
// misift_adjust_bundle_radial_batch is the same sequence: R (NULL in the focal call) has the pinned copies of `radial`
// and `k0`, d_radial, and `on`: an image has a group and some k_g is an unknown or starts off zero, so the RADIAL
// instances run in place of the FOCAL ones, launch for launch.  One launch more at the end writes d_radial.
struct BundleRadialArgs {
  const int *h_radial;
  const float *h_k0;
  bool on;
  int *d_radial;
};
static int bundle_launch(misift_ctx *ctx, const TrackScene &scene, const int *h_held, int min_views, int min_obs,
                         int num_loops, int cg_iters, float thresh2, float lambda0, int orthonormalise, int loss,
                         float loss_scale, float loss_scale2, int ngroups, const int *h_group, bool focal,
                         float *d_cam_out, float *d_points_out, int *d_cam_obs, int *d_cam_status, float *d_cam_rms,
                         int *d_point_obs, float *d_history, float *d_cost, float *d_obs_weight, int *d_summary,
                         float *d_intrinsics_out, int *d_focal, const BundleRadialArgs *R)
{
  const int max_tracks = scene.max_tracks, max_obs = scene.max_obs, nimages = scene.nimages;
  const bool radial = R && R->on;
  const int rc = misift_ensure_tmp(ctx, radial  ? adjust_bundle_radial_batch_tmp_bytes(max_tracks, max_obs, nimages)
                                        : focal ? adjust_bundle_focal_batch_tmp_bytes(max_tracks, max_obs, nimages)
                                                : adjust_bundle_batch_tmp_bytes(max_tracks, max_obs, nimages));
  if (rc) return rc;
  BundleData D;
  if (R) {
    D.rad = R->h_radial; D.k0 = R->h_k0; D.radial_out = R->d_radial;
  }
  D.ngroups = ngroups; D.grp = h_group; D.intrinsics_out = d_intrinsics_out; D.focal_out = d_focal;
  D.s = scene; D.min_views = min_views; D.min_obs = min_obs;
  D.num_loops = num_loops; D.cg_iters = cg_iters; D.orthonormalise = orthonormalise; D.thresh2 = thresh2;
  D.lambda0 = lambda0;
  D.loss = loss; D.loss_scale = loss_scale; D.loss_scale2 = loss_scale2;
  D.held = h_held;
  bundle_layout(D, reinterpret_cast<char *>(ctx->d_match_tmp), focal, radial);
  D.cam_out = d_cam_out; D.points_out = d_points_out; D.cam_rms = d_cam_rms; D.history = d_history; D.cost = d_cost;
  D.cam_obs = d_cam_obs; D.cam_status = d_cam_status; D.point_obs = d_point_obs; D.summary = d_summary;
  D.obs_weight = d_obs_weight;
  HIP_TRY(hipMemsetAsync(D.owner, 0xff, sizeof(int) * (size_t)max_obs, ctx->stream));
  HIP_TRY(hipMemsetAsync(D.ctl, 0, sizeof(int) * BUNDLE_CTL, ctx->stream));
  HIP_TRY(hipMemsetAsync(d_summary, 0, 8 * sizeof(int), ctx->stream));
  hipStream_t s = ctx->stream;
  const dim3 th(BUNDLE_THREADS), per_track = bundle_blocks(max_tracks), per_slot = bundle_blocks(max_obs),
             per_image = bundle_blocks(nimages), image_wg((unsigned)nimages), one(1);
  // a profile entry per kind of launch (misift_profile_read): tools/bundle_time.py reports their shares
  auto scope = [&](const char *name, auto launches) {
    LaunchScope ls(ctx, name);
    launches();
    return ls.finish();
  };
  // the loss is the same for the whole call: the two kernels that read it are picked here
  const bool robust = loss != BUNDLE_LOSS_NONE;
  auto eval = [&](int trial) {
    if (radial && robust) hipLaunchKernelGGL((bundle_eval_kernel<true, true, true>), per_slot, th, 0, s, D, trial);
    else if (radial) hipLaunchKernelGGL((bundle_eval_kernel<false, true, true>), per_slot, th, 0, s, D, trial);
    else if (focal && robust) hipLaunchKernelGGL((bundle_eval_kernel<true, true>), per_slot, th, 0, s, D, trial);
    else if (focal) hipLaunchKernelGGL((bundle_eval_kernel<false, true>), per_slot, th, 0, s, D, trial);
    else if (robust) hipLaunchKernelGGL(bundle_eval_kernel<true>, per_slot, th, 0, s, D, trial);
    else hipLaunchKernelGGL(bundle_eval_kernel<false>, per_slot, th, 0, s, D, trial);
  };
  auto track_normal = [&] {
    if (radial && robust) hipLaunchKernelGGL(bundle_track_normal_radial_kernel<true>, per_track, th, 0, s, D);
    else if (radial) hipLaunchKernelGGL(bundle_track_normal_radial_kernel<false>, per_track, th, 0, s, D);
    else if (focal && robust) hipLaunchKernelGGL(bundle_track_normal_focal_kernel<true>, per_track, th, 0, s, D);
    else if (focal) hipLaunchKernelGGL(bundle_track_normal_focal_kernel<false>, per_track, th, 0, s, D);
    else if (robust) hipLaunchKernelGGL(bundle_track_normal_kernel<true>, per_track, th, 0, s, D);
    else hipLaunchKernelGGL(bundle_track_normal_kernel<false>, per_track, th, 0, s, D);
  };
  // a phase that reads the focal scale has a FOCAL instance; the plain one holds no trace of it
  auto pick = [&](auto plain, auto with_focal, auto with_radial, dim3 grid) {
    if (radial) hipLaunchKernelGGL(with_radial, grid, th, 0, s, D);
    else if (focal) hipLaunchKernelGGL(with_focal, grid, th, 0, s, D);
    else hipLaunchKernelGGL(plain, grid, th, 0, s, D);
  };
  const dim3 per_image_or_group = bundle_blocks(nimages > BUNDLE_MAX_GROUPS ? nimages : BUNDLE_MAX_GROUPS);
  int r = scope("bundle_setup", [&] {
    launch_track_candidates(ctx, scene, D.owner, D.key);
    hipLaunchKernelGGL(bundle_image_init_kernel, per_image, th, 0, s, D);
    pick(bundle_premember_kernel, bundle_premember_kernel, bundle_premember_radial_kernel, per_slot);
    hipLaunchKernelGGL(bundle_activate_kernel, per_track, th, 0, s, D);
    hipLaunchKernelGGL(bundle_gather_kernel, image_wg, th, 0, s, D);
    if (radial) hipLaunchKernelGGL(bundle_radial_init_kernel, one, th, 0, s, D);
    else if (focal) hipLaunchKernelGGL(bundle_focal_init_kernel, one, th, 0, s, D);
    eval(0);
    hipLaunchKernelGGL(bundle_cost_kernel, image_wg, th, 0, s, D, 0);
    hipLaunchKernelGGL(bundle_start_kernel, one, th, 0, s, D);
  });
  for (int loop = 0; loop < num_loops && !r; loop++) {
    r = scope("bundle_track", [&] { track_normal(); });
    if (!r) r = scope("bundle_image", [&] { pick(bundle_image_normal_kernel, bundle_image_normal_focal_kernel, bundle_image_normal_radial_kernel, image_wg); });
    if (!r) r = scope("bundle_scalar", [&] { pick(bundle_cg_start_kernel, bundle_cg_start_focal_kernel, bundle_cg_start_radial_kernel, one); });
    for (int it = 0; it < cg_iters && !r; it++) {
      r = scope("bundle_track", [&] { pick(bundle_cg_track_kernel, bundle_cg_track_focal_kernel, bundle_cg_track_radial_kernel, per_track); });
      if (!r) r = scope("bundle_image", [&] { pick(bundle_cg_image_kernel, bundle_cg_image_focal_kernel, bundle_cg_image_radial_kernel, image_wg); });
      if (!r) r = scope("bundle_scalar", [&] { pick(bundle_cg_scalar_kernel, bundle_cg_scalar_focal_kernel, bundle_cg_scalar_radial_kernel, one); });
    }
    if (!r) r = scope("bundle_track", [&] { pick(bundle_track_trial_kernel, bundle_track_trial_focal_kernel, bundle_track_trial_radial_kernel, per_track); });
    if (!r) r = scope("bundle_trial", [&] {
      if (radial) hipLaunchKernelGGL(bundle_image_trial_radial_kernel, per_image_or_group, th, 0, s, D);
      else if (focal) hipLaunchKernelGGL(bundle_image_trial_focal_kernel, per_image_or_group, th, 0, s, D);
      else hipLaunchKernelGGL(bundle_image_trial_kernel, per_image, th, 0, s, D);
      eval(1);
    });
    if (!r) r = scope("bundle_image", [&] { hipLaunchKernelGGL(bundle_cost_kernel, image_wg, th, 0, s, D, 1); });
    if (!r) r = scope("bundle_scalar", [&] { hipLaunchKernelGGL(bundle_decide_kernel, one, th, 0, s, D); });
  }
  if (r) return r;
  return scope("bundle_out", [&] {
    hipLaunchKernelGGL(bundle_image_out_kernel, per_image, th, 0, s, D);
    hipLaunchKernelGGL(bundle_track_out_kernel, per_track, th, 0, s, D);
    if (d_obs_weight) pick(bundle_weight_out_kernel, bundle_weight_out_focal_kernel, bundle_weight_out_radial_kernel, per_slot);
    if (d_intrinsics_out) hipLaunchKernelGGL(bundle_focal_out_kernel, per_image_or_group, th, 0, s, D, focal ? 1 : 0);
    if (R && ngroups > 0) hipLaunchKernelGGL(bundle_radial_out_kernel, one, th, 0, s, D, focal ? 1 : 0, radial ? 1 : 0);
  });
}

int launch_adjust_bundle_focal_batch(misift_ctx *ctx, const TrackScene &scene, const int *h_held, int min_views,
                                     int min_obs, int num_loops, int cg_iters, float thresh2, float lambda0,
                                     int orthonormalise, int loss, float loss_scale, float loss_scale2, int ngroups,
                                     const int *h_group, bool focal, float *d_cam_out, float *d_points_out, int *d_cam_obs,
                                     int *d_cam_status, float *d_cam_rms, int *d_point_obs, float *d_history,
                                     float *d_cost, float *d_obs_weight, int *d_summary, float *d_intrinsics_out,
                                     int *d_focal)
{
  return bundle_launch(ctx, scene, h_held, min_views, min_obs, num_loops, cg_iters, thresh2, lambda0, orthonormalise, loss,
                       loss_scale, loss_scale2, ngroups, h_group, focal, d_cam_out, d_points_out, d_cam_obs, d_cam_status,
                       d_cam_rms, d_point_obs, d_history, d_cost, d_obs_weight, d_summary, d_intrinsics_out, d_focal,
                       nullptr);
}

int launch_adjust_bundle_radial_batch(misift_ctx *ctx, const TrackScene &scene, const int *h_held, int min_views,
                                      int min_obs, int num_loops, int cg_iters, float thresh2, float lambda0,
                                      int orthonormalise, int loss, float loss_scale, float loss_scale2, int ngroups,
                                      const int *h_group, bool focal, const int *h_radial, const float *h_k0, bool radial,
                                      float *d_cam_out, float *d_points_out, int *d_cam_obs, int *d_cam_status,
                                      float *d_cam_rms, int *d_point_obs, float *d_history, float *d_cost,
                                      float *d_obs_weight, int *d_summary, float *d_intrinsics_out, int *d_focal,
                                      int *d_radial)
{
  const BundleRadialArgs R{h_radial, h_k0, radial, d_radial};
  return bundle_launch(ctx, scene, h_held, min_views, min_obs, num_loops, cg_iters, thresh2, lambda0, orthonormalise, loss,
                       loss_scale, loss_scale2, ngroups, h_group, focal, d_cam_out, d_points_out, d_cam_obs, d_cam_status,
                       d_cam_rms, d_point_obs, d_history, d_cost, d_obs_weight, d_summary, d_intrinsics_out, d_focal, &R);
}

// Enqueue misift_undistort_obs_batch: one launch, no temp
int launch_undistort_obs_batch(misift_ctx *ctx, int max_obs, const TrackObs *d_obs, const int *d_export_summary,
                               int nimages, const float *h_intrinsics, const int *h_group, const int *d_radial,
                               TrackObs *d_obs_out)
{
  LaunchScope ls(ctx, "undistort_obs");
  hipLaunchKernelGGL(undistort_obs_kernel, bundle_blocks(max_obs), dim3(BUNDLE_THREADS), 0, ctx->stream, max_obs, d_obs,
                     d_export_summary, nimages, h_intrinsics, h_group, d_radial, d_obs_out);
  return ls.finish();
}

// The hooks' common body (bundle_host.hpp) with the library's error message.
static int bundle_hook(const char *who, int max_tracks, int max_obs, const int *track_offsets,
                       const misift_track_obs *obs, const int *export_summary, const float *points,
                       const int *point_status, int nimages, const float *cam, const int *cam_pair,
                       const float *intrinsics, int nhold, const int *hold, int min_views, int min_obs, int num_loops,
                       int cg_iters, float max_error, float lambda0, int orthonormalise, int loss, float loss_scale,
                       int ngroups, const int *group, float *cam_out, float *points_out, int *cam_obs, int *cam_status,
                       float *cam_rms, int *point_obs, float *history, float *cost, float *obs_weight, int *summary,
                       float *intrinsics_out, int *focal_out, const int *radial_flags = nullptr,
                       const float *k0 = nullptr, int *radial_out = nullptr)
{
  if (bundle_host(max_tracks, max_obs, track_offsets, reinterpret_cast<const TrackObs *>(obs), export_summary, points,
                  point_status, nimages, cam, cam_pair, intrinsics, nhold, hold, min_views, min_obs, num_loops, cg_iters,
                  max_error, lambda0, orthonormalise, loss, loss_scale, ngroups, group, cam_out, points_out, cam_obs,
                  cam_status, cam_rms, point_obs, history, cost, obs_weight, summary, intrinsics_out, focal_out,
                  radial_flags, k0, radial_out))
    return MISIFT_OK;
  misift_set_error((std::string(who) + ": invalid argument").c_str());
  return MISIFT_EINVAL;
}

// Test-only, host-only: the whole call on host arrays, phase after phase through bundle_core.hpp.
extern "C" int misift_test_adjust_bundle_focal(int max_tracks, int max_obs, const int *track_offsets,
                                               const misift_track_obs *obs, const int *export_summary,
                                               const float *points, const int *point_status, int nimages,
                                               const float *cam, const int *cam_pair, const float *intrinsics,
                                               int nhold, const int *hold, int min_views, int min_obs, int num_loops,
                                               int cg_iters, float max_error, float lambda0, int orthonormalise,
                                               int loss, float loss_scale, int ngroups, const int *group, float *cam_out,
                                               float *points_out, int *cam_obs, int *cam_status, float *cam_rms,
                                               int *point_obs, float *history, float *cost, float *obs_weight,
                                               int *summary, float *intrinsics_out, int *focal)
{
  if (!intrinsics_out || (ngroups > 0 && !focal)) {
    misift_set_error("misift_test_adjust_bundle_focal: invalid argument");
    return MISIFT_EINVAL;
  }
  return bundle_hook(__func__, max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status, nimages, cam,
                     cam_pair, intrinsics, nhold, hold, min_views, min_obs, num_loops, cg_iters, max_error, lambda0,
                     orthonormalise, loss, loss_scale, ngroups, group, cam_out, points_out, cam_obs, cam_status, cam_rms,
                     point_obs, history, cost, obs_weight, summary, intrinsics_out, focal);
}

// The same for misift_adjust_bundle_radial_batch.
extern "C" int misift_test_adjust_bundle_radial(int max_tracks, int max_obs, const int *track_offsets,
                                                const misift_track_obs *obs, const int *export_summary,
                                                const float *points, const int *point_status, int nimages,
                                                const float *cam, const int *cam_pair, const float *intrinsics,
                                                int nhold, const int *hold, int min_views, int min_obs, int num_loops,
                                                int cg_iters, float max_error, float lambda0, int orthonormalise,
                                                int loss, float loss_scale, int ngroups, const int *group,
                                                const int *radial, const float *k0, float *cam_out, float *points_out,
                                                int *cam_obs, int *cam_status, float *cam_rms, int *point_obs,
                                                float *history, float *cost, float *obs_weight, int *summary,
                                                float *intrinsics_out, int *focal, float *radial_out)
{
  static const int no_flag[BUNDLE_MAX_GROUPS] = {0};
  static const float no_k0[BUNDLE_MAX_GROUPS] = {0.0f};
  if (!intrinsics_out || (ngroups > 0 && (!focal || !radial_out)) || (radial != nullptr) != (k0 != nullptr)) {
    misift_set_error("misift_test_adjust_bundle_radial: invalid argument");
    return MISIFT_EINVAL;
  }
  return bundle_hook(__func__, max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status, nimages, cam,
                     cam_pair, intrinsics, nhold, hold, min_views, min_obs, num_loops, cg_iters, max_error, lambda0,
                     orthonormalise, loss, loss_scale, ngroups, group, cam_out, points_out, cam_obs, cam_status, cam_rms,
                     point_obs, history, cost, obs_weight, summary, intrinsics_out, focal, radial ? radial : no_flag,
                     k0 ? k0 : no_k0, reinterpret_cast<int *>(radial_out));
}

// Test-only, host-only: misift_undistort_obs_batch on host arrays.
extern "C" int misift_test_undistort_obs(int max_obs, const misift_track_obs *obs, const int *export_summary, int nimages,
                                         const float *intrinsics, int ngroups, const int *group, const float *radial,
                                         misift_track_obs *obs_out)
{
  if (bundle_host_undistort(max_obs, reinterpret_cast<const TrackObs *>(obs), export_summary, nimages, intrinsics, ngroups,
                            group, reinterpret_cast<const int *>(radial), reinterpret_cast<TrackObs *>(obs_out)))
    return MISIFT_OK;
  misift_set_error("misift_test_undistort_obs: invalid argument");
  return MISIFT_EINVAL;
}

extern "C" int misift_test_adjust_bundle_robust(int max_tracks, int max_obs, const int *track_offsets,
                                                const misift_track_obs *obs, const int *export_summary,
                                                const float *points, const int *point_status, int nimages,
                                                const float *cam, const int *cam_pair, const float *intrinsics,
                                                int nhold, const int *hold, int min_views, int min_obs, int num_loops,
                                                int cg_iters, float max_error, float lambda0, int orthonormalise,
                                                int loss, float loss_scale, float *cam_out, float *points_out,
                                                int *cam_obs, int *cam_status, float *cam_rms, int *point_obs,
                                                float *history, float *cost, float *obs_weight, int *summary)
{
  return bundle_hook(__func__, max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status, nimages, cam,
                     cam_pair, intrinsics, nhold, hold, min_views, min_obs, num_loops, cg_iters, max_error, lambda0,
                     orthonormalise, loss, loss_scale, 0, nullptr, cam_out, points_out, cam_obs, cam_status, cam_rms,
                     point_obs, history, cost, obs_weight, summary, nullptr, nullptr);
}

extern "C" int misift_test_adjust_bundle(int max_tracks, int max_obs, const int *track_offsets, const misift_track_obs *obs,
                                         const int *export_summary, const float *points, const int *point_status,
                                         int nimages, const float *cam, const int *cam_pair, const float *intrinsics,
                                         int nhold, const int *hold, int min_views, int min_obs, int num_loops,
                                         int cg_iters, float max_error, float lambda0, int orthonormalise,
                                         float *cam_out, float *points_out, int *cam_obs, int *cam_status,
                                         float *cam_rms, int *point_obs, float *history, float *cost, int *summary)
{
  return misift_test_adjust_bundle_robust(max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status,
                                          nimages, cam, cam_pair, intrinsics, nhold, hold, min_views, min_obs, num_loops,
                                          cg_iters, max_error, lambda0, orthonormalise, MISIFT_LOSS_NONE, 0.0f, cam_out,
                                          points_out, cam_obs, cam_status, cam_rms, point_obs, history, cost, nullptr,
                                          summary);
}

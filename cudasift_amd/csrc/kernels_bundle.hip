// kernels_bundle.hip — misift_adjust_bundle_batch: Levenberg-Marquardt over all free cameras and all active track points
// at once.  Each step eliminates the points (Schur complement), solves the reduced camera system matrix-free by a fixed
// number of block-Jacobi preconditioned conjugate-gradient iterations, back-substitutes the points and is kept or turned
// away on the device.  No reference counterpart.  The arithmetic is bundle_core.hpp: every kernel here is a few lines
// that hand one work item to the function of its phase, the same function the host-only test hook at the end of this
// file runs in a loop.
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
// Jc, Jp and r are written once per LM step and read by both views: recomputing them in each CG pass instead gives the
// same bits and measured 10 to 13 % slower.
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "common.hpp"
#include "bundle_core.hpp"
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

template <bool ROBUST, bool FOCAL = false>
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_eval_kernel(BundleData D, int trial)
{
  const int o = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (o < scene_O(D.s)) bundle_eval_slot<ROBUST, FOCAL>(D, o, trial != 0);
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

// the temp of the call laid out behind `base` (NULL: only the size is wanted); every array starts 16-byte aligned
size_t bundle_layout(BundleData &D, char *base, bool focal = false)
{
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char *p = base ? base + at : nullptr;
    at += (bytes + 15) & ~(size_t)15;
    return p;
  };
  const size_t mo = (size_t)D.s.max_obs, mt = (size_t)D.s.max_tracks, n = (size_t)D.s.nimages;
  D.owner = reinterpret_cast<int *>(take(4 * mo));
  D.key = reinterpret_cast<int *>(take(4 * mo));
  D.list = reinterpret_cast<int *>(take(4 * mo));
  D.istart = reinterpret_cast<int *>(take(4 * n));
  D.icount = reinterpret_cast<int *>(take(4 * n));
  D.istate = reinterpret_cast<int *>(take(4 * n));
  D.tcount = reinterpret_cast<int *>(take(4 * mt));
  D.ctl = reinterpret_cast<int *>(take(4 * BUNDLE_CTL));
  D.fctl = reinterpret_cast<float *>(take(4 * BUNDLE_FCTL));
  D.lin = reinterpret_cast<float *>(take(4 * BUNDLE_LIN * mo));
  D.eterm = reinterpret_cast<float *>(take(4 * 2 * mo));
  D.cams = reinterpret_cast<float *>(take(4 * 2 * 12 * n));
  D.pts = reinterpret_cast<float *>(take(4 * 2 * 3 * mt));
  D.tv = reinterpret_cast<float *>(take(4 * 9 * mt));
  D.tq = reinterpret_cast<float *>(take(4 * 3 * mt));
  D.iu = reinterpret_cast<float *>(take(4 * REFINE_SUMS * n));
  D.ivec = reinterpret_cast<float *>(take(4 * 5 * 6 * n));
  D.icost = reinterpret_cast<float *>(take(4 * 3 * n));
  if (!focal) return at;
  D.fcount = reinterpret_cast<int *>(take(4 * BUNDLE_MAX_GROUPS));
  D.fs = reinterpret_cast<float *>(take(4 * 2 * BUNDLE_MAX_GROUPS));
  D.fvec = reinterpret_cast<float *>(take(4 * 5 * BUNDLE_MAX_GROUPS));
  D.fsc = reinterpret_cast<float *>(take(4 * 2 * BUNDLE_MAX_GROUPS));
  D.flin = reinterpret_cast<float *>(take(4 * 2 * mo));
  D.tfd = reinterpret_cast<float *>(take(4 * BUNDLE_MAX_GROUPS * mt));
  D.iuf = reinterpret_cast<float *>(take(4 * BUNDLE_IMAGE_FOCAL * n));
  D.ifv = reinterpret_cast<float *>(take(4 * 2 * n));
  return at;
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
int launch_adjust_bundle_focal_batch(misift_ctx *ctx, const TrackScene &scene, const int *h_held, int min_views,
                                     int min_obs, int num_loops, int cg_iters, float thresh2, float lambda0,
                                     int orthonormalise, int loss, float loss_scale, float loss_scale2, int ngroups,
                                     const int *h_group, bool focal, float *d_cam_out, float *d_points_out, int *d_cam_obs,
                                     int *d_cam_status, float *d_cam_rms, int *d_point_obs, float *d_history,
                                     float *d_cost, float *d_obs_weight, int *d_summary, float *d_intrinsics_out,
                                     int *d_focal)
{
  const int max_tracks = scene.max_tracks, max_obs = scene.max_obs, nimages = scene.nimages;
  const int rc = misift_ensure_tmp(ctx, focal ? adjust_bundle_focal_batch_tmp_bytes(max_tracks, max_obs, nimages)
                                              : adjust_bundle_batch_tmp_bytes(max_tracks, max_obs, nimages));
  if (rc) return rc;
  BundleData D;
  D.ngroups = ngroups; D.grp = h_group; D.intrinsics_out = d_intrinsics_out; D.focal_out = d_focal;
  D.s = scene; D.min_views = min_views; D.min_obs = min_obs;
  D.num_loops = num_loops; D.cg_iters = cg_iters; D.orthonormalise = orthonormalise; D.thresh2 = thresh2;
  D.lambda0 = lambda0;
  D.loss = loss; D.loss_scale = loss_scale; D.loss_scale2 = loss_scale2;
  D.held = h_held;
  bundle_layout(D, reinterpret_cast<char *>(ctx->d_match_tmp), focal);
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
    if (focal && robust) hipLaunchKernelGGL((bundle_eval_kernel<true, true>), per_slot, th, 0, s, D, trial);
    else if (focal) hipLaunchKernelGGL((bundle_eval_kernel<false, true>), per_slot, th, 0, s, D, trial);
    else if (robust) hipLaunchKernelGGL(bundle_eval_kernel<true>, per_slot, th, 0, s, D, trial);
    else hipLaunchKernelGGL(bundle_eval_kernel<false>, per_slot, th, 0, s, D, trial);
  };
  auto track_normal = [&] {
    if (focal && robust) hipLaunchKernelGGL(bundle_track_normal_focal_kernel<true>, per_track, th, 0, s, D);
    else if (focal) hipLaunchKernelGGL(bundle_track_normal_focal_kernel<false>, per_track, th, 0, s, D);
    else if (robust) hipLaunchKernelGGL(bundle_track_normal_kernel<true>, per_track, th, 0, s, D);
    else hipLaunchKernelGGL(bundle_track_normal_kernel<false>, per_track, th, 0, s, D);
  };
  // a phase that reads the focal scale has a FOCAL instance; the plain one holds no trace of it
  auto pick = [&](auto plain, auto with_focal, dim3 grid) {
    if (focal) hipLaunchKernelGGL(with_focal, grid, th, 0, s, D);
    else hipLaunchKernelGGL(plain, grid, th, 0, s, D);
  };
  const dim3 per_image_or_group = bundle_blocks(nimages > BUNDLE_MAX_GROUPS ? nimages : BUNDLE_MAX_GROUPS);
  int r = scope("bundle_setup", [&] {
    launch_track_candidates(ctx, scene, D.owner, D.key);
    hipLaunchKernelGGL(bundle_image_init_kernel, per_image, th, 0, s, D);
    hipLaunchKernelGGL(bundle_premember_kernel, per_slot, th, 0, s, D);
    hipLaunchKernelGGL(bundle_activate_kernel, per_track, th, 0, s, D);
    hipLaunchKernelGGL(bundle_gather_kernel, image_wg, th, 0, s, D);
    if (focal) hipLaunchKernelGGL(bundle_focal_init_kernel, one, th, 0, s, D);
    eval(0);
    hipLaunchKernelGGL(bundle_cost_kernel, image_wg, th, 0, s, D, 0);
    hipLaunchKernelGGL(bundle_start_kernel, one, th, 0, s, D);
  });
  for (int loop = 0; loop < num_loops && !r; loop++) {
    r = scope("bundle_track", [&] { track_normal(); });
    if (!r) r = scope("bundle_image", [&] { pick(bundle_image_normal_kernel, bundle_image_normal_focal_kernel, image_wg); });
    if (!r) r = scope("bundle_scalar", [&] { pick(bundle_cg_start_kernel, bundle_cg_start_focal_kernel, one); });
    for (int it = 0; it < cg_iters && !r; it++) {
      r = scope("bundle_track", [&] { pick(bundle_cg_track_kernel, bundle_cg_track_focal_kernel, per_track); });
      if (!r) r = scope("bundle_image", [&] { pick(bundle_cg_image_kernel, bundle_cg_image_focal_kernel, image_wg); });
      if (!r) r = scope("bundle_scalar", [&] { pick(bundle_cg_scalar_kernel, bundle_cg_scalar_focal_kernel, one); });
    }
    if (!r) r = scope("bundle_track", [&] { pick(bundle_track_trial_kernel, bundle_track_trial_focal_kernel, per_track); });
    if (!r) r = scope("bundle_trial", [&] {
      if (focal) hipLaunchKernelGGL(bundle_image_trial_focal_kernel, per_image_or_group, th, 0, s, D);
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
    if (d_obs_weight) pick(bundle_weight_out_kernel, bundle_weight_out_focal_kernel, per_slot);
    if (d_intrinsics_out) hipLaunchKernelGGL(bundle_focal_out_kernel, per_image_or_group, th, 0, s, D, focal ? 1 : 0);
  });
}

namespace {

// the phases of the host hook that read the loss
template <bool ROBUST, bool FOCAL>
void bundle_host_eval(const BundleData &D, int O, bool trial)
{
  for (int o = 0; o < O; o++) bundle_eval_slot<ROBUST, FOCAL>(D, o, trial);
}
template <bool ROBUST, bool FOCAL>
void bundle_host_track_normal(const BundleData &D, int T)
{
  for (int t = 0; t < T; t++) FOCAL ? bundle_track_normal_focal<ROBUST>(D, t) : bundle_track_normal<ROBUST>(D, t);
}

// the phases of the hook in the order of the launches
template <bool ROBUST, bool FOCAL>
void bundle_host_run(const BundleData &D, int T, int O)
{
  const int nimages = D.s.nimages;
  BundleHostSum S;
  if (FOCAL) bundle_focal_init(D, S, 0, 1);
  bundle_host_eval<ROBUST, FOCAL>(D, O, false);
  for (int i = 0; i < nimages; i++) bundle_image_cost(D, S, i, false, true);
  bundle_scalar_init(D, S, true);
  for (int loop = 0; loop < D.num_loops; loop++) {
    bundle_host_track_normal<ROBUST, FOCAL>(D, T);
    for (int i = 0; i < nimages; i++) FOCAL ? bundle_image_normal_focal(D, S, i, true) : bundle_image_normal(D, S, i, true);
    bundle_cg_start<FOCAL>(D, S, 0, 1, true);
    for (int it = 0; it < D.cg_iters; it++) {
      for (int t = 0; t < T; t++) bundle_cg_track<FOCAL>(D, t);
      for (int i = 0; i < nimages; i++) FOCAL ? bundle_cg_image_focal(D, S, i, true) : bundle_cg_image(D, S, i, true);
      bundle_cg_scalar<FOCAL>(D, S, 0, 1, true);
    }
    for (int t = 0; t < T; t++) bundle_track_trial<FOCAL>(D, t);
    for (int i = 0; i < nimages; i++) bundle_image_trial(D, i);
    if (FOCAL)
      for (int g = 0; g < BUNDLE_MAX_GROUPS; g++) bundle_focal_trial(D, g);
    bundle_host_eval<ROBUST, FOCAL>(D, O, true);
    for (int i = 0; i < nimages; i++) bundle_image_cost(D, S, i, true, true);
    bundle_decide(D, S, 0, 1, true);
  }
  for (int i = 0; i < nimages; i++) bundle_image_out(D, i);
  for (int t = 0; t < T; t++) bundle_track_out(D, t);
  if (D.obs_weight)
    for (int o = 0; o < O; o++) bundle_weight_slot<FOCAL>(D, o);
  if (D.intrinsics_out) {
    for (int i = 0; i < nimages; i++) bundle_intrinsics_out(D, i, FOCAL);
    for (int g = 0; g < D.ngroups; g++) bundle_focal_out(D, g, FOCAL);
  }
}

}  // namespace

// The hooks' common body: the whole call on host arrays; ngroups 0 and no intrinsics_out is the robust call.
static int bundle_host(const char *who, int max_tracks, int max_obs, const int *track_offsets,
                       const misift_track_obs *obs, const int *export_summary, const float *points,
                       const int *point_status, int nimages, const float *cam, const int *cam_pair,
                       const float *intrinsics, int nhold, const int *hold, int min_views, int min_obs, int num_loops,
                       int cg_iters, float max_error, float lambda0, int orthonormalise, int loss, float loss_scale,
                       int ngroups, const int *group, float *cam_out, float *points_out, int *cam_obs, int *cam_status,
                       float *cam_rms, int *point_obs, float *history, float *cost, float *obs_weight, int *summary,
                       float *intrinsics_out, int *focal_out)
{
  bool ok = max_tracks >= 1 && max_obs >= 1 && nimages >= 1 && track_offsets && obs && export_summary && points &&
            point_status && cam && cam_pair && intrinsics && nhold >= 0 && (nhold == 0 || hold) && min_views >= 2 &&
            min_obs >= 3 && num_loops >= 0 && cg_iters >= 0 && max_error > 0.0f && lambda0 > 0.0f &&
            fundamental_finite(lambda0) && (orthonormalise == 0 || orthonormalise == 1) && cam_out && points_out &&
            cam_obs && cam_status && cam_rms && point_obs && (history || num_loops == 0) && cost && summary &&
            loss >= BUNDLE_LOSS_NONE && loss <= BUNDLE_LOSS_GEMAN_MCCLURE &&
            (loss == BUNDLE_LOSS_NONE || (loss_scale > 0.0f && fundamental_finite(loss_scale)));
  for (int j = 0; ok && j < nhold; j++) ok = hold[j] >= 0 && hold[j] < nimages;
  ok = ok && ngroups >= 0 && ngroups <= BUNDLE_MAX_GROUPS && (ngroups == 0 || group);
  bool focal = false;
  for (int i = 0; ok && ngroups > 0 && i < nimages; i++) {
    ok = group[i] >= -1 && group[i] < ngroups;
    focal = focal || group[i] >= 0;
  }
  if (!ok) {
    misift_set_error((std::string(who) + ": invalid argument").c_str());
    return MISIFT_EINVAL;
  }
  BundleData D;
  D.ngroups = ngroups; D.grp = ngroups > 0 ? group : nullptr; D.intrinsics_out = intrinsics_out; D.focal_out = focal_out;
  D.s = TrackScene{max_tracks, max_obs, nimages, track_offsets, reinterpret_cast<const TrackObs *>(obs), export_summary,
                   points, point_status, cam, cam_pair, intrinsics};
  D.min_views = min_views; D.min_obs = min_obs; D.num_loops = num_loops; D.cg_iters = cg_iters;
  D.orthonormalise = orthonormalise;
  D.thresh2 = max_error * max_error; D.lambda0 = lambda0;
  const bool robust = loss != BUNDLE_LOSS_NONE;
  D.loss = loss; D.loss_scale = robust ? loss_scale : 0.0f; D.loss_scale2 = D.loss_scale * D.loss_scale;
  std::vector<int> held(nimages, 0);
  for (int j = 0; j < nhold; j++) held[hold[j]] = 1;
  D.held = held.data();
  std::vector<char> tmp(bundle_layout(D, nullptr, focal) + 16, 0);
  bundle_layout(D, reinterpret_cast<char *>(((uintptr_t)tmp.data() + 15) & ~(uintptr_t)15), focal);
  D.cam_out = cam_out; D.points_out = points_out; D.cam_rms = cam_rms; D.history = history; D.cost = cost;
  D.cam_obs = cam_obs; D.cam_status = cam_status; D.point_obs = point_obs; D.summary = summary;
  D.obs_weight = obs_weight;
  const int T = scene_T(D.s), O = scene_O(D.s);
  // the owners and the candidates, as launch_track_candidates
  for (int o = 0; o < max_obs; o++) D.owner[o] = -1;
  for (int t = 0; t < T; t++) scene_track_owns(D.s, D.owner, t);
  for (int o = 0; o < O; o++) D.key[o] = scene_slot_key(D.s, D.owner, o);
  for (int j = 0; j < 8; j++) summary[j] = 0;
  for (int i = 0; i < nimages; i++) bundle_image_init(D, i);
  for (int o = 0; o < O; o++) bundle_slot_premember(D, o);
  for (int t = 0; t < T; t++) bundle_track_activate(D, t);
  {
    int at = 0;
    for (int i = 0; i < nimages; i++) {
      D.istart[i] = at;
      for (int o = 0; o < O; o++)
        if (D.key[o] == i) D.list[at++] = o;
      D.icount[i] = at - D.istart[i];
      if (D.istate[i] == BUNDLE_ADJUSTED && D.icount[i] < min_obs) D.istate[i] = BUNDLE_FEW_OBS;
    }
  }
  if (focal) robust ? bundle_host_run<true, true>(D, T, O) : bundle_host_run<false, true>(D, T, O);
  else robust ? bundle_host_run<true, false>(D, T, O) : bundle_host_run<false, false>(D, T, O);
  return MISIFT_OK;
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
  return bundle_host(__func__, max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status, nimages, cam,
                     cam_pair, intrinsics, nhold, hold, min_views, min_obs, num_loops, cg_iters, max_error, lambda0,
                     orthonormalise, loss, loss_scale, ngroups, group, cam_out, points_out, cam_obs, cam_status, cam_rms,
                     point_obs, history, cost, obs_weight, summary, intrinsics_out, focal);
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
  return bundle_host(__func__, max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status, nimages, cam,
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

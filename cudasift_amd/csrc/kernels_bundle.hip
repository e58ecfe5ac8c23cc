// kernels_bundle.hip — misift_adjust_bundle_batch: Levenberg-Marquardt over all free cameras and all active track points
// at once.  Each step eliminates the points (Schur complement), solves the reduced camera system matrix-free by a fixed
// number of block-Jacobi preconditioned conjugate-gradient iterations, back-substitutes the points and is kept or turned
// away on the device.  No reference counterpart.  The arithmetic is bundle_core.hpp, the order of the phases is
// bundle_schedule (bundle_host.hpp), which the host-only test hook runs too; here are five kernels, one per shape of
// work item, each a few lines that hand the work item to the phase type P they are instantiated over:
//   bundle_slot_kernel<P>       lane per slot
//   bundle_track_kernel<P>      lane per track
//   bundle_image_kernel<P>      lane per image, and where P says so the first lanes of the launch a group each
//   bundle_image_sum_kernel<P>  256-thread workgroup per image, P::SUMS sums through LDS at once
//   bundle_scalar_kernel<P>     the scalar workgroup, P::SUMS sums
// two kernels written by hand (bundle_gather_kernel, bundle_radial_out_kernel), and the device executor
// (BundleDeviceExec), which turns a phase of the schedule into a launch.
//
// Three memsets (the owners, the control words, the summary) and 11 + num_loops * (8 + 3 * cg_iters) launches, whatever
// the data.  A dispatch boundary is the only barrier between workgroups: nothing in here waits for another workgroup.
//   cand_owner_kernel, cand_key_kernel     launch_track_candidates: the owner of every slot, the image it is a candidate of
//   image<BundleImageInit>      usable / held / free, the camera of refine's step 1 into both buffers
//   slot<BundlePremember>       refine's member test under that camera
//   track<BundleActivate>       its pre-members counted; an inactive track's leave the keys
//   bundle_gather_kernel        two walks over the keys: the members of lower images counted (the start of its list),
//                               then its members listed in ascending slot (ballot and popcount keep the order, as
//                               resect's gather); demotion
//   slot<BundleEval>            a member's squared residual under a state buffer
//   image_sum<BundleCost>       its cost by the position rule
//   scalar<BundleStart>         the cost of the start, lambda0
//   per LM step:
//   track<BundleTrackNormal>      Jc, Jp, r of its members into temp, V, gp, V', V'^-1 gp
//   image_sum<BundleImageNormal>  U, gc, sum W y (33 sums, 33 KiB of LDS), U', b, the LDL^T checked
//   scalar<BundleCgStart>         x, r, z, p, rho
//   per CG iteration: track<BundleCgTrack>, image_sum<BundleCgImage> (6 sums), scalar<BundleCgScalar>
//   track<BundleTrackTrial>, image<BundleImageTrial>   the trial state
//   slot<BundleEval>, image_sum<BundleCost>            under the trial state
//   scalar<BundleDecide>        kept or not, lambda, the history
//   then image<BundleImageOut> and track<BundleTrackOut> write the outputs.
// The loss and the model are template arguments <ROBUST, FOCAL, RADIAL> of the phase types that read them; bundle_run
// picks one of the six instances of the schedule once per call, so no launch chooses again.
// misift_adjust_bundle_robust_batch is the same sequence with a loss (bundle_loss): BundleTrackNormal<true, ..> scales a
// member's 20 values by sqrt(w) where it writes them and BundleEval<true, ..> stores rho; the plain call launches the
// <false, ..> instances, which hold no trace of the loss.  With d_obs_weight one launch more at the end,
//   slot<BundleWeightOut>       w of a member under the final state, -1 for any other slot
// misift_adjust_bundle_focal_batch adds one focal scale per camera group to the unknowns.  Without a grouped image it
// is the sequence above and one launch more at the end (image<BundleIntrinsicsOut>: d_intrinsics_out and d_focal).
// With one, the FOCAL instances run, beside the plain ones, which hold no trace of the scale:
//   scalar<BundleGroupInit>     behind the gather: s_g = 1, the members of every group; no LDS
//   BundleEval, BundleWeightOut   the member projected with fx*s_g, fy*s_g
//   BundleTrackNormal           Juf, Jvf of every member beside the 20 values; per group w_gt . V'^-1 w_gt
//   BundleImageNormal           42 sums (42 KiB of LDS): the 33, U_cf, Uff, gf, wf . y_t
//   BundleCgStart (3 sums)      per group the cross-image sums U_gg, g_g and the cross-track sum of the Schur
//                               scalar S_gg, in the scalar workgroup one group after another
//   BundleCgTrack, BundleCgImage (7 sums), BundleCgScalar (2)   the focal terms of the gather, of y_i, and y_g
//   BundleTrackTrial, BundleImageTrial   the trial point; the trial camera and, in the first 8 lanes, the trial scale
// so 13 + num_loops * (8 + 3 * cg_iters) launches: the two more are the groups' members and the two new outputs.
// misift_adjust_bundle_radial_batch adds one radial coefficient per camera group, applied to the observation.  With
// nothing radial (no grouped image, or no unknown coefficient and every start zero) it is the focal call's sequence and
// one launch more at the end (bundle_radial_out_kernel: d_radial).  Otherwise the RADIAL instances run where the FOCAL
// ones ran, launch for launch:
//   BundlePremember, BundleEval, BundleWeightOut   the observation enters as (x', y') under k_g (the member test: under k0)
//   BundleGroupInit             and k_g = k0_g in both state buffers
//   BundleTrackNormal           the column Juk, Jvk of every member beside Juf, Jvf; per group wk_gt . V'^-1 wk_gt,
//                               the wk_gt from a walk of their own in the registers of the w_gt (no scratch)
//   BundleImageNormal           52 sums (52 KiB of LDS): the 42, U_ck, Ukk, gk, wk . y_t, Ufk
//   BundleCgStart (4), BundleCgTrack, BundleCgImage (8), BundleCgScalar (2)   S_kk and U_fk per group; the terms of
//                               k_g in the gather, in y_i, y_g and y_k
//   BundleTrackTrial, BundleImageTrial   the trial point; the trial camera, scale and k_g
// so 14 + num_loops * (8 + 3 * cg_iters) launches.  misift_undistort_obs_batch is undistort_obs_kernel alone.
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

// ---- one kernel per shape of work item, instantiated over the phase types of bundle_core.hpp; a trailing int of the
// launch (the trial flag, `refined`) travels as A

template <class P, class... A>
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_slot_kernel(BundleData D, A... a)
{
  const int o = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (o < scene_O(D.s)) P::run(D, o, a...);
}

template <class P, class... A>
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_track_kernel(BundleData D, A... a)
{
  const int t = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (t < scene_T(D.s)) P::run(D, t, a...);
}

// lane per image; with P::GROUPS the first P::groups(D) lanes of the launch take a group each as well
template <class P, class... A>
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_image_kernel(BundleData D, A... a)
{
  const int i = blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (i < D.s.nimages) P::run(D, i, a...);
  if constexpr (P::GROUPS)
    if (i < P::groups(D)) P::group(D, i, a...);
}

// workgroup per image, P::SUMS sums through LDS at once
template <class P, class... A>
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_image_sum_kernel(BundleData D, A... a)
{
  __shared__ float s_p[P::SUMS * FUND_SLOTS];
  BundleBlockSum S{s_p};
  P::template run<BundleBlockSum>(D, S, blockIdx.x, threadIdx.x == 0, a...);
}

// the scalar workgroup; a phase that takes no sum gets a Sum without LDS
template <class P>
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_scalar_kernel(BundleData D)
{
  if constexpr (P::SUMS > 0) {
    __shared__ float s_p[P::SUMS * FUND_SLOTS];
    BundleBlockSum S{s_p};
    P::template run<BundleBlockSum>(D, S, threadIdx.x, BUNDLE_THREADS, threadIdx.x == 0);
  } else {
    BundleBlockSum S{nullptr};
    P::template run<BundleBlockSum>(D, S, threadIdx.x, BUNDLE_THREADS, threadIdx.x == 0);
  }
}

// ---- the two kernels that stay hand-written beside them

// 256-thread workgroup per image, two walks over the keys
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

// the first ngroups lanes of one workgroup: d_radial.  It indexes by threadIdx.x alone, which bundle_image_kernel would
// not
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

// The device executor of bundle_schedule (bundle_host.hpp): a phase is one launch of the kernel of its shape on the
// context stream, a scope one profile entry (misift_profile_read: tools/bundle_time.py reports their shares).
struct BundleDeviceExec {
  misift_ctx *ctx;
  const BundleData &D;
  const dim3 th{BUNDLE_THREADS}, one{1};
  template <class K, class... A>
  void launch(K kernel, dim3 grid, A... a)
  {
    hipLaunchKernelGGL(kernel, grid, th, 0, ctx->stream, D, a...);
  }
  int clear()
  {
    HIP_TRY(hipMemsetAsync(D.owner, 0xff, sizeof(int) * (size_t)D.s.max_obs, ctx->stream));
    HIP_TRY(hipMemsetAsync(D.ctl, 0, sizeof(int) * BUNDLE_CTL, ctx->stream));
    HIP_TRY(hipMemsetAsync(D.summary, 0, 8 * sizeof(int), ctx->stream));
    return MISIFT_OK;
  }
  template <class F>
  int scope(const char *entry, F phases)
  {
    LaunchScope ls(ctx, entry);
    phases();
    return ls.finish();
  }
  void candidates() { launch_track_candidates(ctx, D.s, D.owner, D.key); }
  void gather() { launch(bundle_gather_kernel, dim3((unsigned)D.s.nimages)); }
  template <class P, class... A>
  void slots(A... a)
  {
    launch(bundle_slot_kernel<P, A...>, bundle_blocks(D.s.max_obs), a...);
  }
  template <class P, class... A>
  void tracks(A... a)
  {
    launch(bundle_track_kernel<P, A...>, bundle_blocks(D.s.max_tracks), a...);
  }
  template <class P, class... A>
  void images(A... a)
  {
    const int lanes = P::GROUPS && D.s.nimages < BUNDLE_MAX_GROUPS ? BUNDLE_MAX_GROUPS : D.s.nimages;
    launch(bundle_image_kernel<P, A...>, bundle_blocks(lanes), a...);
  }
  template <class P, class... A>
  void image_sums(A... a)
  {
    launch(bundle_image_sum_kernel<P, A...>, dim3((unsigned)D.s.nimages), a...);
  }
  template <class P>
  void scalar()
  {
    launch(bundle_scalar_kernel<P>, one);
  }
  void radial_out(bool refined, bool radial) { launch(bundle_radial_out_kernel, one, refined ? 1 : 0, radial ? 1 : 0); }
};

}  // namespace

size_t adjust_bundle_batch_tmp_bytes(int max_tracks, int max_obs, int nimages, bool focal, bool radial)
{
  BundleData D;
  D.s.max_tracks = max_tracks; D.s.max_obs = max_obs; D.s.nimages = nimages;
  return bundle_layout(D, nullptr, focal, radial);
}

// Enqueue any of the four bundle calls on the context stream (common.hpp): three memsets and the launches of
// bundle_schedule.
int launch_adjust_bundle_batch(misift_ctx *ctx, const TrackScene &scene, const BundleCall &call,
                               const BundleDerived &derived, const BundleLists &pinned)
{
  const bool focal = derived.focal, radial = derived.radial;
  const int rc = misift_ensure_tmp(ctx, adjust_bundle_batch_tmp_bytes(scene.max_tracks, scene.max_obs, scene.nimages,
                                                                      focal, radial));
  if (rc) return rc;
  BundleData D = bundle_data(scene, call, derived, pinned);
  bundle_layout(D, reinterpret_cast<char *>(ctx->d_match_tmp), focal, radial);
  BundleDeviceExec x{ctx, D};
  return bundle_run(x, D, focal, radial);
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
static int bundle_hook(const char *who, bool ok, const BundleCall &call)
{
  if (ok && bundle_host(call)) return MISIFT_OK;
  misift_set_error((std::string(who) + ": invalid argument").c_str());
  return MISIFT_EINVAL;
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

// Test-only, host-only: the whole call on host arrays, phase after phase through bundle_schedule.
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
  return bundle_hook(__func__, intrinsics_out && (ngroups <= 0 || (focal && radial_out)),
                     {.max_tracks = max_tracks, .max_obs = max_obs, .track_offsets = track_offsets,
                      .obs = reinterpret_cast<const TrackObs *>(obs), .export_summary = export_summary, .points = points,
                      .point_status = point_status, .nimages = nimages, .cam = cam, .cam_pair = cam_pair,
                      .intrinsics = intrinsics, .nhold = nhold, .hold = hold, .min_views = min_views, .min_obs = min_obs,
                      .num_loops = num_loops, .cg_iters = cg_iters, .max_error = max_error, .lambda0 = lambda0,
                      .orthonormalise = orthonormalise, .loss = loss, .loss_scale = loss_scale, .ngroups = ngroups,
                      .group = group, .radial_call = true, .radial = radial, .k0 = k0, .cam_out = cam_out,
                      .points_out = points_out, .cam_obs = cam_obs, .cam_status = cam_status, .cam_rms = cam_rms,
                      .point_obs = point_obs, .history = history, .cost = cost, .obs_weight = obs_weight,
                      .summary = summary, .intrinsics_out = intrinsics_out, .focal_out = focal,
                      .radial_out = reinterpret_cast<int *>(radial_out)});
}

// The same for misift_adjust_bundle_focal_batch.
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
  return bundle_hook(__func__, intrinsics_out && (ngroups <= 0 || focal),
                     {.max_tracks = max_tracks, .max_obs = max_obs, .track_offsets = track_offsets,
                      .obs = reinterpret_cast<const TrackObs *>(obs), .export_summary = export_summary, .points = points,
                      .point_status = point_status, .nimages = nimages, .cam = cam, .cam_pair = cam_pair,
                      .intrinsics = intrinsics, .nhold = nhold, .hold = hold, .min_views = min_views, .min_obs = min_obs,
                      .num_loops = num_loops, .cg_iters = cg_iters, .max_error = max_error, .lambda0 = lambda0,
                      .orthonormalise = orthonormalise, .loss = loss, .loss_scale = loss_scale, .ngroups = ngroups,
                      .group = group, .cam_out = cam_out, .points_out = points_out, .cam_obs = cam_obs,
                      .cam_status = cam_status, .cam_rms = cam_rms, .point_obs = point_obs, .history = history,
                      .cost = cost, .obs_weight = obs_weight, .summary = summary, .intrinsics_out = intrinsics_out,
                      .focal_out = focal});
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
  return bundle_hook(__func__, true,
                     {.max_tracks = max_tracks, .max_obs = max_obs, .track_offsets = track_offsets,
                      .obs = reinterpret_cast<const TrackObs *>(obs), .export_summary = export_summary, .points = points,
                      .point_status = point_status, .nimages = nimages, .cam = cam, .cam_pair = cam_pair,
                      .intrinsics = intrinsics, .nhold = nhold, .hold = hold, .min_views = min_views, .min_obs = min_obs,
                      .num_loops = num_loops, .cg_iters = cg_iters, .max_error = max_error, .lambda0 = lambda0,
                      .orthonormalise = orthonormalise, .loss = loss, .loss_scale = loss_scale, .cam_out = cam_out,
                      .points_out = points_out, .cam_obs = cam_obs, .cam_status = cam_status, .cam_rms = cam_rms,
                      .point_obs = point_obs, .history = history, .cost = cost, .obs_weight = obs_weight,
                      .summary = summary});
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

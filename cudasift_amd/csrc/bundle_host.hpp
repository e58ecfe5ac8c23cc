// bundle_host.hpp — the host's side of the bundle calls, shared by the device path and the test hooks: the temp layout;
// the call as one struct (BundleCall), what is derived from it (bundle_derive) and the BundleData both sides run on
// (bundle_data); the order of the phases of bundle_core.hpp, written once (bundle_schedule) over an executor; and the
// host executor with the whole call on host arrays (bundle_host).  kernels_bundle.hip holds the device executor and
// wraps bundle_host into the test hooks (misift_test_adjust_bundle*); tools/bundle_radial_sanitize.cpp runs it under the
// sanitizers.  Host code only.
#pragma once
#include <stdint.h>
#include <vector>
#include "bundle_core.hpp"

// the temp of the call laid out behind `base` (NULL: only the size is wanted); every array starts 16-byte aligned
inline size_t bundle_layout(BundleData &D, char *base, bool focal = false, bool radial = false)
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
  if (!radial) return at;
  D.ks = reinterpret_cast<float *>(take(4 * 2 * BUNDLE_MAX_GROUPS));
  D.kvec = reinterpret_cast<float *>(take(4 * 5 * BUNDLE_MAX_GROUPS));
  D.ksc = reinterpret_cast<float *>(take(4 * 3 * BUNDLE_MAX_GROUPS));
  D.rlin = reinterpret_cast<float *>(take(4 * 2 * mo));
  D.tkd = reinterpret_cast<float *>(take(4 * BUNDLE_MAX_GROUPS * mt));
  D.iuk = reinterpret_cast<float *>(take(4 * BUNDLE_IMAGE_RADIAL * n));
  D.ikv = reinterpret_cast<float *>(take(4 * 2 * n));
  return at;
}

// ---- one call description

// The public arguments of the four calls (include/misift.h) in one struct; what a call does not have is NULL or 0.  The
// plain call is loss 0 without obs_weight, the robust call ngroups 0 without intrinsics_out.  The pointers are the
// device's for the entry points and the host's for the hooks.
struct BundleCall {
  int max_tracks, max_obs;
  const int *track_offsets;
  const TrackObs *obs;
  const int *export_summary;
  const float *points;
  const int *point_status;
  int nimages;
  const float *cam;
  const int *cam_pair;
  const float *intrinsics;                     // host
  int nhold;
  const int *hold;                             // host
  int min_views, min_obs, num_loops, cg_iters;
  float max_error, lambda0;
  int orthonormalise, loss;
  float loss_scale;
  int ngroups;
  const int *group;                            // host
  bool radial_call;                            // misift_adjust_bundle_radial_batch: its two lists may both be NULL
  const int *radial;                           // host, ngroups flags
  const float *k0;                             // host, ngroups
  float *cam_out, *points_out;
  int *cam_obs, *cam_status;
  float *cam_rms;
  int *point_obs;
  float *history, *cost, *obs_weight;
  int *summary;
  float *intrinsics_out;
  int *focal_out, *radial_out;
};

// What a call with valid arguments derives from them, once, for the device and the hook alike.
struct BundleDerived {
  bool focal;                                  // an image has a group: the FOCAL instances run
  bool radial;                                 // and some k_g is an unknown or starts off zero: the RADIAL ones
  int rad[BUNDLE_MAX_GROUPS];                  // the flags and k0, 0 from ngroups on
  float k0[BUNDLE_MAX_GROUPS];
  float thresh2, c, c2;                        // max_error^2; the loss scale (0 with loss 0) and its square: each
                                               // rounded once, here, so that host and device read the same bits
  std::vector<int> held;                       // nimages flags
  std::vector<int> none;                       // nimages times -1 where intrinsics_out is wanted without a group
};
inline BundleDerived bundle_derive(const BundleCall &c)
{
  BundleDerived d{};
  for (int i = 0; c.ngroups > 0 && i < c.nimages; i++) d.focal = d.focal || c.group[i] >= 0;
  for (int g = 0; c.radial && g < c.ngroups; g++) {
    d.rad[g] = c.radial[g];
    d.k0[g] = c.k0[g];
    d.radial = d.radial || (d.focal && (d.rad[g] != 0 || d.k0[g] != 0.0f));
  }
  d.thresh2 = c.max_error * c.max_error;
  d.c = c.loss != BUNDLE_LOSS_NONE ? c.loss_scale : 0.0f;
  d.c2 = d.c * d.c;
  d.held.assign(c.nimages, 0);
  for (int j = 0; j < c.nhold; j++) d.held[c.hold[j]] = 1;
  d.none.assign(c.intrinsics_out && c.ngroups == 0 ? c.nimages : 0, -1);
  return d;
}

// The lists the phases read through host pointers: the entry points' pinned copies, or for the hook what
// bundle_derive left.  rad and k0 are NULL unless the call is the radial one.
struct BundleLists {
  const int *held, *group, *rad;
  const float *k0;
};

// The arguments and the outputs of the call as the phases read them; the temp is bundle_layout's to add.
inline BundleData bundle_data(const TrackScene &scene, const BundleCall &c, const BundleDerived &d, const BundleLists &l)
{
  BundleData D{};
  D.s = scene;
  D.min_views = c.min_views; D.min_obs = c.min_obs; D.num_loops = c.num_loops; D.cg_iters = c.cg_iters;
  D.orthonormalise = c.orthonormalise; D.thresh2 = d.thresh2; D.lambda0 = c.lambda0;
  D.loss = c.loss; D.loss_scale = d.c; D.loss_scale2 = d.c2;
  D.held = l.held; D.ngroups = c.ngroups; D.grp = l.group; D.rad = l.rad; D.k0 = l.k0;
  D.cam_out = c.cam_out; D.points_out = c.points_out; D.cam_rms = c.cam_rms; D.history = c.history; D.cost = c.cost;
  D.cam_obs = c.cam_obs; D.cam_status = c.cam_status; D.point_obs = c.point_obs; D.summary = c.summary;
  D.obs_weight = c.obs_weight; D.intrinsics_out = c.intrinsics_out; D.focal_out = c.focal_out;
  D.radial_out = c.radial_out;
  return D;
}

// ---- one schedule

// The order of the phases, for the device and the hook alike.  X is the executor: slots, tracks, images, image_sums and
// scalar run a phase type of bundle_core.hpp over its work items (a launch, or a loop), scope groups them under a
// profile entry and gives 0 or the error that ends the call.  What differs by nature between the two sides is a named
// step of the executor: clear (the owners -1, the control words and the summary 0), candidates (the owner of every slot
// and the image it is a candidate of), gather (every image's members listed in ascending slot, an image with too few
// demoted) and radial_out (d_radial from the first ngroups lanes of one workgroup).
template <bool ROBUST, bool FOCAL, bool RADIAL, class X>
inline int bundle_schedule(X &x, const BundleData &D)
{
  int r = x.clear();
  auto step = [&](const char *entry, auto phases) {
    if (!r) r = x.scope(entry, phases);
  };
  step("bundle_setup", [&] {
    x.candidates();
    x.template images<BundleImageInit>();
    x.template slots<BundlePremember<RADIAL>>();
    x.template tracks<BundleActivate>();
    x.gather();
    if (FOCAL) x.template scalar<BundleGroupInit<RADIAL>>();
    x.template slots<BundleEval<ROBUST, FOCAL, RADIAL>>(0);
    x.template image_sums<BundleCost>(0);
    x.template scalar<BundleStart>();
  });
  for (int loop = 0; loop < D.num_loops; loop++) {
    // the normal equations, the points eliminated
    step("bundle_track", [&] { x.template tracks<BundleTrackNormal<ROBUST, FOCAL, RADIAL>>(); });
    step("bundle_image", [&] { x.template image_sums<BundleImageNormal<FOCAL, RADIAL>>(); });
    // the reduced system by conjugate gradients
    step("bundle_scalar", [&] { x.template scalar<BundleCgStart<FOCAL, RADIAL>>(); });
    for (int it = 0; it < D.cg_iters; it++) {
      step("bundle_track", [&] { x.template tracks<BundleCgTrack<FOCAL, RADIAL>>(); });
      step("bundle_image", [&] { x.template image_sums<BundleCgImage<FOCAL, RADIAL>>(); });
      step("bundle_scalar", [&] { x.template scalar<BundleCgScalar<FOCAL, RADIAL>>(); });
    }
    // the trial state, its cost, kept or turned away
    step("bundle_track", [&] { x.template tracks<BundleTrackTrial<FOCAL, RADIAL>>(); });
    step("bundle_trial", [&] {
      x.template images<BundleImageTrial<FOCAL, RADIAL>>();
      x.template slots<BundleEval<ROBUST, FOCAL, RADIAL>>(1);
    });
    step("bundle_image", [&] { x.template image_sums<BundleCost>(1); });
    step("bundle_scalar", [&] { x.template scalar<BundleDecide>(); });
  }
  step("bundle_out", [&] {
    x.template images<BundleImageOut>();
    x.template tracks<BundleTrackOut>();
    if (D.obs_weight) x.template slots<BundleWeightOut<FOCAL, RADIAL>>();
    if (D.intrinsics_out) x.template images<BundleIntrinsicsOut>(FOCAL ? 1 : 0);
    if (D.radial_out && D.ngroups > 0) x.radial_out(FOCAL, RADIAL);
  });
  return r;
}

// the loss and the model are the same for the whole call: one of six instances of the schedule, picked here and nowhere else
template <class X>
inline int bundle_run(X &x, const BundleData &D, bool focal, bool radial)
{
  const bool robust = D.loss != BUNDLE_LOSS_NONE;
  if (radial) return robust ? bundle_schedule<true, true, true>(x, D) : bundle_schedule<false, true, true>(x, D);
  if (focal) return robust ? bundle_schedule<true, true, false>(x, D) : bundle_schedule<false, true, false>(x, D);
  return robust ? bundle_schedule<true, false, false>(x, D) : bundle_schedule<false, false, false>(x, D);
}

// ---- the host executor: every phase a loop over its work items, the workgroup's sums by BundleHostSum

struct BundleHostExec {
  const BundleData &D;
  const int T, O;
  BundleHostSum S;
  int clear()
  {
    for (int o = 0; o < D.s.max_obs; o++) D.owner[o] = -1;
    for (int j = 0; j < BUNDLE_CTL; j++) D.ctl[j] = 0;
    for (int j = 0; j < 8; j++) D.summary[j] = 0;
    return 0;
  }
  template <class F>
  int scope(const char *, F phases)
  {
    phases();
    return 0;
  }
  void candidates()                            // as launch_track_candidates
  {
    for (int t = 0; t < T; t++) scene_track_owns(D.s, D.owner, t);
    for (int o = 0; o < O; o++) D.key[o] = scene_slot_key(D.s, D.owner, o);
  }
  void gather()
  {
    int at = 0;
    for (int i = 0; i < D.s.nimages; i++) {
      D.istart[i] = at;
      for (int o = 0; o < O; o++)
        if (D.key[o] == i) D.list[at++] = o;
      D.icount[i] = at - D.istart[i];
      if (D.istate[i] == BUNDLE_ADJUSTED && D.icount[i] < D.min_obs) D.istate[i] = BUNDLE_FEW_OBS;
    }
  }
  template <class P, class... A>
  void slots(A... a)
  {
    for (int o = 0; o < O; o++) P::run(D, o, a...);
  }
  template <class P, class... A>
  void tracks(A... a)
  {
    for (int t = 0; t < T; t++) P::run(D, t, a...);
  }
  template <class P, class... A>
  void images(A... a)
  {
    for (int i = 0; i < D.s.nimages; i++) P::run(D, i, a...);
    if constexpr (P::GROUPS)
      for (int g = 0; g < P::groups(D); g++) P::group(D, g, a...);
  }
  template <class P, class... A>
  void image_sums(A... a)
  {
    for (int i = 0; i < D.s.nimages; i++) P::template run<BundleHostSum>(D, S, i, true, a...);
  }
  template <class P>
  void scalar()
  {
    P::template run<BundleHostSum>(D, S, 0, 1, true);
  }
  void radial_out(bool refined, bool radial)
  {
    for (int g = 0; g < D.ngroups; g++) bundle_radial_out(D, g, refined, radial);
  }
};

// The rules of the hooks: false for an argument set the calls refuse (the context and the device's alignment and
// aliasing rules aside, which the entry points check for themselves).
inline bool bundle_call_ok(const BundleCall &c)
{
  bool ok = c.max_tracks >= 1 && c.max_obs >= 1 && c.nimages >= 1 && c.track_offsets && c.obs && c.export_summary &&
            c.points && c.point_status && c.cam && c.cam_pair && c.intrinsics && c.nhold >= 0 &&
            (c.nhold == 0 || c.hold) && c.min_views >= 2 && c.min_obs >= 3 && c.num_loops >= 0 && c.cg_iters >= 0 &&
            c.max_error > 0.0f && c.lambda0 > 0.0f && fundamental_finite(c.lambda0) &&
            (c.orthonormalise == 0 || c.orthonormalise == 1) && c.cam_out && c.points_out && c.cam_obs &&
            c.cam_status && c.cam_rms && c.point_obs && (c.history || c.num_loops == 0) && c.cost && c.summary &&
            c.loss >= BUNDLE_LOSS_NONE && c.loss <= BUNDLE_LOSS_GEMAN_MCCLURE &&
            (c.loss == BUNDLE_LOSS_NONE || (c.loss_scale > 0.0f && fundamental_finite(c.loss_scale)));
  for (int j = 0; ok && j < c.nhold; j++) ok = c.hold[j] >= 0 && c.hold[j] < c.nimages;
  ok = ok && c.ngroups >= 0 && c.ngroups <= BUNDLE_MAX_GROUPS && (c.ngroups == 0 || c.group);
  for (int i = 0; ok && c.ngroups > 0 && i < c.nimages; i++) ok = c.group[i] >= -1 && c.group[i] < c.ngroups;
  ok = ok && (c.radial != nullptr) == (c.k0 != nullptr);
  for (int g = 0; ok && c.radial && g < c.ngroups; g++)
    ok = (c.radial[g] == 0 || c.radial[g] == 1) && fundamental_finite(c.k0[g]);
  return ok;
}

// The hooks' common body: the whole call on host arrays.  false: an invalid argument, nothing written.
inline bool bundle_host(const BundleCall &c)
{
  if (!bundle_call_ok(c)) return false;
  const BundleDerived d = bundle_derive(c);
  const TrackScene scene{c.max_tracks, c.max_obs, c.nimages, c.track_offsets, c.obs, c.export_summary,
                         c.points, c.point_status, c.cam, c.cam_pair, c.intrinsics};
  BundleData D = bundle_data(scene, c, d, {d.held.data(), c.ngroups > 0 ? c.group : d.none.data(), d.rad, d.k0});
  std::vector<char> tmp(bundle_layout(D, nullptr, d.focal, d.radial) + 16, 0);
  bundle_layout(D, reinterpret_cast<char *>(((uintptr_t)tmp.data() + 15) & ~(uintptr_t)15), d.focal, d.radial);
  BundleHostExec x{D, scene_T(D.s), scene_O(D.s), {}};
  bundle_run(x, D, d.focal, d.radial);
  return true;
}

// misift_undistort_obs_batch on host arrays; false: an invalid argument, nothing written
inline bool bundle_host_undistort(int max_obs, const TrackObs *obs, const int *export_summary, int nimages,
                                  const float *intrinsics, int ngroups, const int *group, const int *radial,
                                  TrackObs *obs_out)
{
  bool ok = max_obs >= 1 && obs && export_summary && nimages >= 1 && intrinsics && obs_out && ngroups >= 0 &&
            ngroups <= BUNDLE_MAX_GROUPS && (ngroups == 0 || (group && radial));
  for (int i = 0; ok && ngroups > 0 && i < nimages; i++) ok = group[i] >= -1 && group[i] < ngroups;
  if (!ok) return false;
  const std::vector<int> none(nimages, -1);
  const int O = scene_clamp(export_summary[3], max_obs);
  for (int o = 0; o < O; o++)
    obs_out[o] = bundle_undistort_obs(obs[o], nimages, intrinsics, ngroups > 0 ? group : none.data(), radial);
  return true;
}

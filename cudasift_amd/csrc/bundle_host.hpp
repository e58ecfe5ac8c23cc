// bundle_host.hpp — the host's side of the bundle calls: the temp layout, the phases of bundle_core.hpp in the order of
// the launches, and the whole call on host arrays.  kernels_bundle.hip wraps bundle_host into the test hooks
// (misift_test_adjust_bundle*); tools/bundle_radial_sanitize.cpp runs it under the sanitizers.  Host code only.
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


// the phases of the host hook that read the loss
template <bool ROBUST, bool FOCAL, bool RADIAL>
inline void bundle_host_eval(const BundleData &D, int O, bool trial)
{
  for (int o = 0; o < O; o++) bundle_eval_slot<ROBUST, FOCAL, RADIAL>(D, o, trial);
}
template <bool ROBUST, bool FOCAL, bool RADIAL>
inline void bundle_host_track_normal(const BundleData &D, int T)
{
  for (int t = 0; t < T; t++) FOCAL ? bundle_track_normal_focal<ROBUST, RADIAL>(D, t) : bundle_track_normal<ROBUST>(D, t);
}

// the phases of the hook in the order of the launches
template <bool ROBUST, bool FOCAL, bool RADIAL = false>
inline void bundle_host_run(const BundleData &D, int T, int O)
{
  const int nimages = D.s.nimages;
  BundleHostSum S;
  if (FOCAL) bundle_focal_init<RADIAL>(D, S, 0, 1);
  bundle_host_eval<ROBUST, FOCAL, RADIAL>(D, O, false);
  for (int i = 0; i < nimages; i++) bundle_image_cost(D, S, i, false, true);
  bundle_scalar_init(D, S, true);
  for (int loop = 0; loop < D.num_loops; loop++) {
    bundle_host_track_normal<ROBUST, FOCAL, RADIAL>(D, T);
    for (int i = 0; i < nimages; i++) {
      if (RADIAL) bundle_image_normal_radial(D, S, i, true);
      else FOCAL ? bundle_image_normal_focal(D, S, i, true) : bundle_image_normal(D, S, i, true);
    }
    bundle_cg_start<FOCAL, RADIAL>(D, S, 0, 1, true);
    for (int it = 0; it < D.cg_iters; it++) {
      for (int t = 0; t < T; t++) bundle_cg_track<FOCAL, RADIAL>(D, t);
      for (int i = 0; i < nimages; i++) {
        if (RADIAL) bundle_cg_image_radial(D, S, i, true);
        else FOCAL ? bundle_cg_image_focal(D, S, i, true) : bundle_cg_image(D, S, i, true);
      }
      bundle_cg_scalar<FOCAL, RADIAL>(D, S, 0, 1, true);
    }
    for (int t = 0; t < T; t++) bundle_track_trial<FOCAL, RADIAL>(D, t);
    for (int i = 0; i < nimages; i++) bundle_image_trial(D, i);
    if (FOCAL)
      for (int g = 0; g < BUNDLE_MAX_GROUPS; g++) bundle_focal_trial(D, g);
    if (RADIAL)
      for (int g = 0; g < BUNDLE_MAX_GROUPS; g++) bundle_radial_trial(D, g);
    bundle_host_eval<ROBUST, FOCAL, RADIAL>(D, O, true);
    for (int i = 0; i < nimages; i++) bundle_image_cost(D, S, i, true, true);
    bundle_decide(D, S, 0, 1, true);
  }
  for (int i = 0; i < nimages; i++) bundle_image_out(D, i);
  for (int t = 0; t < T; t++) bundle_track_out(D, t);
  if (D.obs_weight)
    for (int o = 0; o < O; o++) bundle_weight_slot<FOCAL, RADIAL>(D, o);
  if (D.intrinsics_out) {
    for (int i = 0; i < nimages; i++) bundle_intrinsics_out(D, i, FOCAL);
    for (int g = 0; g < D.ngroups; g++) bundle_focal_out(D, g, FOCAL);
  }
  if (D.radial_out)
    for (int g = 0; g < D.ngroups; g++) bundle_radial_out(D, g, FOCAL, RADIAL);
}

// The hooks' common body: the whole call on host arrays; ngroups 0 and no intrinsics_out is the robust call, no
// radial_flags the focal call.  false: an invalid argument, nothing written.
inline bool bundle_host(int max_tracks, int max_obs, const int *track_offsets, const TrackObs *obs,
                        const int *export_summary, const float *points, const int *point_status, int nimages,
                        const float *cam, const int *cam_pair, const float *intrinsics, int nhold, const int *hold,
                        int min_views, int min_obs, int num_loops, int cg_iters, float max_error, float lambda0,
                        int orthonormalise, int loss, float loss_scale, int ngroups, const int *group, float *cam_out,
                        float *points_out, int *cam_obs, int *cam_status, float *cam_rms, int *point_obs, float *history,
                        float *cost, float *obs_weight, int *summary, float *intrinsics_out, int *focal_out,
                        const int *radial_flags = nullptr, const float *k0 = nullptr, int *radial_out = nullptr)
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
  // the radial call: the flags and k0 padded to BUNDLE_MAX_GROUPS; on: the RADIAL instances run
  int rad[BUNDLE_MAX_GROUPS] = {0};
  float kstart[BUNDLE_MAX_GROUPS] = {0.0f};
  bool radial = false;
  ok = ok && (radial_flags != nullptr) == (k0 != nullptr);
  for (int g = 0; ok && radial_flags && g < ngroups; g++) {
    ok = (radial_flags[g] == 0 || radial_flags[g] == 1) && fundamental_finite(k0[g]);
    rad[g] = radial_flags[g];
    kstart[g] = k0[g];
    radial = radial || (focal && (rad[g] != 0 || kstart[g] != 0.0f));
  }
  if (!ok) return false;
  BundleData D;
  D.rad = rad; D.k0 = kstart; D.radial_out = radial_out;
  D.ngroups = ngroups; D.grp = ngroups > 0 ? group : nullptr; D.intrinsics_out = intrinsics_out; D.focal_out = focal_out;
  D.s = TrackScene{max_tracks, max_obs, nimages, track_offsets, obs, export_summary,
                   points, point_status, cam, cam_pair, intrinsics};
  D.min_views = min_views; D.min_obs = min_obs; D.num_loops = num_loops; D.cg_iters = cg_iters;
  D.orthonormalise = orthonormalise;
  D.thresh2 = max_error * max_error; D.lambda0 = lambda0;
  const bool robust = loss != BUNDLE_LOSS_NONE;
  D.loss = loss; D.loss_scale = robust ? loss_scale : 0.0f; D.loss_scale2 = D.loss_scale * D.loss_scale;
  std::vector<int> held(nimages, 0);
  for (int j = 0; j < nhold; j++) held[hold[j]] = 1;
  D.held = held.data();
  std::vector<char> tmp(bundle_layout(D, nullptr, focal, radial) + 16, 0);
  bundle_layout(D, reinterpret_cast<char *>(((uintptr_t)tmp.data() + 15) & ~(uintptr_t)15), focal, radial);
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
  for (int o = 0; o < O; o++) radial ? bundle_slot_premember<true>(D, o) : bundle_slot_premember(D, o);
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
  if (radial) robust ? bundle_host_run<true, true, true>(D, T, O) : bundle_host_run<false, true, true>(D, T, O);
  else if (focal) robust ? bundle_host_run<true, true>(D, T, O) : bundle_host_run<false, true>(D, T, O);
  else robust ? bundle_host_run<true, false>(D, T, O) : bundle_host_run<false, false>(D, T, O);
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

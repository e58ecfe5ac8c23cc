// triangulate_core.hpp — the arithmetic of misift_triangulate_tracks_batch, for host and device: which observation is a
// usable view, the normal equations of the linear start and of a Gauss-Newton step, the 3x3 LDL^T solve, the residuals
// of a point, and the whole of one track.  The kernel (kernels_triangulate.hip) and the host-only test hook
// (misift_test_triangulate_track) compile these same functions, so what a CPU test pins is what the device runs.  The
// definition, step by step, is in include/misift.h.
//
// The rules of pose_core.hpp hold: fp32 with every operation rounded, only + - * / and sqrtf, no fmaf, and the build's
// -ffp-contract=off.  Every sum runs in ascending k over the observations and left to right as the header states it.
//
// A function here reads the cameras through a `Cams` (cam(i): the twelve floats of image i, k(i): its fx fy cx cy,
// set(i): whether it has a camera whose floats are all finite), so the kernel can hand in its LDS copy or the global
// arrays and the hook plain host arrays.
//
// The scene that the five track-chain calls share (triangulate, refine, resect, adjust, filter) is stated here once:
// TrackObs and how it is loaded, TrackScene with T and O, and, at the end of the file, the candidate rule of
// include/misift.h (misift_refine_cameras_batch) as the two functions that the candidate kernels
// (kernels_track_candidates.hip) and the host hooks both run.
#pragma once
#include <math.h>
#include "posegraph_core.hpp"

enum { TRI_OK = 0, TRI_FEW_VIEWS = 1, TRI_SINGULAR = 2, TRI_BEHIND = 3, TRI_BAD_RANGE = 4 };

// misift_track_obs (the static_assert is in common.hpp, which sees both).  The type is as aligned as its
// fields: a host hook reads the caller's array where it lies.
struct TrackObs {
  int frame, record;
  float xpos, ypos;
};

// One observation.  On the device it is one 16-byte load: every entry point rejects a d_obs that is not 16-byte aligned
// (check_scene, misift_host.hip), and this is the one place that relies on it.
FUND_HD TrackObs track_obs_load(const TrackObs *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return *static_cast<const TrackObs *>(__builtin_assume_aligned(p, 16));
#else
  return *p;
#endif
}

// what the five calls are given: the lists of misift_export_tracks_batch, the points of triangulate (NULL in triangulate
// itself) and the cameras
struct TrackScene {
  int max_tracks, max_obs, nimages;
  const int *track_offsets;
  const TrackObs *obs;
  const int *export_summary;
  const float *points;                         // max_tracks x 4
  const int *point_status;
  const float *cam;                            // nimages x 12
  const int *cam_pair;
  const float *intrinsics;                     // nimages x 4
};

FUND_HD int scene_clamp(int v, int hi) { const int lo = v > 0 ? v : 0; return lo < hi ? lo : hi; }   // min(max(v, 0), hi)
FUND_HD int scene_T(const TrackScene &S) { return scene_clamp(S.export_summary[2], S.max_tracks); }
FUND_HD int scene_O(const TrackScene &S) { return scene_clamp(S.export_summary[3], S.max_obs); }

// the cameras as misift_link_poses_batch leaves them and the intrinsics as the caller lists them
struct TriCamsPlain {
  const float *cams;                           // nimages x 12
  const int *cam_pair;                         // nimages
  const float *intrinsics;                     // nimages x 4
  FUND_HD const float *cam(int i) const { return cams + 12 * (size_t)i; }
  FUND_HD const float *k(int i) const { return intrinsics + 4 * (size_t)i; }
  FUND_HD bool set(int i) const
  {
    bool ok = cam_pair[i] != POSEGRAPH_UNSET;
    const float *c = cam(i);
    for (int j = 0; j < 12; j++) ok = ok && fundamental_finite(c[j]);
    return ok;
  }
};

// the six unique entries of a symmetric 3x3 and a right-hand side
struct TriNormal {
  float m00, m01, m02, m11, m12, m22, g0, g1, g2;
};

FUND_HD void tri_clear(TriNormal &N) { N.m00 = N.m01 = N.m02 = N.m11 = N.m12 = N.m22 = N.g0 = N.g1 = N.g2 = 0.0f; }

// M += a a^T, g += a rhs
FUND_HD void tri_accumulate(TriNormal &N, float a0, float a1, float a2, float rhs)
{
  N.m00 = N.m00 + a0 * a0; N.m01 = N.m01 + a0 * a1; N.m02 = N.m02 + a0 * a2;
  N.m11 = N.m11 + a1 * a1; N.m12 = N.m12 + a1 * a2; N.m22 = N.m22 + a2 * a2;
  N.g0 = N.g0 + a0 * rhs; N.g1 = N.g1 + a1 * rhs; N.g2 = N.g2 + a2 * rhs;
}

FUND_HD bool tri_pivot(float d) { return d > 0.0f && fundamental_finite(d); }

// M x = g by LDL^T without pivoting; false for a pivot that is not finite and > 0 or a non-finite x
FUND_HD bool tri_solve(const TriNormal &N, float (&x)[3])
{
  x[0] = x[1] = x[2] = 0.0f;
  const float d0 = N.m00;
  if (!tri_pivot(d0)) return false;
  const float l10 = N.m01 / d0, l20 = N.m02 / d0;
  const float d1 = N.m11 - l10 * N.m01;
  if (!tri_pivot(d1)) return false;
  const float e = N.m12 - l20 * N.m01;
  const float l21 = e / d1;
  const float d2 = (N.m22 - l20 * N.m02) - l21 * e;
  if (!tri_pivot(d2)) return false;
  const float y0 = N.g0, y1 = N.g1 - l10 * y0, y2 = (N.g2 - l20 * y0) - l21 * y1;
  const float x2 = y2 / d2, x1 = y1 / d1 - l21 * x2, x0 = (y0 / d0 - l10 * x1) - l20 * x2;
  if (!(fundamental_finite(x0) && fundamental_finite(x1) && fundamental_finite(x2))) return false;
  x[0] = x0; x[1] = x1; x[2] = x2;
  return true;
}

// step 1: observation o is a usable view
template <class Cams>
FUND_HD bool tri_usable(const Cams &C, int nimages, const TrackObs &o)
{
  const int f = o.frame;
  if (!(f >= 0 && f < nimages)) return false;  // before it addresses anything
  return fundamental_finite(o.xpos) && fundamental_finite(o.ypos) && C.set(f);
}

// step 2: the two rows of one usable view
FUND_HD void tri_linear_rows(const float *c, const float *k, float x, float y, TriNormal &N)
{
  const float u = (x - k[2]) / k[0], v = (y - k[3]) / k[1];
  tri_accumulate(N, c[0] - u * c[6], c[1] - u * c[7], c[2] - u * c[8], u * c[11] - c[9]);
  tri_accumulate(N, c[3] - v * c[6], c[4] - v * c[7], c[5] - v * c[8], v * c[11] - c[10]);
}

// step 3 for one usable view under X: false when the point is not in front; otherwise (ru, rv) and, with `normal`, the
// view's share of c, M and g
FUND_HD bool tri_view(const float *c, const float *k, float x, float y, const float (&X)[3], float &ru, float &rv,
                      bool normal, float &cost, TriNormal &N)
{
  const float xc = ((c[0] * X[0] + c[1] * X[1]) + c[2] * X[2]) + c[9];
  const float yc = ((c[3] * X[0] + c[4] * X[1]) + c[5] * X[2]) + c[10];
  const float zc = ((c[6] * X[0] + c[7] * X[1]) + c[8] * X[2]) + c[11];
  if (!(zc > 0.0f)) return false;
  const float iz = 1.0f / zc, a = xc * iz, b = yc * iz;
  ru = x - (k[0] * a + k[2]);
  rv = y - (k[1] * b + k[3]);
  if (!normal) return true;
  cost = cost + (ru * ru + rv * rv);
  const float su = k[0] * iz, sv = k[1] * iz;
  tri_accumulate(N, su * (c[0] - a * c[6]), su * (c[1] - a * c[7]), su * (c[2] - a * c[8]), ru);
  tri_accumulate(N, sv * (c[3] - b * c[6]), sv * (c[4] - b * c[7]), sv * (c[5] - b * c[8]), rv);
  return true;
}

// step 3 over a track: false when a used view is not in front
template <class Cams>
FUND_HD bool tri_residuals(const Cams &C, int nimages, const TrackObs *obs, int n, const float (&X)[3], float &cost,
                           TriNormal &N)
{
  cost = 0.0f;
  tri_clear(N);
  TrackObs next = n > 0 ? track_obs_load(obs) : TrackObs{};
  for (int k = 0; k < n; k++) {
    const TrackObs o = next;
    if (k + 1 < n) next = track_obs_load(obs + k + 1);          // the next load is under way while this view is worked on
    if (!tri_usable(C, nimages, o)) continue;
    float ru, rv;
    if (!tri_view(C.cam(o.frame), C.k(o.frame), o.xpos, o.ypos, X, ru, rv, true, cost, N)) return false;
  }
  return true;
}

// Steps 1-5 for one track of n >= 0 observations: the status; point4, *views and, when not NULL, obs_error[0 .. n) as the
// call writes them; *accepted = the Gauss-Newton steps kept.
template <class Cams>
FUND_HD int tri_track(const Cams &C, int nimages, const TrackObs *obs, int n, int min_views, int num_loops, float *point4,
                      int *views, float *obs_error, int *accepted)
{
  const float nan = pose_one_nan(NAN);
  int m = 0, status = TRI_OK, kept = 0;
  float X[3] = {0.0f, 0.0f, 0.0f}, cost = 0.0f;
  TriNormal N;
  tri_clear(N);
  TrackObs next = n > 0 ? track_obs_load(obs) : TrackObs{};
  for (int k = 0; k < n; k++) {
    const TrackObs o = next;
    if (k + 1 < n) next = track_obs_load(obs + k + 1);
    if (!tri_usable(C, nimages, o)) continue;
    m++;
    tri_linear_rows(C.cam(o.frame), C.k(o.frame), o.xpos, o.ypos, N);
  }
  if (m < min_views) status = TRI_FEW_VIEWS;
  else if (!tri_solve(N, X)) status = TRI_SINGULAR;
  else if (!tri_residuals(C, nimages, obs, n, X, cost, N)) status = TRI_BEHIND;
  if (status == TRI_OK) {
    for (int loop = 0; loop < num_loops; loop++) {
      float d[3], cost2;
      TriNormal N2;
      if (!tri_solve(N, d)) break;
      const float X2[3] = {X[0] + d[0], X[1] + d[1], X[2] + d[2]};
      if (!tri_residuals(C, nimages, obs, n, X2, cost2, N2)) break;
      if (!(cost2 < cost)) break;
      X[0] = X2[0]; X[1] = X2[1]; X[2] = X2[2];
      cost = cost2;
      N = N2;
      kept++;
    }
  }
  *views = m;
  *accepted = kept;
  if (status == TRI_OK) {
    point4[0] = X[0]; point4[1] = X[1]; point4[2] = X[2];
    point4[3] = pose_one_nan(sqrtf(cost / (float)m));
  } else {
    point4[0] = point4[1] = point4[2] = point4[3] = nan;
  }
  if (obs_error) {
    if (n > 0) next = track_obs_load(obs);
    for (int k = 0; k < n; k++) {
      float e = nan;
      const TrackObs o = next;
      if (k + 1 < n) next = track_obs_load(obs + k + 1);
      if (status == TRI_OK) {
        float ru, rv;
        if (tri_usable(C, nimages, o) &&
            tri_view(C.cam(o.frame), C.k(o.frame), o.xpos, o.ypos, X, ru, rv, false, cost, N))
          e = pose_one_nan(sqrtf(ru * ru + rv * rv));
      }
      obs_error[k] = e;
    }
  }
  return status;
}

// the track's range in d_obs, from device memory: checked before it addresses anything
FUND_HD bool tri_range_ok(int off, int end, int max_obs) { return 0 <= off && off <= end && end <= max_obs; }

// ---- the candidate rule, for the kernels and the host hooks alike

// what track t < T does to owner[] (-1 everywhere before): a slot ends with the largest valid track that holds it
FUND_HD void scene_track_owns(const TrackScene &S, int *owner, int t)
{
  const int off = S.track_offsets[t], end = S.track_offsets[t + 1];
  if (!tri_range_ok(off, end, scene_O(S))) return;           // before it addresses anything
  for (int o = off; o < end; o++) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(&owner[o], t);
#else
    if (t > owner[o]) owner[o] = t;
#endif
  }
}

// the image slot o < O is a candidate of: its frame when its owner has status 0 and a finite point, its position is
// finite and its frame lies in [0, nimages); otherwise -1
FUND_HD int scene_slot_key(const TrackScene &S, const int *owner, int o)
{
  const int t = owner[o];
  if (t < 0 || S.point_status[t] != TRI_OK) return -1;
  const float *X = S.points + 4 * (size_t)t;
  const TrackObs ob = track_obs_load(S.obs + o);
  const bool ok = fundamental_finite(X[0]) && fundamental_finite(X[1]) && fundamental_finite(X[2]) &&
                  fundamental_finite(ob.xpos) && fundamental_finite(ob.ypos) && ob.frame >= 0 && ob.frame < S.nimages;
  return ok ? ob.frame : -1;
}

// filter_core.hpp — the rules of misift_filter_tracks_batch, for host and device: what becomes of a slot, which of two
// views of one frame loses, a view's unit ray, the pair test of the angle rule, and the rms of the kept views.  The
// kernels (kernels_filter.hip) and the host-only test hook (misift_test_filter_tracks) compile these same functions, so
// what a CPU test pins is what the device runs.  The definition, rule by rule, is in include/misift.h.
//
// The rules of refine_core.hpp hold: fp32 with every operation rounded, only + - * / and sqrtf, no fmaf, and the build's
// -ffp-contract=off; a comparison with a NaN is false.
#pragma once
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "refine_core.hpp"

enum {
  FILTER_NO_OWNER = -1, FILTER_BAD_POINT = -2, FILTER_NOT_USABLE = -3, FILTER_BEHIND = -4, FILTER_ERROR = -5,
  FILTER_DUPLICATE = -6, FILTER_FEW_VIEWS = -7, FILTER_NARROW = -8
};

// rules 1 and 3: the point of a track is bad
FUND_HD bool filter_bad_point(int status, const float *P)
{
  return status != TRI_OK || !(fundamental_finite(P[0]) && fundamental_finite(P[1]) && fundamental_finite(P[2]));
}

// rule 3: the unit ray from the camera centre C = -R^T t to X; a point on the centre gives NaNs, which fail every test
FUND_HD void filter_ray(const float (&c)[12], const float (&X)[3], float (&u)[3])
{
  float d[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float C = -((c[j] * c[9] + c[3 + j] * c[10]) + c[6 + j] * c[11]);
    d[j] = X[j] - C;
  }
  const float n = sqrtf(pose_dot(d, d));
#pragma unroll
  for (int j = 0; j < 3; j++) u[j] = d[j] / n;
}

// rule 1: 0 for a SURVIVOR (with e2 and its ray), otherwise the first reason that applies.  owner < 0: no owner.
template <class Cams>
FUND_HD int filter_classify(const Cams &C, int nimages, int owner, const int *point_status, const float *points,
                            const TrackObs &ob, float E2, float &e2, float (&u)[3])
{
  e2 = 0.0f;
  u[0] = u[1] = u[2] = 0.0f;
  if (owner < 0) return FILTER_NO_OWNER;
  const float *P = points + 4 * (size_t)owner;
  if (filter_bad_point(point_status[owner], P)) return FILTER_BAD_POINT;
  if (!tri_usable(C, nimages, ob)) return FILTER_NOT_USABLE;
  const float *cp = C.cam(ob.frame);
  float c[12];
#pragma unroll
  for (int j = 0; j < 12; j++) c[j] = cp[j];
  const float X[3] = {P[0], P[1], P[2]};
  RefineView v;
  if (!refine_view(c, C.k(ob.frame), X, ob.xpos, ob.ypos, v)) return FILTER_BEHIND;
  e2 = v.ru * v.ru + v.rv * v.rv;
  if (!(e2 < E2)) return FILTER_ERROR;
  filter_ray(c, X, u);
  return 0;
}

// rule 2: the survivor at slot o with e2 loses to the survivor at slot p with e2p of the same track and frame
FUND_HD bool filter_loses(float e2, int o, float e2p, int p) { return e2p < e2 || (e2p == e2 && p < o); }

// rule 3: two kept views are far enough apart
FUND_HD bool filter_pair_wide(const float (&a)[3], const float (&b)[3], float max_cos) { return pose_dot(a, b) < max_cos; }

// rule 4: the fourth word of a surviving point
FUND_HD float filter_rms(float s, int m) { return sqrtf(s / (float)m); }

// The whole call on host arrays, one slot and one track after the other.  obs_map may be NULL.
inline void filter_tracks_host(const TrackScene &S, float E2, float max_cos, int min_views, int unique_frames,
                               int *track_offsets_out, TrackObs *obs_out, int *export_summary_out, float *points_out,
                               int *point_views_out, int *point_status_out, int *track_map, int *obs_map, int *summary)
{
  const int T = scene_T(S), O = scene_O(S), nimages = S.nimages;
  const int *track_offsets = S.track_offsets, *point_status = S.point_status;
  const TrackObs *obs = S.obs;
  const float *points = S.points;
  const TriCamsPlain C{S.cam, S.cam_pair, S.intrinsics};
  std::vector<int> owner(O, -1), code(O, 0);
  std::vector<float> e2(O, 0.0f), ray(3 * (size_t)O, 0.0f);
  for (int t = 0; t < T; t++) scene_track_owns(S, owner.data(), t);
  int sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int o = 0; o < O; o++) {
    float u[3];
    code[o] = filter_classify(C, nimages, owner[o], point_status, points, obs[o], E2, e2[o], u);
    ray[3 * (size_t)o] = u[0]; ray[3 * (size_t)o + 1] = u[1]; ray[3 * (size_t)o + 2] = u[2];
    if (code[o] == FILTER_BEHIND) sum[2]++;
    else if (code[o] == FILTER_ERROR) sum[3]++;
    else if (code[o] < 0) sum[7]++;
  }
  int Tn = 0, On = 0, longest = 0;
  track_offsets_out[0] = 0;
  std::vector<int> kept;
  for (int t = 0; t < T; t++) {
    const int off = track_offsets[t], end = track_offsets[t + 1];
    if (!tri_range_ok(off, end, O)) {
      track_map[t] = FILTER_NO_OWNER;
      continue;
    }
    if (filter_bad_point(point_status[t], points + 4 * (size_t)t)) {
      track_map[t] = FILTER_BAD_POINT;
      continue;
    }
    kept.clear();
    for (int o = off; o < end; o++) {
      if (owner[o] != t || code[o] != 0) continue;
      bool loses = false;
      for (int p = off; unique_frames && p < end && !loses; p++)
        loses = p != o && owner[p] == t && (code[p] == 0 || code[p] == FILTER_DUPLICATE) &&
                obs[p].frame == obs[o].frame && filter_loses(e2[o], o, e2[p], p);
      if (loses) {
        code[o] = FILTER_DUPLICATE;
        sum[4]++;
      } else {
        kept.push_back(o);
      }
    }
    const int m = (int)kept.size();
    int drop = 0;
    if (m < min_views) {
      drop = FILTER_FEW_VIEWS;
    } else if (max_cos < INFINITY) {
      bool wide = false;
      for (int k = 0; k < m && !wide; k++)
        for (int l = k + 1; l < m && !wide; l++) {
          const float *a = &ray[3 * (size_t)kept[k]], *b = &ray[3 * (size_t)kept[l]];
          const float ua[3] = {a[0], a[1], a[2]}, ub[3] = {b[0], b[1], b[2]};
          wide = filter_pair_wide(ua, ub, max_cos);
        }
      if (!wide) drop = FILTER_NARROW;
    }
    if (drop) {
      sum[drop == FILTER_FEW_VIEWS ? 5 : 6]++;
      track_map[t] = drop;
      for (int o : kept) code[o] = drop;
      continue;
    }
    float s = 0.0f;
    for (int k = 0; k < m; k++) {
      obs_out[On + k] = obs[kept[k]];
      code[kept[k]] = On + k;
      s = s + e2[kept[k]];
    }
    memcpy(points_out + 4 * (size_t)Tn, points + 4 * (size_t)t, 3 * sizeof(float));
    points_out[4 * (size_t)Tn + 3] = filter_rms(s, m);
    point_views_out[Tn] = m;
    point_status_out[Tn] = 0;
    track_map[t] = Tn;
    On += m;
    Tn++;
    track_offsets_out[Tn] = On;
    longest = std::max(longest, m);
  }
  if (obs_map)
    for (int o = 0; o < O; o++) obs_map[o] = code[o];
  const int es[8] = {Tn, On, Tn, On, longest, 0, 0, 0};
  memcpy(export_summary_out, es, sizeof es);
  sum[0] = Tn;
  sum[1] = On;
  memcpy(summary, sum, sizeof sum);
}

// posegraph_core.hpp — the arithmetic of misift_link_poses_batch, for host and device: which row is accepted, the depth
// ratio of one row of a link, which pair is usable, the propagation of the scales over the links and the composition of
// the cameras along the walk.  The kernels (kernels_posegraph.hip) and the host-only test hooks
// (misift_test_posegraph_ratio, _compose) compile these same functions, so what a CPU test pins is what the device runs.
// The definition, step by step, is in include/misift.h.
//
// The rules of pose_core.hpp hold: fp32 with every operation rounded, only + - * /, no fmaf, and the build's
// -ffp-contract=off.  Every three-term sum is taken left to right as the header states it.
#pragma once
#include "pose_core.hpp"

enum { POSEGRAPH_CHAIN = 0, POSEGRAPH_FAN = 1 };
constexpr int POSEGRAPH_UNSET = -2, POSEGRAPH_ROOT = -1;
// what misift_resect_cameras_batch (resect_core.hpp) puts into d_cam_pair: a camera placed by resection, not by a pair
constexpr int POSEGRAPH_RESECTED = -3;

// the rows of a pair that take part: min(max(count, 0), max_pts)
FUND_HD int posegraph_rows(int count, int max_pts)
{
  const int n = count > 0 ? count : 0;
  return n < max_pts ? n : max_pts;
}

// the edge rule of misift_link_tracks_batch on one row's fields; match_error is read only with use_error
template <class Row>
FUND_HD bool posegraph_accept(const Row &row, float min_score, float max_ambiguity, bool use_error, float max_error)
{
  bool ok = row.match >= 0 && row.score > min_score && row.ambiguity < max_ambiguity;
  if (ok && use_error) ok = row.match_error < max_error;
  return ok;
}

// The bits of rho = zq / zp for two depths in the shared camera, or 0 when the row is no sample: both depths > 0 and rho
// finite and > 0.  A positive finite float is never the bit pattern 0, and such floats order as their bits.
FUND_HD unsigned posegraph_ratio_bits(float zp, float zq)
{
  if (!(zp > 0.0f && zq > 0.0f)) return 0u;
  const float rho = zq / zp;
  if (!(rho > 0.0f && fundamental_finite(rho))) return 0u;
  unsigned u;
  __builtin_memcpy(&u, &rho, sizeof u);
  return u;
}

// Row r < np of link (p, q, kind) as a sample: the bits of its rho, or 0.  rows_* / xyz_*: row 0 of the pair, nq: the
// rows of pair q that take part.  The partner index comes from device memory and is checked before it addresses anything.
template <class Row>
FUND_HD unsigned posegraph_sample(const Row *rows_p, const float *xyz_p, const Row *rows_q, const float *xyz_q, int nq,
                                  int kind, int r, float min_score, float max_ambiguity, bool use_error,
                                  float max_error)
{
  const Row &a = rows_p[r];
  const int r2 = kind == POSEGRAPH_CHAIN ? a.match : r;
  if (!(r2 >= 0 && r2 < nq)) return 0u;
  if (!posegraph_accept(a, min_score, max_ambiguity, use_error, max_error)) return 0u;
  if (!posegraph_accept(rows_q[r2], min_score, max_ambiguity, use_error, max_error)) return 0u;
  const float a1 = xyz_p[4 * (size_t)r + 2], a2 = xyz_p[4 * (size_t)r + 3];
  const float b1 = xyz_q[4 * (size_t)r2 + 2], b2 = xyz_q[4 * (size_t)r2 + 3];
  if (!(a1 > 0.0f && a2 > 0.0f && b1 > 0.0f && b2 > 0.0f)) return 0u;
  return posegraph_ratio_bits(kind == POSEGRAPH_CHAIN ? a2 : a1, b1);
}

// a pair takes part in step 2 iff its pose won a vote and is finite
FUND_HD bool posegraph_usable(const float *pose12, int num_front)
{
  bool ok = num_front > 0;
  for (int j = 0; j < 12; j++) ok = ok && fundamental_finite(pose12[j]);
  return ok;
}

FUND_HD bool posegraph_positive(float v) { return v > 0.0f && fundamental_finite(v); }

// camera b from camera a through X_b = R X_a + s t:  R_b = R . R_a,  t_b = (R . t_a) + s t
FUND_HD void posegraph_forward(const float *pose, float s, const float *ca, float *cb)
{
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++)
      cb[3 * r + c] = pose_one_nan((pose[3 * r] * ca[c] + pose[3 * r + 1] * ca[3 + c]) + pose[3 * r + 2] * ca[6 + c]);
    const float rt = (pose[3 * r] * ca[9] + pose[3 * r + 1] * ca[10]) + pose[3 * r + 2] * ca[11];
    cb[9 + r] = pose_one_nan(rt + s * pose[9 + r]);
  }
}

// camera a from camera b:  R_a = R^T . R_b,  t_a = R^T . (t_b - s t)
FUND_HD void posegraph_backward(const float *pose, float s, const float *cb, float *ca)
{
  float d[3];
  for (int j = 0; j < 3; j++) d[j] = cb[9 + j] - s * pose[9 + j];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++)
      ca[3 * r + c] = pose_one_nan((pose[r] * cb[c] + pose[3 + r] * cb[3 + c]) + pose[6 + r] * cb[6 + c]);
    ca[9 + r] = pose_one_nan((pose[r] * d[0] + pose[3 + r] * d[1]) + pose[6 + r] * d[2]);
  }
}

// Step 2, serial.  On entry scale[] is zeros, cam[] zeros and cam_pair[] POSEGRAPH_UNSET.  links: nlinks x 3, pairs:
// npairs x 2, usable: npairs flags, all checked by the host or computed here; nothing in them is used unchecked as an
// address.  counts[0] = pairs with a scale, counts[1] = images with a camera.
FUND_HD void posegraph_solve(int npairs, const int *pairs, const int *usable, const float *pose, int nlinks,
                             const int *links, const float *ratio, int seed_pair, int root_image, int nwalk,
                             const int *walk, float *scale, float *cam, int *cam_pair, int *counts)
{
  int nscaled = 0, ncams = 1;
  if (npairs > 0 && usable[seed_pair]) {
    scale[seed_pair] = 1.0f;
    nscaled = 1;
  }
  for (int l = 0; l < nlinks; l++) {
    const int p = links[3 * l], q = links[3 * l + 1];
    const float rho = ratio[l];
    if (!(rho > 0.0f) || !usable[p] || !usable[q]) continue;
    const float sp = scale[p], sq = scale[q];
    if (sp > 0.0f && sq == 0.0f) {
      const float v = sp / rho;
      if (posegraph_positive(v)) { scale[q] = v; nscaled++; }
    } else if (sq > 0.0f && sp == 0.0f) {
      const float v = sq * rho;
      if (posegraph_positive(v)) { scale[p] = v; nscaled++; }
    }
  }
  float *root = cam + 12 * (size_t)root_image;
  root[0] = 1.0f; root[4] = 1.0f; root[8] = 1.0f;
  cam_pair[root_image] = POSEGRAPH_ROOT;
  for (int w = 0; w < nwalk; w++) {
    const int p = walk[w], a = pairs[2 * p], b = pairs[2 * p + 1];
    const float s = scale[p];
    if (!(s > 0.0f) || a == b) continue;
    const bool sa = cam_pair[a] != POSEGRAPH_UNSET, sb = cam_pair[b] != POSEGRAPH_UNSET;
    if (sa == sb) continue;
    float P[12], from[12], to[12];
    for (int j = 0; j < 12; j++) P[j] = pose[12 * (size_t)p + j];
    const int src = sa ? a : b, dst = sa ? b : a;
    for (int j = 0; j < 12; j++) from[j] = cam[12 * (size_t)src + j];
    if (sa) posegraph_forward(P, s, from, to);
    else posegraph_backward(P, s, from, to);
    for (int j = 0; j < 12; j++) cam[12 * (size_t)dst + j] = to[j];
    cam_pair[dst] = p;
    ncams++;
  }
  counts[0] = nscaled;
  counts[1] = ncams;
}

// refine_core.hpp — the arithmetic of misift_refine_cameras_batch, for host and device: the re-orthonormalised rotation,
// which candidate is a member, a member's share of the cost and of the 6x6 normal equations, the LDL^T solve, the Cayley
// update, and the whole of one image.  The kernel (kernels_refine.hip) and the host-only test hook
// (misift_test_refine_camera) compile these same functions, so what a CPU test pins is what the device runs.  The
// definition, step by step, is in include/misift.h.
//
// The rules of triangulate_core.hpp hold: fp32 with every operation rounded, only + - * / and sqrtf, no fmaf, and the
// build's -ffp-contract=off.  A sum over the members is the sum of the call of fundamental_core.hpp (256 slots, slot
// o mod 256, ascending o, then the halving tree); how the members are walked is the Exec's business: the kernel's
// workgroup scans the slot keys, the hook walks plain arrays.  An Exec has
//   pass(cam1, cam, thresh2, S, n, behind): S = the REFINE_SUMS sums under `cam` over the members under `cam1`, n = the
//   members, behind = whether a member is not in front under `cam`; the same values in every thread that runs it.
// Nothing here indexes an array with a run-time value, so everything stays in registers.
#pragma once
#include <math.h>
#include "triangulate_core.hpp"

enum { REFINE_OK = 0, REFINE_FEW_OBS = 1, REFINE_SINGULAR = 2, REFINE_HELD = 3, REFINE_NO_CAMERA = 4 };
constexpr int REFINE_SUMS = 28;                // c, the 21 entries M[r][c'] with r <= c' row-major, the 6 of g

// what the call writes for one image; as_given: d_cam_out gets the twelve input floats bit for bit, cam is not used
struct RefineResult {
  float cam[12];
  bool as_given;
  int nobs, steps, status;
  float rms0, rms1;
};

FUND_HD bool refine_finite12(const float (&c)[12])
{
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 12; j++) ok = ok && fundamental_finite(c[j]);
  return ok;
}

// step 1: Gram-Schmidt on the rows, r2 = r0 x r1; false for a non-finite result
FUND_HD bool refine_orthonormalise(float (&c)[12])
{
  float r0[3] = {c[0], c[1], c[2]}, r1[3] = {c[3], c[4], c[5]}, r2[3];
  const float n0 = sqrtf(pose_dot(r0, r0));
  r0[0] = r0[0] / n0; r0[1] = r0[1] / n0; r0[2] = r0[2] / n0;
  const float d = pose_dot(r1, r0);
  float w[3] = {r1[0] - d * r0[0], r1[1] - d * r0[1], r1[2] - d * r0[2]};
  const float n1 = sqrtf(pose_dot(w, w));
  r1[0] = w[0] / n1; r1[1] = w[1] / n1; r1[2] = w[2] / n1;
  pose_cross(r0, r1, r2);
#pragma unroll
  for (int j = 0; j < 3; j++) {
    c[j] = r0[j]; c[3 + j] = r1[j]; c[6 + j] = r2[j];
  }
  return refine_finite12(c);
}

// a candidate under a camera, as step 3 of triangulate: false when it is not in front
struct RefineView {
  float xc, yc, zc, iz, a, b, ru, rv;
};
FUND_HD bool refine_view(const float (&c)[12], const float *k, const float (&X)[3], float x, float y, RefineView &v)
{
  v.xc = ((c[0] * X[0] + c[1] * X[1]) + c[2] * X[2]) + c[9];
  v.yc = ((c[3] * X[0] + c[4] * X[1]) + c[5] * X[2]) + c[10];
  v.zc = ((c[6] * X[0] + c[7] * X[1]) + c[8] * X[2]) + c[11];
  if (!(v.zc > 0.0f)) return false;
  v.iz = 1.0f / v.zc;
  v.a = v.xc * v.iz;
  v.b = v.yc * v.iz;
  v.ru = x - (k[0] * v.a + k[2]);
  v.rv = y - (k[1] * v.b + k[3]);
  return true;
}

// step 2: the candidate is a member under the camera of step 1; thresh2 = max_error^2 rounded once, +inf: no gate
FUND_HD bool refine_member(const float (&cam1)[12], const float *k, const float (&X)[3], float x, float y, float thresh2)
{
  RefineView v;
  if (!refine_view(cam1, k, X, x, y, v)) return false;
  return thresh2 == INFINITY || v.ru * v.ru + v.rv * v.rv < thresh2;
}

// step 3: a member's 28 terms under `cam`; false when it is not in front
FUND_HD bool refine_terms(const float (&cam)[12], const float *k, const float (&X)[3], float x, float y,
                          float (&t)[REFINE_SUMS])
{
  RefineView v;
  if (!refine_view(cam, k, X, x, y, v)) return false;
  const float gx = k[0] * v.iz, gy = k[1] * v.iz;
  const float ju[6] = {gx * -(v.a * v.yc), gx * (v.zc + v.a * v.xc), gx * -v.yc, gx * 1.0f, gx * 0.0f, gx * -v.a};
  const float jv[6] = {gy * -(v.zc + v.b * v.yc), gy * (v.b * v.xc), gy * v.xc, gy * 0.0f, gy * 1.0f, gy * -v.b};
  t[0] = v.ru * v.ru + v.rv * v.rv;
  int i = 1;
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = r; c < 6; c++) t[i++] = ju[r] * ju[c] + jv[r] * jv[c];
#pragma unroll
  for (int r = 0; r < 6; r++) t[22 + r] = ju[r] * v.ru + jv[r] * v.rv;
  return true;
}

// step 4: M delta = g from the 28 sums by LDL^T without pivoting, every subtraction in ascending k; false at the first
// pivot that is not finite and > 0 or for a non-finite delta
FUND_HD bool refine_solve(const float (&S)[REFINE_SUMS], float (&delta)[6])
{
  float M[6][6], L[6][6], d[6], v[6], y[6];
  {
    int i = 1;
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
      for (int c = r; c < 6; c++) {
        M[r][c] = S[i];
        M[c][r] = S[i];
        i++;
      }
  }
#pragma unroll
  for (int j = 0; j < 6; j++) delta[j] = 0.0f;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    float dj = M[j][j];
#pragma unroll
    for (int k = 0; k < j; k++) {
      v[k] = L[j][k] * d[k];
      dj = dj - L[j][k] * v[k];
    }
    d[j] = dj;
    ok = ok && tri_pivot(dj);
    if (!ok) return false;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      float e = M[i][j];
#pragma unroll
      for (int k = 0; k < j; k++) e = e - L[i][k] * v[k];
      L[i][j] = e / dj;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    float e = S[22 + i];
#pragma unroll
    for (int k = 0; k < i; k++) e = e - L[i][k] * y[k];
    y[i] = e;
  }
  float x[6];
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    float e = y[i] / d[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) e = e - L[k][i] * x[k];
    x[i] = e;
    ok = ok && fundamental_finite(e);
  }
  if (!ok) return false;
#pragma unroll
  for (int j = 0; j < 6; j++) delta[j] = x[j];
  return true;
}

// step 5: R' = C R, t' = C t + upsilon with C the Cayley map of omega / 2
FUND_HD void refine_update(const float (&cam)[12], const float (&delta)[6], float (&out)[12])
{
  const float h[3] = {0.5f * delta[0], 0.5f * delta[1], 0.5f * delta[2]};
  const float s = pose_dot(h, h);
  const float den = 1.0f + s, e = 1.0f - s;
  const float xy = 2.0f * (h[0] * h[1]), xz = 2.0f * (h[0] * h[2]), yz = 2.0f * (h[1] * h[2]);
  const float x2 = 2.0f * h[0], y2 = 2.0f * h[1], z2 = 2.0f * h[2];
  const float C[3][3] = {{(e + 2.0f * (h[0] * h[0])) / den, (xy - z2) / den, (xz + y2) / den},
                         {(xy + z2) / den, (e + 2.0f * (h[1] * h[1])) / den, (yz - x2) / den},
                         {(xz - y2) / den, (yz + x2) / den, (e + 2.0f * (h[2] * h[2])) / den}};
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) out[3 * i + j] = (C[i][0] * cam[j] + C[i][1] * cam[3 + j]) + C[i][2] * cam[6 + j];
    out[9 + i] = ((C[i][0] * cam[9] + C[i][1] * cam[10]) + C[i][2] * cam[11]) + delta[3 + i];
  }
}

// Steps 0-7 for one image: cam_in = its twelve floats, unset = d_cam_pair says it has no camera, fixed = it is the root
// or held, k = fx fy cx cy.
template <class Exec>
FUND_HD void refine_camera(Exec &ex, const float (&cam_in)[12], bool unset, bool fixed, const float *k, int orthonormalise,
                           int min_obs, int num_loops, float thresh2, RefineResult &out)
{
  const float nan = pose_one_nan(NAN);
  out.as_given = true;
  out.nobs = 0;
  out.steps = 0;
  out.rms0 = out.rms1 = nan;
#pragma unroll
  for (int j = 0; j < 12; j++) out.cam[j] = cam_in[j];
  if (unset || !refine_finite12(cam_in)) {
    out.status = REFINE_NO_CAMERA;
    return;
  }
  if (fixed) {
    out.status = REFINE_HELD;
    return;
  }
  float cam[12];
#pragma unroll
  for (int j = 0; j < 12; j++) cam[j] = cam_in[j];
  if (orthonormalise) {
    if (!refine_orthonormalise(cam)) {
      out.status = REFINE_NO_CAMERA;
      return;
    }
    out.as_given = false;
  }
  float cam1[12];
#pragma unroll
  for (int j = 0; j < 12; j++) cam1[j] = out.cam[j] = cam[j];
  float S[REFINE_SUMS];
  int n;
  bool behind;
  ex.pass(cam1, cam, thresh2, S, n, behind);   // under the camera of step 1 no member is behind
  out.nobs = n;
  if (n < min_obs) {
    out.status = REFINE_FEW_OBS;
    return;
  }
  out.status = REFINE_OK;
  const float c0 = S[0];
  for (int loop = 0; loop < num_loops; loop++) {
    float delta[6], cam2[12], S2[REFINE_SUMS];
    if (!refine_solve(S, delta)) {
      if (loop == 0) out.status = REFINE_SINGULAR;
      break;
    }
    refine_update(cam, delta, cam2);
    int n2;
    ex.pass(cam1, cam2, thresh2, S2, n2, behind);
    if (behind || !(S2[0] < S[0])) break;
#pragma unroll
    for (int j = 0; j < 12; j++) cam[j] = cam2[j];
#pragma unroll
    for (int j = 0; j < REFINE_SUMS; j++) S[j] = S2[j];
    out.steps++;
  }
  if (out.steps > 0) {
    out.as_given = false;
#pragma unroll
    for (int j = 0; j < 12; j++) out.cam[j] = pose_one_nan(cam[j]);
  }
  out.rms0 = pose_one_nan(sqrtf(c0 / (float)n));
  out.rms1 = pose_one_nan(sqrtf(S[0] / (float)n));
}

// The host's Exec: the candidates of one image as plain arrays, slot[] ascending.
struct RefineHostExec {
  int ncand;
  const int *slot;
  const float *X, *xy, *k;
  float p[REFINE_SUMS * FUND_SLOTS];
  void pass(const float (&cam1)[12], const float (&cam)[12], float thresh2, float (&S)[REFINE_SUMS], int &n, bool &behind)
  {
    for (int i = 0; i < REFINE_SUMS * FUND_SLOTS; i++) p[i] = 0.0f;
    n = 0;
    behind = false;
    for (int i = 0; i < ncand; i++) {
      const float P[3] = {X[3 * i], X[3 * i + 1], X[3 * i + 2]};
      if (!refine_member(cam1, k, P, xy[2 * i], xy[2 * i + 1], thresh2)) continue;
      n++;
      float t[REFINE_SUMS];
      if (!refine_terms(cam, k, P, xy[2 * i], xy[2 * i + 1], t)) {
        behind = true;
        continue;
      }
      const int s = slot[i] % FUND_SLOTS;
      for (int j = 0; j < REFINE_SUMS; j++) p[j * FUND_SLOTS + s] = p[j * FUND_SLOTS + s] + t[j];
    }
    for (int off = FUND_SLOTS / 2; off > 0; off >>= 1)
      for (int t = 0; t < off; t++) fundamental_tree_step<REFINE_SUMS>(p, t, off);
    for (int j = 0; j < REFINE_SUMS; j++) S[j] = p[j * FUND_SLOTS];
  }
};

// resect_core.hpp — the arithmetic of misift_resect_cameras_batch, for host and device: the draw of six distinct sample
// positions, and the calibrated six-point solve of one RANSAC hypothesis (the world points normalised, the 11 x 12 system,
// its null vector by complete pivoting, the nearest rotation by the fixed-sweep Jacobi SVD of pose_core.hpp, the world
// normalisation undone).  The inlier test is refine_member of refine_core.hpp as it stands.  The kernels
// (kernels_resect.hip) and the host-only test hooks (misift_test_resect_samples, _solve) compile these same functions, so
// what a CPU test pins is what the device runs.  The definition, step by step, is in include/misift.h.
//
// The rules of refine_core.hpp hold: fp32 with every operation rounded, only + - * /, sqrtf and fabsf, no fmaf, and the
// build's -ffp-contract=off.  Every sum is written left to right as the header states it.  Nothing here indexes an array
// in registers with a run-time value: the system lives behind a Mat (float get(r, c), void set(r, c, v)), a plain array
// on the host and a lane's column of LDS on the device.
#pragma once
#include <math.h>
#include "libc_rand.hpp"
#include "refine_core.hpp"

enum { RESECT_OK = 0, RESECT_FEW_CAND = 1, RESECT_NO_MODEL = 2, RESECT_SKIPPED = 3, RESECT_OVER = 4 };
constexpr int RESECT_SAMPLE = 6, RESECT_ROWS = 11, RESECT_COLS = 12;

// One hypothesis' six distinct positions in the ordered list of n >= 6 candidates: six draws first, then p[1] .. p[5] in
// turn are redrawn while they repeat an earlier position (fundamental_draw8 cut to six).
template <class Ring>
LIBC_RAND_HD void resect_draw6(LibcRand<Ring> &g, const FastMod31 &fm, int (&p)[6])
{
  int p0 = (int)fm.mod((uint32_t)g.next()), p1 = (int)fm.mod((uint32_t)g.next());
  int p2 = (int)fm.mod((uint32_t)g.next()), p3 = (int)fm.mod((uint32_t)g.next());
  int p4 = (int)fm.mod((uint32_t)g.next()), p5 = (int)fm.mod((uint32_t)g.next());
  while (p1 == p0) p1 = (int)fm.mod((uint32_t)g.next());
  while (p2 == p0 || p2 == p1) p2 = (int)fm.mod((uint32_t)g.next());
  while (p3 == p0 || p3 == p1 || p3 == p2) p3 = (int)fm.mod((uint32_t)g.next());
  while (p4 == p0 || p4 == p1 || p4 == p2 || p4 == p3) p4 = (int)fm.mod((uint32_t)g.next());
  while (p5 == p0 || p5 == p1 || p5 == p2 || p5 == p3 || p5 == p4) p5 = (int)fm.mod((uint32_t)g.next());
  p[0] = p0; p[1] = p1; p[2] = p2; p[3] = p3; p[4] = p4; p[5] = p5;
}

// the host's 11 x 12 system
struct ResectArrayMat {
  float a[RESECT_ROWS][RESECT_COLS];
  FUND_HD float get(int r, int c) const { return a[r][c]; }
  FUND_HD void set(int r, int c, float v) { a[r][c] = v; }
};

// step 4a: centroid = sum in sample order / 6, d = sum in sample order of the distances to it, s = 6 sqrt(3) / d
FUND_HD void resect_normalise(const float (&X)[6], const float (&Y)[6], const float (&Z)[6], float (&c)[3], float &s)
{
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
#pragma unroll
  for (int k = 0; k < 6; k++) { sx = sx + X[k]; sy = sy + Y[k]; sz = sz + Z[k]; }
  c[0] = sx / 6.0f;
  c[1] = sy / 6.0f;
  c[2] = sz / 6.0f;
  float d = 0.0f;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const float dx = X[k] - c[0], dy = Y[k] - c[1], dz = Z[k] - c[2];
    d = d + sqrtf((dx * dx + dy * dy) + dz * dz);
  }
  s = 10.3923048f / d;
}

// step 4c: the camera from the null vector P = [M | p] (row-major 3 x 4) of the normalised system, c and s of
// resect_normalise.  False, with cam untouched, for an invalid hypothesis.
FUND_HD bool resect_camera(const float (&n)[12], const float (&c)[3], float s, float (&cam)[12])
{
  float P[12], m = 0.0f;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 12; j++) {
    const float v = fabsf(n[j]);
    ok = ok && fundamental_finite(v);
    m = v > m ? v : m;
  }
  if (!ok || m == 0.0f) return false;
#pragma unroll
  for (int j = 0; j < 12; j++) P[j] = n[j] / m;
  const float det = (P[0] * (P[5] * P[10] - P[6] * P[9]) - P[1] * (P[4] * P[10] - P[6] * P[8])) +
                    P[2] * (P[4] * P[9] - P[5] * P[8]);
  if (det == 0.0f || !fundamental_finite(det)) return false;
  if (det < 0.0f) {
#pragma unroll
    for (int j = 0; j < 12; j++) P[j] = -P[j];
  }
  float A[9], V[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int q = 0; q < 3; q++) {
      A[3 * r + q] = P[4 * r + q];
      V[3 * r + q] = r == q ? 1.0f : 0.0f;
    }
  for (int sweep = 0; sweep < POSE_SWEEPS; sweep++) {
    pose_rotate<0, 1>(A, V);
    pose_rotate<0, 2>(A, V);
    pose_rotate<1, 2>(A, V);
  }
  float sg[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    sg[j] = sqrtf(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
    ok = ok && fundamental_finite(sg[j]) && sg[j] > 0.0f;
  }
  if (!ok) return false;
  float U[9], out[12];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int j = 0; j < 3; j++) U[3 * r + j] = A[3 * r + j] / sg[j];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int q = 0; q < 3; q++)
      out[3 * r + q] = (U[3 * r] * V[3 * q] + U[3 * r + 1] * V[3 * q + 1]) + U[3 * r + 2] * V[3 * q + 2];
  const float lambda = ((sg[0] + sg[1]) + sg[2]) / 3.0f;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const float tn = P[4 * r + 3] / lambda;
    out[9 + r] = tn / s - ((out[3 * r] * c[0] + out[3 * r + 1] * c[1]) + out[3 * r + 2] * c[2]);
  }
  if (!refine_finite12(out)) return false;
#pragma unroll
  for (int j = 0; j < 12; j++) cam[j] = out[j];
  return true;
}

// Step 4 for one sample: (x, y) the observations, (X, Y, Z) the world points, k = fx fy cx cy.  Returns whether the
// hypothesis is valid; an invalid one (a zero or non-finite pivot, a zero or non-finite determinant, a non-finite entry)
// gets twelve zeros, which no candidate fits.
template <class Mat>
FUND_HD bool resect_solve6(Mat &m, const float (&x)[6], const float (&y)[6], const float (&X)[6], const float (&Y)[6],
                           const float (&Z)[6], const float *k, float (&cam)[12])
{
  float c[3], s;
  resect_normalise(X, Y, Z, c, s);
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const float a = (X[i] - c[0]) * s, b = (Y[i] - c[1]) * s, w = (Z[i] - c[2]) * s;
    const float u = (x[i] - k[2]) / k[0], v = (y[i] - k[3]) / k[1];
    const float ru[12] = {a, b, w, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, -(u * a), -(u * b), -(u * w), -u};
#pragma unroll
    for (int j = 0; j < 12; j++) m.set(2 * i, j, ru[j]);
    if (i < 5) {
      const float rv[12] = {0.0f, 0.0f, 0.0f, 0.0f, a, b, w, 1.0f, -(v * a), -(v * b), -(v * w), -v};
#pragma unroll
      for (int j = 0; j < 12; j++) m.set(2 * i + 1, j, rv[j]);
    }
  }
  float n[12];
  bool ok = fundamental_eliminate<RESECT_ROWS>(m, n);
#pragma unroll
  for (int j = 0; j < 12; j++) cam[j] = 0.0f;
  ok = ok && resect_camera(n, c, s, cam);
  if (!ok) {
#pragma unroll
    for (int j = 0; j < 12; j++) cam[j] = 0.0f;
  }
  return ok;
}

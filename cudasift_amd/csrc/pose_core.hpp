// pose_core.hpp — the arithmetic of misift_recover_pose_batch, for host and device: E = K2^T F K1, its one-sided Jacobi
// SVD in a fixed number of sweeps, the four (R, t) hypotheses, and the depth terms of one match under one hypothesis.  The
// kernel (kernels_pose.hip) and the host-only test hooks (misift_test_pose_decompose, _vote) compile these same functions,
// so what a CPU test pins is what the device runs.  The definition, step by step, is in include/misift.h.
//
// The rules of fundamental_core.hpp hold: fp32 with every operation rounded, only + - * /, sqrtf and fabsf, no fmaf, and
// the build's -ffp-contract=off.  Every sum of products is written left to right as the header states it.  Nothing here
// indexes an array with a run-time value: columns are chosen with selects, so everything stays in registers.
#pragma once
#include <math.h>
#include "fundamental_core.hpp"

constexpr int POSE_SWEEPS = 6;

// K8 = fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2
struct PoseIntrinsics {
  float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
};

// what the four hypotheses share: k < 2 takes Ra, otherwise Rb; even k takes t, odd k takes -t
struct PoseHypotheses {
  float Ra[9], Rb[9], t[3];
};

FUND_HD void pose_cross(const float (&a)[3], const float (&b)[3], float (&c)[3])
{
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

FUND_HD float pose_dot(const float (&a)[3], const float (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// step 1: A = E / max |E| with E = K2^T F K1; false for a non-finite entry of E or E = 0
FUND_HD bool pose_essential(const float (&F)[9], const PoseIntrinsics &K, float (&A)[9])
{
  float G[9];                                  // F . K1
#pragma unroll
  for (int r = 0; r < 3; r++) {
    G[3 * r + 0] = F[3 * r + 0] * K.fx1;
    G[3 * r + 1] = F[3 * r + 1] * K.fy1;
    G[3 * r + 2] = (F[3 * r + 0] * K.cx1 + F[3 * r + 1] * K.cy1) + F[3 * r + 2];
  }
  float m = 0.0f;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; c++) {                // K2^T . (F . K1)
    A[0 + c] = K.fx2 * G[0 + c];
    A[3 + c] = K.fy2 * G[3 + c];
    A[6 + c] = (K.cx2 * G[0 + c] + K.cy2 * G[3 + c]) + G[6 + c];
  }
#pragma unroll
  for (int j = 0; j < 9; j++) {
    const float v = fabsf(A[j]);
    ok = ok && fundamental_finite(v);
    m = v > m ? v : m;
  }
  if (!ok || m == 0.0f) return false;
#pragma unroll
  for (int j = 0; j < 9; j++) A[j] = A[j] / m;
  return true;
}

// step 2, one column pair (P, Q) of A and V alike
template <int P, int Q>
FUND_HD void pose_rotate(float (&A)[9], float (&V)[9])
{
  const float alpha = A[P] * A[P] + A[3 + P] * A[3 + P] + A[6 + P] * A[6 + P];
  const float beta = A[Q] * A[Q] + A[3 + Q] * A[3 + Q] + A[6 + Q] * A[6 + Q];
  const float gamma = A[P] * A[Q] + A[3 + P] * A[3 + Q] + A[6 + P] * A[6 + Q];
  if (gamma == 0.0f) return;
  const float zeta = (beta - alpha) / (2.0f * gamma);
  float tau = 1.0f / (fabsf(zeta) + sqrtf(1.0f + zeta * zeta));
  if (zeta < 0.0f) tau = -tau;
  const float c = 1.0f / sqrtf(1.0f + tau * tau), s = c * tau;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const float ap = A[3 * r + P], aq = A[3 * r + Q], vp = V[3 * r + P], vq = V[3 * r + Q];
    A[3 * r + P] = c * ap - s * aq;
    A[3 * r + Q] = s * ap + c * aq;
    V[3 * r + P] = c * vp - s * vq;
    V[3 * r + Q] = s * vp + c * vq;
  }
}

// column i of a row-major 3x3, i chosen with selects between values read beforehand: a conditional read would leave the
// matrix in scratch memory
FUND_HD void pose_column(const float (&M)[9], int i, float (&v)[3])
{
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const float m0 = M[3 * r], m1 = M[3 * r + 1], m2 = M[3 * r + 2];
    v[r] = i == 0 ? m0 : (i == 1 ? m1 : m2);
  }
}

// steps 1-4: the hypotheses of F under K; an invalid entry returns false and zeros
FUND_HD bool pose_decompose(const float (&F)[9], const PoseIntrinsics &K, PoseHypotheses &h)
{
#pragma unroll
  for (int j = 0; j < 9; j++) { h.Ra[j] = 0.0f; h.Rb[j] = 0.0f; }
#pragma unroll
  for (int j = 0; j < 3; j++) h.t[j] = 0.0f;
  float A[9], V[9];
  if (!pose_essential(F, K, A)) return false;
#pragma unroll
  for (int j = 0; j < 9; j++) V[j] = (j == 0 || j == 4 || j == 8) ? 1.0f : 0.0f;
  for (int sweep = 0; sweep < POSE_SWEEPS; sweep++) {
    pose_rotate<0, 1>(A, V);
    pose_rotate<0, 2>(A, V);
    pose_rotate<1, 2>(A, V);
  }
  float w[3];
#pragma unroll
  for (int j = 0; j < 3; j++) w[j] = A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j];
  int i1 = 0;                                  // the largest, the first maximum wins
  if (w[1] > w[0]) i1 = 1;
  if (w[2] > (i1 == 0 ? w[0] : w[1])) i1 = 2;
  const int ja = i1 == 0 ? 1 : 0, jb = i1 == 2 ? 1 : 2;          // the other two, in index order
  const float wa = ja == 0 ? w[0] : w[1], wb = jb == 1 ? w[1] : w[2];
  const int i2 = wb > wa ? jb : ja;
  const float w1 = i1 == 0 ? w[0] : (i1 == 1 ? w[1] : w[2]), w2 = wb > wa ? wb : wa;
  if (!(w2 > 0.0f)) return false;
  float u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
  pose_column(A, i1, u1);
  pose_column(A, i2, u2);
  pose_column(V, i1, v1);
  pose_column(V, i2, v2);
  const float n1 = sqrtf(w1), n2 = sqrtf(w2);
#pragma unroll
  for (int r = 0; r < 3; r++) { u1[r] = u1[r] / n1; u2[r] = u2[r] / n2; }
  pose_cross(u1, u2, u3);
  pose_cross(v1, v2, v3);
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      h.Ra[3 * r + c] = (u2[r] * v1[c] - u1[r] * v2[c]) + u3[r] * v3[c];
      h.Rb[3 * r + c] = (u1[r] * v2[c] - u2[r] * v1[c]) + u3[r] * v3[c];
    }
    h.t[r] = u3[r];
  }
  return true;
}

// hypothesis k as R (row-major) and t, 12 floats
FUND_HD void pose_hypothesis(const PoseHypotheses &h, int k, float (&pose)[12])
{
#pragma unroll
  for (int j = 0; j < 9; j++) pose[j] = k < 2 ? h.Ra[j] : h.Rb[j];
#pragma unroll
  for (int j = 0; j < 3; j++) pose[9 + j] = (k & 1) ? -h.t[j] : h.t[j];
}

// step 5: a record in normalised coordinates, p = ((x - cx) / fx, (y - cy) / fy, 1) in each image
FUND_HD void pose_normalised(const PoseIntrinsics &K, float x1, float y1, float x2, float y2, float (&p1)[3],
                             float (&p2)[3])
{
  p1[0] = (x1 - K.cx1) / K.fx1; p1[1] = (y1 - K.cy1) / K.fy1; p1[2] = 1.0f;
  p2[0] = (x2 - K.cx2) / K.fx2; p2[1] = (y2 - K.cy2) / K.fy2; p2[2] = 1.0f;
}

// step 5: den, n1 and n2 of a record under X2 = R X1 + t; the depths are n1 / den in camera 1 and n2 / den in camera 2.
// Under -t, den is the same and n1 and n2 change sign and nothing else: every product and every rounded sum does.
FUND_HD void pose_depth_terms(const float (&R)[9], const float (&t)[3], const float (&p1)[3], const float (&p2)[3],
                              float &den, float &n1, float &n2)
{
  float a[3], n[3], p2t[3], at[3];
#pragma unroll
  for (int r = 0; r < 3; r++) a[r] = R[3 * r] * p1[0] + R[3 * r + 1] * p1[1] + R[3 * r + 2] * p1[2];
  pose_cross(a, p2, n);
  pose_cross(p2, t, p2t);
  pose_cross(a, t, at);
  den = pose_dot(n, n);
  n1 = pose_dot(p2t, n);
  n2 = pose_dot(at, n);
}

// in front of both cameras (a comparison with a NaN is false)
FUND_HD bool pose_in_front(float den, float n1, float n2) { return den > 0.0f && n1 > 0.0f && n2 > 0.0f; }

// a NaN becomes the one quiet NaN 0x7fc00000 (see fundamental_error: a computed NaN's sign and payload are the
// processor's choice); on the bits, so that no float select is folded away
FUND_HD float pose_one_nan(float v)
{
  unsigned u;
  __builtin_memcpy(&u, &v, sizeof u);
  if ((u & 0x7fffffffu) > 0x7f800000u) u = 0x7fc00000u;
  __builtin_memcpy(&v, &u, sizeof u);
  return v;
}

// step 7: (z1 p1x, z1 p1y, z1, z2) of a record; four quiet NaNs where den > 0 is false, or for an invalid entry
FUND_HD void pose_xyz(bool valid, float den, float n1, float n2, const float (&p1)[3], float (&out)[4])
{
  if (!valid || !(den > 0.0f)) {
#pragma unroll
    for (int j = 0; j < 4; j++) out[j] = pose_one_nan(NAN);
    return;
  }
  const float z1 = n1 / den, z2 = n2 / den;
  out[0] = pose_one_nan(z1 * p1[0]);
  out[1] = pose_one_nan(z1 * p1[1]);
  out[2] = pose_one_nan(z1);
  out[3] = pose_one_nan(z2);
}

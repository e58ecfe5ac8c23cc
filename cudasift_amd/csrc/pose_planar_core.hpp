// pose_planar_core.hpp — the arithmetic of misift_recover_pose_planar_batch, for host and device: the inlier test of one
// stored match under a homography, the decision between the homography and the fundamental matrix, A = K2^-1 H K1 and
// its sign, the one-sided Jacobi of pose_core.hpp on it, the rotation of a rotation-only pair, the two (R, t, N, d) of a
// plane-induced homography (Ma, Soatto, Kosecka, Sastry, An Invitation to 3-D Vision, Theorem 5.19) with their
// fundamental matrices, and the pick among the four hypotheses.  The kernel (kernels_pose_planar.hip) and the host-only
// test hooks (misift_test_pose_planar_decompose, _vote) compile these same functions, so what a CPU test pins is what
// the device runs.  The definition, step by step, is in include/misift.h.
//
// The rules of fundamental_core.hpp hold: fp32 with every operation rounded, only + - * /, sqrtf and fabsf, no fmaf, and
// the build's -ffp-contract=off.  Every sum of products is associated as the header states it.  Nothing here indexes an
// array with a run-time value: columns are chosen with selects (pose_column), so everything stays in registers.
#pragma once
#include <math.h>
#include "fundamental_core.hpp"
#include "pose_core.hpp"

constexpr int PLANAR_INVALID = -1, PLANAR_GENERAL = 0, PLANAR_PLANE = 1, PLANAR_ROTATION = 2;

// what the four hypotheses share: k < 2 takes (Ra, ta, Na, da), otherwise (Rb, tb, Nb, db); odd k negates t and N.  Fa and
// Fb are the fundamental matrices of k = 0 and k = 2.  A rotation-only entry has Ra = Rb = R and zeros elsewhere.
struct PlanarHypotheses {
  float Ra[9], Rb[9], ta[3], tb[3], Na[3], Nb[3], da, db, Fa[9], Fb[9], s1, s3;
};
constexpr int PLANAR_HYP_FLOATS = 9 + 9 + 3 + 3 + 3 + 3 + 1 + 1 + 9 + 9 + 1 + 1;

// the hypotheses as PLANAR_HYP_FLOATS floats in the order of the struct and back, indexed statically: how the kernel
// hands them from one thread to the others
FUND_HD void planar_pack(const PlanarHypotheses &h, float (&a)[PLANAR_HYP_FLOATS])
{
#pragma unroll
  for (int j = 0; j < 9; j++) { a[j] = h.Ra[j]; a[9 + j] = h.Rb[j]; a[32 + j] = h.Fa[j]; a[41 + j] = h.Fb[j]; }
#pragma unroll
  for (int j = 0; j < 3; j++) { a[18 + j] = h.ta[j]; a[21 + j] = h.tb[j]; a[24 + j] = h.Na[j]; a[27 + j] = h.Nb[j]; }
  a[30] = h.da; a[31] = h.db; a[50] = h.s1; a[51] = h.s3;
}

FUND_HD void planar_unpack(const float (&a)[PLANAR_HYP_FLOATS], PlanarHypotheses &h)
{
#pragma unroll
  for (int j = 0; j < 9; j++) { h.Ra[j] = a[j]; h.Rb[j] = a[9 + j]; h.Fa[j] = a[32 + j]; h.Fb[j] = a[41 + j]; }
#pragma unroll
  for (int j = 0; j < 3; j++) { h.ta[j] = a[18 + j]; h.tb[j] = a[21 + j]; h.Na[j] = a[24 + j]; h.Nb[j] = a[27 + j]; }
  h.da = a[30]; h.db = a[31]; h.s1 = a[50]; h.s3 = a[51];
}

// M . v, each row ((m0 v0 + m1 v1) + m2 v2)
FUND_HD void planar_apply(const float (&M)[9], const float (&v)[3], float (&out)[3])
{
#pragma unroll
  for (int r = 0; r < 3; r++) out[r] = M[3 * r] * v[0] + M[3 * r + 1] * v[1] + M[3 * r + 2] * v[2];
}

// step 1: a match is an H-inlier iff errx^2 + erry^2 < thresh^2 * deno^2 (a comparison with a NaN is false); plain
// rounded products, all nine entries as given
FUND_HD bool planar_h_inlier(const float (&H)[9], float x1, float y1, float x2, float y2, float thresh2)
{
  const float deno = (H[6] * x1 + H[7] * y1) + H[8];
  const float nomx = (H[0] * x1 + H[1] * y1) + H[2];
  const float nomy = (H[3] * x1 + H[4] * y1) + H[5];
  const float errx = x2 * deno - nomx, erry = y2 * deno - nomy;
  return errx * errx + erry * erry < thresh2 * (deno * deno);
}

// step 2: whether the entry goes on to the decomposition
FUND_HD bool planar_candidate(int nH, int nF, bool has_f, int min_inliers, float planar_ratio)
{
  if (nH < min_inliers) return false;
  if (has_f && !((float)nH >= planar_ratio * (float)nF)) return false;
  return true;
}

FUND_HD float planar_det(const float (&A)[9])
{
  return (A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6])) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}

// step 3: A = K2^-1 H K1 over its largest fabsf, negated where its determinant is negative; false for a non-finite entry,
// A = 0, or a determinant that is not > 0 afterwards
FUND_HD bool planar_normalise(const float (&H)[9], const PoseIntrinsics &K, float (&A)[9])
{
  float G[9];                                  // H . K1
#pragma unroll
  for (int r = 0; r < 3; r++) {
    G[3 * r + 0] = H[3 * r + 0] * K.fx1;
    G[3 * r + 1] = H[3 * r + 1] * K.fy1;
    G[3 * r + 2] = (H[3 * r + 0] * K.cx1 + H[3 * r + 1] * K.cy1) + H[3 * r + 2];
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {                // K2^-1 . (H . K1)
    A[0 + c] = (G[0 + c] - K.cx2 * G[6 + c]) / K.fx2;
    A[3 + c] = (G[3 + c] - K.cy2 * G[6 + c]) / K.fy2;
    A[6 + c] = G[6 + c];
  }
  float m = 0.0f;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 9; j++) {
    const float v = fabsf(A[j]);
    ok = ok && fundamental_finite(v);
    m = v > m ? v : m;
  }
  if (!ok || m == 0.0f) return false;
#pragma unroll
  for (int j = 0; j < 9; j++) A[j] = A[j] / m;
  float det = planar_det(A);
  if (det < 0.0f) {
#pragma unroll
    for (int j = 0; j < 9; j++) A[j] = -A[j];
    det = planar_det(A);
  }
  return det > 0.0f;
}

// step 7: F = K2^-T . [t]x . R . K1^-1, the inverse intrinsics as divisions
FUND_HD void planar_fundamental(const float (&R)[9], const float (&t)[3], const PoseIntrinsics &K, float (&F)[9])
{
  float E[9], G[9];
#pragma unroll
  for (int c = 0; c < 3; c++) {                // [t]x . R
    E[0 + c] = t[1] * R[6 + c] - t[2] * R[3 + c];
    E[3 + c] = t[2] * R[0 + c] - t[0] * R[6 + c];
    E[6 + c] = t[0] * R[3 + c] - t[1] * R[0 + c];
  }
#pragma unroll
  for (int r = 0; r < 3; r++) {                // E . K1^-1
    G[3 * r + 0] = E[3 * r + 0] / K.fx1;
    G[3 * r + 1] = E[3 * r + 1] / K.fy1;
    G[3 * r + 2] = (E[3 * r + 2] - G[3 * r + 0] * K.cx1) - G[3 * r + 1] * K.cy1;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {                // K2^-T . (E . K1^-1)
    F[0 + c] = G[0 + c] / K.fx2;
    F[3 + c] = G[3 + c] / K.fy2;
    F[6 + c] = (G[6 + c] - K.cx2 * F[0 + c]) - K.cy2 * F[3 + c];
  }
}

// step 6 for one u: R, t = T / |T|, N and d = 1 / |T|; false where |T| is not finite and > 0
FUND_HD bool planar_solution(const float (&Hn)[9], const float (&v2)[3], const float (&u)[3], float (&R)[9],
                             float (&t)[3], float (&N)[3], float &d)
{
  float p[3], q[3], s[3], T[3];
  pose_cross(v2, u, N);
  planar_apply(Hn, v2, p);
  planar_apply(Hn, u, q);
  pose_cross(p, q, s);
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) R[3 * r + c] = (p[r] * v2[c] + q[r] * u[c]) + s[r] * N[c];
#pragma unroll
  for (int r = 0; r < 3; r++)
    T[r] = ((Hn[3 * r] - R[3 * r]) * N[0] + (Hn[3 * r + 1] - R[3 * r + 1]) * N[1]) +
           (Hn[3 * r + 2] - R[3 * r + 2]) * N[2];
  const float nT = sqrtf(pose_dot(T, T));
  if (!(fundamental_finite(nT) && nT > 0.0f)) return false;
#pragma unroll
  for (int r = 0; r < 3; r++) t[r] = T[r] / nT;
  d = 1.0f / nT;
  return true;
}

// steps 3-6 and the two F of step 7: PLANAR_INVALID (h is zeros), PLANAR_PLANE or PLANAR_ROTATION
FUND_HD int planar_decompose(const float (&H)[9], const PoseIntrinsics &K, float min_baseline, PlanarHypotheses &h)
{
#pragma unroll
  for (int j = 0; j < 9; j++) { h.Ra[j] = 0.0f; h.Rb[j] = 0.0f; h.Fa[j] = 0.0f; h.Fb[j] = 0.0f; }
#pragma unroll
  for (int j = 0; j < 3; j++) { h.ta[j] = 0.0f; h.tb[j] = 0.0f; h.Na[j] = 0.0f; h.Nb[j] = 0.0f; }
  h.da = 0.0f; h.db = 0.0f; h.s1 = 0.0f; h.s3 = 0.0f;
  float A[9], B[9], V[9];
  if (!planar_normalise(H, K, A)) return PLANAR_INVALID;
#pragma unroll
  for (int j = 0; j < 9; j++) { B[j] = A[j]; V[j] = (j == 0 || j == 4 || j == 8) ? 1.0f : 0.0f; }
  for (int sweep = 0; sweep < POSE_SWEEPS; sweep++) {
    pose_rotate<0, 1>(B, V);
    pose_rotate<0, 2>(B, V);
    pose_rotate<1, 2>(B, V);
  }
  float w[3];
#pragma unroll
  for (int j = 0; j < 3; j++) w[j] = B[j] * B[j] + B[3 + j] * B[3 + j] + B[6 + j] * B[6 + j];
  int hi = 0;                                  // the largest, the first maximum wins
  if (w[1] > w[0]) hi = 1;
  if (w[2] > (hi == 0 ? w[0] : w[1])) hi = 2;
  const int ja = hi == 0 ? 1 : 0, jb = hi == 2 ? 1 : 2;          // the other two, in index order
  const float wa = ja == 0 ? w[0] : w[1], wb = jb == 1 ? w[1] : w[2];
  const int mid = wb > wa ? jb : ja, lo = wb > wa ? ja : jb;
  const float whi = hi == 0 ? w[0] : (hi == 1 ? w[1] : w[2]), wmid = wb > wa ? wb : wa, wlo = wb > wa ? wa : wb;
  if (!(wlo > 0.0f)) return PLANAR_INVALID;
  const float s1 = whi / wmid, s3 = wlo / wmid;
  const float b = sqrtf(s1) - sqrtf(s3);
  if (!(b > min_baseline)) {                   // step 5: R = sum_j (B.j / |B.j|) V.j^T
    const float n0 = sqrtf(w[0]), n1 = sqrtf(w[1]), n2 = sqrtf(w[2]);
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const float u0 = B[3 * r] / n0, u1 = B[3 * r + 1] / n1, u2 = B[3 * r + 2] / n2;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        h.Ra[3 * r + c] = (u0 * V[3 * c] + u1 * V[3 * c + 1]) + u2 * V[3 * c + 2];
        h.Rb[3 * r + c] = h.Ra[3 * r + c];
      }
    }
    h.s1 = s1; h.s3 = s3;
    return PLANAR_ROTATION;
  }
  float Hn[9], v1[3], v2[3], v3[3], ua[3], ub[3];
  const float nm = sqrtf(wmid);
#pragma unroll
  for (int j = 0; j < 9; j++) Hn[j] = A[j] / nm;
  pose_column(V, hi, v1);
  pose_column(V, mid, v2);
  pose_column(V, lo, v3);
  const float a = sqrtf(1.0f - s3), c = sqrtf(s1 - 1.0f), dd = sqrtf(s1 - s3);
#pragma unroll
  for (int r = 0; r < 3; r++) {
    ua[r] = (a * v1[r] + c * v3[r]) / dd;
    ub[r] = (a * v1[r] - c * v3[r]) / dd;
  }
  PlanarHypotheses g;
  const bool oka = planar_solution(Hn, v2, ua, g.Ra, g.ta, g.Na, g.da);
  const bool okb = planar_solution(Hn, v2, ub, g.Rb, g.tb, g.Nb, g.db);
  if (!(oka && okb)) return PLANAR_INVALID;
  planar_fundamental(g.Ra, g.ta, K, g.Fa);
  planar_fundamental(g.Rb, g.tb, K, g.Fb);
  g.s1 = s1; g.s3 = s3;
  h = g;
  return PLANAR_PLANE;
}

// hypothesis k as R (row-major) and t, 12 floats, and its plane (N, d), 4 floats
FUND_HD void planar_hypothesis(const PlanarHypotheses &h, int k, float (&pose)[12], float (&plane)[4])
{
#pragma unroll
  for (int j = 0; j < 9; j++) pose[j] = k < 2 ? h.Ra[j] : h.Rb[j];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float t = k < 2 ? h.ta[j] : h.tb[j], n = k < 2 ? h.Na[j] : h.Nb[j];
    pose[9 + j] = (k & 1) ? -t : t;
    plane[j] = (k & 1) ? -n : n;
  }
  plane[3] = k < 2 ? h.da : h.db;
}

// step 7 for one record that passes the gate: whether it counts for each of the four hypotheses
FUND_HD void planar_record_votes(const PlanarHypotheses &h, const PoseIntrinsics &K, float x1, float y1, float x2,
                                 float y2, float thresh2, bool (&v)[4])
{
  float p1[3], p2[3], den, n1, n2, sden;
  pose_normalised(K, x1, y1, x2, y2, p1, p2);
  float e2 = fundamental_sampson(h.Fa, x1, y1, x2, y2, sden);
  const bool ina = fundamental_inlier(e2, sden, thresh2);
  pose_depth_terms(h.Ra, h.ta, p1, p2, den, n1, n2);
  v[0] = ina && pose_in_front(den, n1, n2);
  v[1] = ina && pose_in_front(den, -n1, -n2);
  e2 = fundamental_sampson(h.Fb, x1, y1, x2, y2, sden);
  const bool inb = fundamental_inlier(e2, sden, thresh2);
  pose_depth_terms(h.Rb, h.tb, p1, p2, den, n1, n2);
  v[2] = inb && pose_in_front(den, n1, n2);
  v[3] = inb && pose_in_front(den, -n1, -n2);
}

// step 7: the largest vote at the smallest k, and the better-voted hypothesis of the other rotation (the smaller k on a
// tie)
FUND_HD void planar_pick(const int (&votes)[4], int &best, int &alt)
{
  best = 0;
#pragma unroll
  for (int k = 1; k < 4; k++) {
    const int vb = best == 0 ? votes[0] : (best == 1 ? votes[1] : votes[2]);
    best = votes[k] > vb ? k : best;
  }
  alt = best < 2 ? (votes[3] > votes[2] ? 3 : 2) : (votes[1] > votes[0] ? 1 : 0);
}

// ---- the bodies of the host-only test hooks (the extern "C" wrappers are in kernels_pose_planar.hip)

// model, and out84 = s1, s3, then for k = 0..3 the pose (12) and the plane (4), then Fa and Fb; zeros for an invalid entry
inline int planar_hook_decompose(const float *H9, const float *K8, float min_baseline, float *out, int *model)
{
  float H[9];
  for (int k = 0; k < 9; k++) H[k] = H9[k];
  const PoseIntrinsics K{K8[0], K8[1], K8[2], K8[3], K8[4], K8[5], K8[6], K8[7]};
  PlanarHypotheses h;
  *model = planar_decompose(H, K, min_baseline, h);
  out[0] = h.s1;
  out[1] = h.s3;
  for (int k = 0; k < 4; k++) {
    float pose[12], plane[4];
    planar_hypothesis(h, k, pose, plane);
    const bool rot = *model != PLANAR_PLANE;                     // t = 0 and no plane: no signed zeros
    for (int j = 0; j < 12; j++) out[2 + 16 * k + j] = rot && j >= 9 ? 0.0f : pose[j];
    for (int j = 0; j < 4; j++) out[2 + 16 * k + 12 + j] = rot ? 0.0f : plane[j];
  }
  for (int j = 0; j < 9; j++) { out[66 + j] = h.Fa[j]; out[75 + j] = h.Fb[j]; }
  return 0;
}

// per record: whether it is an H-inlier, an F-inlier (0 without F9) and counts for each hypothesis of out84; `gate` is
// the record's gate.  decision9 = nH, nF, whether step 2 lets the entry go on, the four votes, the pick, the alternative
inline int planar_hook_vote(const float *H9, const float *F9, const float *hyp84, const float *K8, const float *xy,
                            const unsigned char *gate, int n, float thresh_h, float thresh_f, float planar_ratio,
                            int min_inliers, unsigned char *h_in, unsigned char *f_in, unsigned char *votes,
                            int *decision9)
{
  float H[9], F[9];
  for (int k = 0; k < 9; k++) { H[k] = H9[k]; F[k] = F9 ? F9[k] : 0.0f; }
  const PoseIntrinsics K{K8[0], K8[1], K8[2], K8[3], K8[4], K8[5], K8[6], K8[7]};
  PlanarHypotheses h;
  for (int j = 0; j < 9; j++) {
    h.Ra[j] = hyp84[2 + j]; h.Rb[j] = hyp84[2 + 32 + j];
    h.Fa[j] = hyp84[66 + j]; h.Fb[j] = hyp84[75 + j];
  }
  for (int j = 0; j < 3; j++) {
    h.ta[j] = hyp84[2 + 9 + j]; h.tb[j] = hyp84[2 + 32 + 9 + j];
    h.Na[j] = hyp84[2 + 12 + j]; h.Nb[j] = hyp84[2 + 32 + 12 + j];
  }
  h.da = hyp84[2 + 15]; h.db = hyp84[2 + 32 + 15];
  h.s1 = hyp84[0]; h.s3 = hyp84[1];
  const float th2 = thresh_h * thresh_h, tf2 = thresh_f * thresh_f;
  int nH = 0, nF = 0, sum[4] = {0, 0, 0, 0};
  for (int i = 0; i < n; i++) {
    const float x1 = xy[4 * i], y1 = xy[4 * i + 1], x2 = xy[4 * i + 2], y2 = xy[4 * i + 3];
    const bool g = gate[i] != 0;
    h_in[i] = g && planar_h_inlier(H, x1, y1, x2, y2, th2) ? 1 : 0;
    float den;
    const float e2 = fundamental_sampson(F, x1, y1, x2, y2, den);
    f_in[i] = g && F9 && fundamental_inlier(e2, den, tf2) ? 1 : 0;
    bool v[4];
    planar_record_votes(h, K, x1, y1, x2, y2, tf2, v);
    for (int k = 0; k < 4; k++) {
      votes[4 * i + k] = g && v[k] ? 1 : 0;
      sum[k] += votes[4 * i + k];
    }
    nH += h_in[i];
    nF += f_in[i];
  }
  int best, alt;
  planar_pick(sum, best, alt);
  decision9[0] = nH;
  decision9[1] = nF;
  decision9[2] = planar_candidate(nH, nF, F9 != nullptr, min_inliers, planar_ratio) ? 1 : 0;
  for (int k = 0; k < 4; k++) decision9[3 + k] = sum[k];
  decision9[7] = best;
  decision9[8] = alt;
  return 0;
}

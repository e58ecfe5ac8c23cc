// align_core.hpp — the arithmetic of misift_align_points_batch and misift_transform_scene_batch, for host and device: the
// draw of three distinct sample positions, Horn's closed-form similarity transform (scale s, rotation R, translation t with
// b = s R a + t) from three correspondences or from the sums over a member set, the member test, the refits over the
// members, and a camera moved into the transformed frame.  The kernels (kernels_align.hip) and the host-only test hooks
// (misift_test_align_samples, _solve, _refit, misift_test_transform_camera) compile these same functions, so what a CPU
// test pins is what the device runs.  The definition, step by step, is in include/misift.h.
//
// The rules of refine_core.hpp hold: fp32 with every operation rounded, only + - * /, sqrtf and fabsf, no fmaf, and the
// build's -ffp-contract=off.  Every sum is written left to right as the header states it.  Nothing here indexes an array
// in registers with a run-time value: the columns of the SVD are chosen with selects (pose_column).
#pragma once
#include <math.h>
#include "libc_rand.hpp"
#include "pose_core.hpp"

enum { ALIGN_OK = 0, ALIGN_FEW_CAND = 1, ALIGN_NO_MODEL = 2 };
constexpr int ALIGN_SAMPLE = 3, ALIGN_PARAMS = 13;     // R row-major, t, s
constexpr int ALIGN_CENTROID_SUMS = 6, ALIGN_MOMENT_SUMS = 11;
// sigma2 / sigma1 <= 1e-5 (about 84 float32 eps): a second singular value the roundings of M / m alone can produce, so
// the set is collinear as far as float32 can tell
constexpr float ALIGN_MIN_W_RATIO = 1e-10f;

// One hypothesis' three distinct positions in the ordered list of n >= 3 candidates: three draws first, then p[1] and p[2]
// in turn are redrawn while they repeat an earlier position (fundamental_draw8 cut to three).
template <class Ring>
LIBC_RAND_HD void align_draw3(LibcRand<Ring> &g, const FastMod31 &fm, int (&p)[3])
{
  int p0 = (int)fm.mod((uint32_t)g.next()), p1 = (int)fm.mod((uint32_t)g.next());
  int p2 = (int)fm.mod((uint32_t)g.next());
  while (p1 == p0) p1 = (int)fm.mod((uint32_t)g.next());
  while (p2 == p0 || p2 == p1) p2 = (int)fm.mod((uint32_t)g.next());
  p[0] = p0; p[1] = p1; p[2] = p2;
}

// thirteen copies of the one quiet NaN: the INVALID hypothesis, which no candidate fits
FUND_HD void align_invalid(float (&h)[ALIGN_PARAMS])
{
#pragma unroll
  for (int j = 0; j < ALIGN_PARAMS; j++) h[j] = pose_one_nan(NAN);
}

// Step 3 behind the sums: the transform from the moments M[3r + c] = sum db[r] da[c], the spreads sa and sb and the
// centroids ca and cb.  Returns whether it is valid; an invalid one is thirteen quiet NaNs.
FUND_HD bool align_from_moments(const float (&M)[9], float sa, float sb, const float (&ca)[3], const float (&cb)[3],
                                float (&h)[ALIGN_PARAMS])
{
  align_invalid(h);
  float m = 0.0f;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 9; j++) {
    const float v = fabsf(M[j]);
    ok = ok && fundamental_finite(v);
    m = v > m ? v : m;
  }
  if (!ok || m == 0.0f) return false;
  float A[9], V[9];
#pragma unroll
  for (int j = 0; j < 9; j++) {
    A[j] = M[j] / m;
    V[j] = (j == 0 || j == 4 || j == 8) ? 1.0f : 0.0f;
  }
  for (int sweep = 0; sweep < POSE_SWEEPS; sweep++) {
    pose_rotate<0, 1>(A, V);
    pose_rotate<0, 2>(A, V);
    pose_rotate<1, 2>(A, V);
  }
  float w[3];
#pragma unroll
  for (int j = 0; j < 3; j++) w[j] = A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j];
  int i1 = 0;                                  // the largest, the first maximum wins (as pose_decompose)
  if (w[1] > w[0]) i1 = 1;
  if (w[2] > (i1 == 0 ? w[0] : w[1])) i1 = 2;
  const int ja = i1 == 0 ? 1 : 0, jb = i1 == 2 ? 1 : 2;          // the other two, in index order
  const float wa = ja == 0 ? w[0] : w[1], wb = jb == 1 ? w[1] : w[2];
  const int i2 = wb > wa ? jb : ja;
  const float w1 = i1 == 0 ? w[0] : (i1 == 1 ? w[1] : w[2]), w2 = wb > wa ? wb : wa;
  if (!(w2 > 0.0f) || !(w2 > w1 * ALIGN_MIN_W_RATIO)) return false;          // a collinear (or coincident) set
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
  float out[ALIGN_PARAMS];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) out[3 * r + c] = (u1[r] * v1[c] + u2[r] * v2[c]) + u3[r] * v3[c];
  if (sa == 0.0f) return false;
  const float s = sqrtf(sb / sa);
  if (s == 0.0f || !fundamental_finite(s)) return false;
#pragma unroll
  for (int r = 0; r < 3; r++)
    out[9 + r] = cb[r] - s * ((out[3 * r] * ca[0] + out[3 * r + 1] * ca[1]) + out[3 * r + 2] * ca[2]);
  out[12] = s;
#pragma unroll
  for (int j = 0; j < ALIGN_PARAMS; j++) ok = ok && fundamental_finite(out[j]);
  if (!ok) return false;
#pragma unroll
  for (int j = 0; j < ALIGN_PARAMS; j++) h[j] = out[j];
  return true;
}

// the eleven terms one correspondence adds to the second pass: the nine moments, then its shares of sa and sb
FUND_HD void align_moment_terms(const float (&a)[3], const float (&b)[3], const float (&ca)[3], const float (&cb)[3],
                                float (&x)[ALIGN_MOMENT_SUMS])
{
  const float da[3] = {a[0] - ca[0], a[1] - ca[1], a[2] - ca[2]};
  const float db[3] = {b[0] - cb[0], b[1] - cb[1], b[2] - cb[2]};
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) x[3 * r + c] = db[r] * da[c];
  x[9] = (da[0] * da[0] + da[1] * da[1]) + da[2] * da[2];
  x[10] = (db[0] * db[0] + db[1] * db[1]) + db[2] * db[2];
}

// Step 3 for one sample: a[k], b[k] the k-th correspondence, every sum from +0 in ascending k
FUND_HD bool align_solve3(const float (&a)[3][3], const float (&b)[3][3], float (&h)[ALIGN_PARAMS])
{
  float ca[3], cb[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    ca[j] = (((0.0f + a[0][j]) + a[1][j]) + a[2][j]) / 3.0f;
    cb[j] = (((0.0f + b[0][j]) + b[1][j]) + b[2][j]) / 3.0f;
  }
  float S[ALIGN_MOMENT_SUMS];
#pragma unroll
  for (int j = 0; j < ALIGN_MOMENT_SUMS; j++) S[j] = 0.0f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    float x[ALIGN_MOMENT_SUMS];
    align_moment_terms(a[k], b[k], ca, cb, x);
#pragma unroll
    for (int j = 0; j < ALIGN_MOMENT_SUMS; j++) S[j] = S[j] + x[j];
  }
  const float M[9] = {S[0], S[1], S[2], S[3], S[4], S[5], S[6], S[7], S[8]};
  return align_from_moments(M, S[9], S[10], ca, cb, h);
}

// step 4: the squared distance of b from a under the transform h
FUND_HD float align_error2(const float (&h)[ALIGN_PARAMS], float ax, float ay, float az, float bx, float by, float bz)
{
  const float s = h[12];
  const float d0 = bx - (s * ((h[0] * ax + h[1] * ay) + h[2] * az) + h[9]);
  const float d1 = by - (s * ((h[3] * ax + h[4] * ay) + h[5] * az) + h[10]);
  const float d2 = bz - (s * ((h[6] * ax + h[7] * ay) + h[8] * az) + h[11]);
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

// Step 6: the refits of h over its members and the rms of the final ones.  Cand hands out candidate p's six coordinates
// (load(p, a, b)); Exec provides the 256-slot sum over the candidate position (sum<K>(n, v, out)) and the integer count
// (count(n, pred)) as FundamentalHostExec does on the host and a 256-thread workgroup does on the device.  Every thread
// of the workgroup runs this with the same values, so every branch is uniform.
template <class Exec, class Cand>
FUND_HD void align_refit(Exec &ex, const Cand &cand, int n, float thresh2, int refit_loops, float (&h)[ALIGN_PARAMS],
                         int &members, int &kept, float &rms)
{
  auto member = [&](const float(&g)[ALIGN_PARAMS], int p, float (&a)[3], float (&b)[3], float &e2) {
    cand.load(p, a, b);
    e2 = align_error2(g, a[0], a[1], a[2], b[0], b[1], b[2]);
    return e2 < thresh2;
  };
  auto count_of = [&](const float(&g)[ALIGN_PARAMS]) {
    return ex.count(n, [&](int p) {
      float a[3], b[3], e2;
      return member(g, p, a, b, e2);
    });
  };
  int c = count_of(h);
  kept = 0;
  for (int loop = 0; loop < refit_loops; loop++) {
    if (c < 1) break;
    const float fc = (float)c;
    auto centroid_terms = [&](int p, float (&x)[ALIGN_CENTROID_SUMS]) {
      float a[3], b[3], e2;
      if (!member(h, p, a, b, e2)) return false;
      x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = b[0]; x[4] = b[1]; x[5] = b[2];
      return true;
    };
    float C[ALIGN_CENTROID_SUMS];
    ex.template sum<ALIGN_CENTROID_SUMS>(n, centroid_terms, C);
    const float ca[3] = {C[0] / fc, C[1] / fc, C[2] / fc}, cb[3] = {C[3] / fc, C[4] / fc, C[5] / fc};
    auto moment_terms = [&](int p, float (&x)[ALIGN_MOMENT_SUMS]) {
      float a[3], b[3], e2;
      if (!member(h, p, a, b, e2)) return false;
      align_moment_terms(a, b, ca, cb, x);
      return true;
    };
    float S[ALIGN_MOMENT_SUMS];
    ex.template sum<ALIGN_MOMENT_SUMS>(n, moment_terms, S);
    const float M[9] = {S[0], S[1], S[2], S[3], S[4], S[5], S[6], S[7], S[8]};
    float hp[ALIGN_PARAMS];
    if (!align_from_moments(M, S[9], S[10], ca, cb, hp)) break;  // an invalid refit: h is kept
    const int cp = count_of(hp);
    if (cp < c) break;                         // fewer members: h is kept
#pragma unroll
    for (int j = 0; j < ALIGN_PARAMS; j++) h[j] = hp[j];
    c = cp;
    kept++;
  }
  auto error_term = [&](int p, float (&x)[1]) {
    float a[3], b[3], e2;
    if (!member(h, p, a, b, e2)) return false;
    x[0] = e2;
    return true;
  };
  float E[1];
  ex.template sum<1>(n, error_term, E);
  members = c;
  rms = c > 0 ? pose_one_nan(sqrtf(E[0] / (float)c)) : 0.0f;
}

// misift_transform_scene_batch, one point: s (R X) + t, each result with the one quiet NaN
FUND_HD void align_transform_point(const float *sim, const float (&X)[3], float (&out)[3])
{
  const float s = sim[12];
#pragma unroll
  for (int r = 0; r < 3; r++)
    out[r] = pose_one_nan(s * ((sim[3 * r] * X[0] + sim[3 * r + 1] * X[1]) + sim[3 * r + 2] * X[2]) + sim[9 + r]);
}

// misift_transform_scene_batch, one camera (R_i row-major, t_i): R' = R_i R^T, t' = s t_i - R' t
FUND_HD void align_transform_camera(const float *sim, const float (&cam)[12], float (&out)[12])
{
  const float s = sim[12];
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++)
      out[3 * r + c] = (cam[3 * r] * sim[3 * c] + cam[3 * r + 1] * sim[3 * c + 1]) + cam[3 * r + 2] * sim[3 * c + 2];
    out[9 + r] = s * cam[9 + r] - ((out[3 * r] * sim[9] + out[3 * r + 1] * sim[10]) + out[3 * r + 2] * sim[11]);
  }
#pragma unroll
  for (int j = 0; j < 12; j++) out[j] = pose_one_nan(out[j]);
}

// misift_correspond_tracks_batch: the track of [0, T) whose range of offsets holds slot o, or -1.  The search reads
// offsets[0 .. T] only and its answer is verified, so hostile offsets only drop the record.
FUND_HD int align_track_of(const int *offsets, int T, int o)
{
  if (T < 1) return -1;
  int lo = 0, hi = T;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (offsets[mid] <= o) lo = mid; else hi = mid;
  }
  return (offsets[lo] <= o && o < offsets[lo + 1]) ? lo : -1;
}

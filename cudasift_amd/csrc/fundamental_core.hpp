// fundamental_core.hpp — the arithmetic of misift_find_fundamental_batch / misift_score_fundamental_batch, for host and
// device: the normalised 8-point solve of one RANSAC hypothesis and the Sampson test of one stored match.  The kernels
// (kernels_fundamental.hip) and the host-only test hooks (misift_test_fundamental_solve, _sampson, _error) compile these
// same functions, so what a CPU test pins is what the device runs.
//
// Everything is fp32 with every operation rounded: only + - * /, sqrtf and fabsf, no fmaf, and the build's
// -ffp-contract=off keeps the compiler from fusing.  The order of every sum is written out; tests restate it in numpy.
//
// Convention: (x2, y2, 1) . F . (x1, y1, 1)^T = 0, F row-major in 9 floats.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define FUND_HD __host__ __device__ __forceinline__
#else
#define FUND_HD inline
#endif

// false for NaN and +-inf
FUND_HD bool fundamental_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

// Hartley normalisation of the 8 points of one sample (per sample: no cross-lane sum, nothing order-dependent):
// centroid = sum in sample order * 0.125f, d = sum in sample order of the distances to it, s = 8 sqrt(2) / d.
FUND_HD void fundamental_normalise(const float (&x)[8], const float (&y)[8], float &cx, float &cy, float &s)
{
  float sx = 0.0f, sy = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; k++) { sx = sx + x[k]; sy = sy + y[k]; }
  cx = sx * 0.125f;
  cy = sy * 0.125f;
  float d = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const float dx = x[k] - cx, dy = y[k] - cy;
    d = d + sqrtf(dx * dx + dy * dy);
  }
  s = 11.3137085f / d;
}

// The 8x9 system of one hypothesis, wherever it lives: a plain array on the host, a lane's column of LDS on the device
// (a dynamically indexed array in registers would go to scratch memory).  Mat: float get(r, c), void set(r, c, v).
struct FundamentalArrayMat {
  float a[8][9];
  FUND_HD float get(int r, int c) const { return a[r][c]; }
  FUND_HD void set(int r, int c, float v) { a[r][c] = v; }
};

// F (9 floats, row-major) through the 8 matches (x1, y1) -> (x2, y2); returns whether the hypothesis is valid.  An
// invalid hypothesis (a zero or non-finite pivot, a non-finite entry of F) gets nine zeros, which no match fits.
//   rows      row k = (u2 u1, u2 v1, u2, v2 u1, v2 v1, v2, u1, v1, 1) of the normalised sample
//   eliminate Gaussian elimination with complete pivoting: at step k the entry of rows k..7 x columns k..8 with the
//             largest fabsf, searched row-major with a strict '>' (the first maximum wins, a NaN never does)
//   solve     the one free column = 1, back-substitution, the column permutation undone -> Fn
//   F         T2^T . Fn . T1 with T = [s 0 -s cx; 0 s -s cy; 0 0 1], as computed: no rescaling, no rank-2 projection
template <class Mat>
FUND_HD bool fundamental_solve8(Mat &m, const float (&x1)[8], const float (&y1)[8], const float (&x2)[8],
                                const float (&y2)[8], float (&F)[9])
{
  float c1x, c1y, s1, c2x, c2y, s2;
  fundamental_normalise(x1, y1, c1x, c1y, s1);
  fundamental_normalise(x2, y2, c2x, c2y, s2);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const float u1 = (x1[k] - c1x) * s1, v1 = (y1[k] - c1y) * s1;
    const float u2 = (x2[k] - c2x) * s2, v2 = (y2[k] - c2y) * s2;
    m.set(k, 0, u2 * u1); m.set(k, 1, u2 * v1); m.set(k, 2, u2);
    m.set(k, 3, v2 * u1); m.set(k, 4, v2 * v1); m.set(k, 5, v2);
    m.set(k, 6, u1); m.set(k, 7, v1); m.set(k, 8, 1.0f);
  }
  int col[9];                                  // col[j] = the original column now at position j; indexed statically
#pragma unroll
  for (int j = 0; j < 9; j++) col[j] = j;
  bool ok = true;
  for (int k = 0; k < 8; k++) {
    int pr = k, pc = k;
    float best = -1.0f;
    for (int r = k; r < 8; r++)
      for (int c = k; c < 9; c++) {
        const float v = fabsf(m.get(r, c));
        if (v > best) { best = v; pr = r; pc = c; }
      }
    for (int c = k; c < 9; c++) {              // rows k <-> pr (the columns left of k are dead)
      const float t = m.get(k, c);
      m.set(k, c, m.get(pr, c));
      m.set(pr, c, t);
    }
    for (int r = 0; r < 8; r++) {              // columns k <-> pc, all rows: the rows above feed the back-substitution
      const float t = m.get(r, k);
      m.set(r, k, m.get(r, pc));
      m.set(r, pc, t);
    }
    int ck = 0, cp = 0;
#pragma unroll
    for (int j = 0; j < 9; j++) { ck = j == k ? col[j] : ck; cp = j == pc ? col[j] : cp; }
#pragma unroll
    for (int j = 0; j < 9; j++) col[j] = j == k ? cp : (j == pc ? ck : col[j]);
    const float piv = m.get(k, k);
    ok = ok && piv != 0.0f && fundamental_finite(piv);
    for (int r = k + 1; r < 8; r++) {
      const float f = m.get(r, k) / piv;
      for (int c = k + 1; c < 9; c++) m.set(r, c, m.get(r, c) - f * m.get(k, c));
    }
  }
  float z[9];
  z[8] = 1.0f;
#pragma unroll
  for (int k = 7; k >= 0; k--) {
    float s = 0.0f;
#pragma unroll
    for (int c = k + 1; c < 9; c++) s = s + m.get(k, c) * z[c];
    z[k] = (-s) / m.get(k, k);
  }
  float n[9];
#pragma unroll
  for (int j = 0; j < 9; j++) n[j] = 0.0f;
#pragma unroll
  for (int i = 0; i < 9; i++)
#pragma unroll
    for (int j = 0; j < 9; j++) n[j] = col[i] == j ? z[i] : n[j];
  const float t1x = -(s1 * c1x), t1y = -(s1 * c1y), t2x = -(s2 * c2x), t2y = -(s2 * c2y);
  float g[9];                                  // Fn . T1
#pragma unroll
  for (int i = 0; i < 3; i++) {
    g[3 * i + 0] = n[3 * i + 0] * s1;
    g[3 * i + 1] = n[3 * i + 1] * s1;
    g[3 * i + 2] = (n[3 * i + 0] * t1x + n[3 * i + 1] * t1y) + n[3 * i + 2];
  }
#pragma unroll
  for (int j = 0; j < 3; j++) {                // T2^T . (Fn . T1)
    F[0 + j] = s2 * g[0 + j];
    F[3 + j] = s2 * g[3 + j];
    F[6 + j] = (t2x * g[0 + j] + t2y * g[3 + j]) + g[6 + j];
  }
#pragma unroll
  for (int j = 0; j < 9; j++) ok = ok && fundamental_finite(F[j]);
  if (!ok) {
#pragma unroll
    for (int j = 0; j < 9; j++) F[j] = 0.0f;
  }
  return ok;
}

// The Sampson test of one stored match without its division: with a = F (x1, y1, 1)^T and b = F^T (x2, y2, 1)^T,
// e = x2 a0 + y2 a1 + a2 and den = a0^2 + a1^2 + b0^2 + b1^2, each summed left to right; the squared Sampson distance is
// e^2 / den.  Returns e^2.
FUND_HD float fundamental_sampson(const float (&F)[9], float x1, float y1, float x2, float y2, float &den)
{
  const float a0 = F[0] * x1 + F[1] * y1 + F[2];
  const float a1 = F[3] * x1 + F[4] * y1 + F[5];
  const float a2 = F[6] * x1 + F[7] * y1 + F[8];
  const float b0 = F[0] * x2 + F[3] * y2 + F[6];
  const float b1 = F[1] * x2 + F[4] * y2 + F[7];
  const float e = x2 * a0 + y2 * a1 + a2;
  den = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1;
  return e * e;
}

// a match is an inlier iff e^2 < thresh^2 * den (a comparison with a NaN is false)
FUND_HD bool fundamental_inlier(float e2, float den, float thresh2) { return e2 < thresh2 * den; }

// match_error: the Sampson distance, +inf where den > 0 is false.  A NaN result (e2 NaN, or inf / inf) is stored as the
// one quiet NaN 0x7fc00000: the sign and payload an operation gives a NaN differ from processor to processor (inf - inf
// is 0xffc00000 on x86 and 0x7fc00000 on the GPU), and match_error is the only output of the two calls that can hold one.
FUND_HD float fundamental_error(float e2, float den)
{
  if (!(den > 0.0f)) return INFINITY;
  float d = sqrtf(e2 / den);
  unsigned u;                                  // on the bits: a float select of a NaN for a NaN may be folded away
  __builtin_memcpy(&u, &d, sizeof u);
  if ((u & 0x7fffffffu) > 0x7f800000u) u = 0x7fc00000u;
  __builtin_memcpy(&d, &u, sizeof u);
  return d;
}

// fundamental_core.hpp — the arithmetic of misift_find_fundamental_batch / misift_score_fundamental_batch /
// misift_improve_fundamental_batch, for host and device: the normalised 8-point solve of one RANSAC hypothesis, the
// Sampson test of one stored match, and the refits of an F over its inliers.  The kernels (kernels_fundamental.hip) and
// the host-only test hooks (misift_test_fundamental_solve, _sampson, _error, _refine, _solve9) compile these same
// functions, so what a CPU test pins is what the device runs.
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

// col[j] = the original column now at position j, indexed statically: positions k and pc change places
template <int C>
FUND_HD void fundamental_swap_columns(int (&col)[C], int k, int pc)
{
  int ck = 0, cp = 0;
#pragma unroll
  for (int j = 0; j < C; j++) { ck = j == k ? col[j] : ck; cp = j == pc ? col[j] : cp; }
#pragma unroll
  for (int j = 0; j < C; j++) col[j] = j == k ? cp : (j == pc ? ck : col[j]);
}

// the one free column = 1, back-substitution of rows C-2..0 of the eliminated system, the column permutation undone -> n
template <class Mat, int C>
FUND_HD void fundamental_back_substitute(const Mat &m, const int (&col)[C], float (&n)[C])
{
  float z[C];
  z[C - 1] = 1.0f;
#pragma unroll
  for (int k = C - 2; k >= 0; k--) {
    float s = 0.0f;
#pragma unroll
    for (int c = k + 1; c < C; c++) s = s + m.get(k, c) * z[c];
    z[k] = (-s) / m.get(k, k);
  }
#pragma unroll
  for (int j = 0; j < C; j++) n[j] = 0.0f;
#pragma unroll
  for (int i = 0; i < C; i++)
#pragma unroll
    for (int j = 0; j < C; j++) n[j] = col[i] == j ? z[i] : n[j];
}

// The elimination and the solve of an R x C system, C taken from n (C = 9 with R = 8: one hypothesis, R = 9: the moment
// matrix of a refinement; C = 12 with R = 11: the six-point resection of resect_core.hpp), C - 1 steps whatever R;
// returns whether every pivot was non-zero and finite.  n = the solution, C floats.
//   eliminate Gaussian elimination with complete pivoting: at step k the entry of rows k..R-1 x columns k..C-1 with the
//             largest fabsf, searched row-major with a strict '>' (the first maximum wins, a NaN never does)
//   solve     the one free column = 1, back-substitution of rows C-2..0, the column permutation undone -> n
template <int R, class Mat, int C>
FUND_HD bool fundamental_eliminate(Mat &m, float (&n)[C])
{
  static_assert(R >= C - 1, "a row per elimination step");
  int col[C];                                  // col[j] = the original column now at position j; indexed statically
#pragma unroll
  for (int j = 0; j < C; j++) col[j] = j;
  bool ok = true;
  for (int k = 0; k < C - 1; k++) {
    int pr = k, pc = k;
    float best = -1.0f;
    for (int r = k; r < R; r++)
      for (int c = k; c < C; c++) {
        const float v = fabsf(m.get(r, c));
        if (v > best) { best = v; pr = r; pc = c; }
      }
    for (int c = k; c < C; c++) {              // rows k <-> pr (the columns left of k are dead)
      const float t = m.get(k, c);
      m.set(k, c, m.get(pr, c));
      m.set(pr, c, t);
    }
    for (int r = 0; r < R; r++) {              // columns k <-> pc, all rows: the rows above feed the back-substitution
      const float t = m.get(r, k);
      m.set(r, k, m.get(r, pc));
      m.set(r, pc, t);
    }
    fundamental_swap_columns(col, k, pc);
    const float piv = m.get(k, k);
    ok = ok && piv != 0.0f && fundamental_finite(piv);
    for (int r = k + 1; r < R; r++) {
      const float f = m.get(r, k) / piv;
      for (int c = k + 1; c < C; c++) m.set(r, c, m.get(r, c) - f * m.get(k, c));
    }
  }
  fundamental_back_substitute(m, col, n);
  return ok;
}

// F = T2^T . Fn . T1 with T = [s 0 -s cx; 0 s -s cy; 0 0 1], as computed: no rescaling, no rank-2 projection.  Returns
// whether every entry of F is finite.
FUND_HD bool fundamental_denormalise(const float (&n)[9], float c1x, float c1y, float s1, float c2x, float c2y, float s2,
                                     float (&F)[9])
{
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
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 9; j++) ok = ok && fundamental_finite(F[j]);
  return ok;
}

// the row of one normalised match in the 9-column system: (u2 u1, u2 v1, u2, v2 u1, v2 v1, v2, u1, v1, 1)
FUND_HD void fundamental_row(float u1, float v1, float u2, float v2, float (&a)[9])
{
  a[0] = u2 * u1; a[1] = u2 * v1; a[2] = u2;
  a[3] = v2 * u1; a[4] = v2 * v1; a[5] = v2;
  a[6] = u1; a[7] = v1; a[8] = 1.0f;
}

// F (9 floats, row-major) through the 8 matches (x1, y1) -> (x2, y2); returns whether the hypothesis is valid.  An
// invalid hypothesis (a zero or non-finite pivot, a non-finite entry of F) gets nine zeros, which no match fits.
//   rows      row k = fundamental_row of the normalised sample
//   solve     fundamental_eliminate<8> -> Fn
//   F         fundamental_denormalise
template <class Mat>
FUND_HD bool fundamental_solve8(Mat &m, const float (&x1)[8], const float (&y1)[8], const float (&x2)[8],
                                const float (&y2)[8], float (&F)[9])
{
  float c1x, c1y, s1, c2x, c2y, s2;
  fundamental_normalise(x1, y1, c1x, c1y, s1);
  fundamental_normalise(x2, y2, c2x, c2y, s2);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    float a[9];
    fundamental_row((x1[k] - c1x) * s1, (y1[k] - c1y) * s1, (x2[k] - c2x) * s2, (y2[k] - c2y) * s2, a);
#pragma unroll
    for (int j = 0; j < 9; j++) m.set(k, j, a[j]);
  }
  float n[9];
  bool ok = fundamental_eliminate<8>(m, n);
  ok = fundamental_denormalise(n, c1x, c1y, s1, c2x, c2y, s2, F) && ok;
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

// ---- misift_improve_fundamental_batch: refits of F over its inliers (the definition is in include/misift.h)
//
// The sum of the call: every floating-point sum over a record set runs through FUND_SLOTS partial sums, slot t adding
// the members r = t, t + 256, ... in ascending order from +0.0f (a record that is no member is skipped, it does not add
// zero), then a halving tree p[t] = p[t] + p[t + off], off = 128 ... 1.  On the device the slot is the thread, on the
// host a loop index; both run the two functions below, so the order of every sum is written here once.
constexpr int FUND_SLOTS = 256;
constexpr int FUND_MOMENTS = 45;               // the upper triangle of the 9x9 moment matrix, row-major

// slot t's partial sums of the K values v(r, x) hands out for each member r (v returns false for a record to skip)
template <int K, class V>
FUND_HD void fundamental_slot_partial(int t, int n, V &v, float (&p)[K])
{
#pragma unroll
  for (int k = 0; k < K; k++) p[k] = 0.0f;
  for (int r = t; r < n; r += FUND_SLOTS) {
    float x[K];
    if (v(r, x)) {
#pragma unroll
      for (int k = 0; k < K; k++) p[k] = p[k] + x[k];
    }
  }
}

// one step of the tree for slot t < off; p holds K rows of FUND_SLOTS partial sums
template <int K>
FUND_HD void fundamental_tree_step(float *p, int t, int off)
{
#pragma unroll
  for (int k = 0; k < K; k++) p[k * FUND_SLOTS + t] = p[k * FUND_SLOTS + t] + p[k * FUND_SLOTS + t + off];
}

// the 9x9 moment matrix, row-major in 81 floats wherever they live (LDS on the device)
struct FundamentalSquareMat {
  float *a;
  FUND_HD float get(int r, int c) const { return a[9 * r + c]; }
  FUND_HD void set(int r, int c, float v) { a[9 * r + c] = v; }
};

// the symmetric matrix from its 45 sums
FUND_HD void fundamental_fill_moments(FundamentalSquareMat &m, const float (&M)[FUND_MOMENTS])
{
  int i = 0;
#pragma unroll
  for (int p = 0; p < 9; p++)
#pragma unroll
    for (int q = p; q < 9; q++) {
      m.set(p, q, M[i]);
      m.set(q, p, M[i]);
      i++;
    }
}

// The same eight steps on the 9x9 matrix spread over 81 lanes, lane t owning entry (t / 9, t % 9): every entry's update
// in a step is one expression of the entries before the step, and the pivot is the smallest row-major index among the
// largest fabsf, so the bits are those of fundamental_eliminate<9>.  A step, with sA the entries before it:
//   key      fundamental_pivot_key of every lane: fabsf's bits above the complement of the index, 0 for a NaN or an
//            entry outside rows k..8 x columns k..8; the largest key is the pivot (none above 0: the entry (k, k))
//   row key  the largest key of each row, then of the nine rows
//   step     fundamental_lane_step: the lane's entry after the two swaps and the row operation
// On the device a lane is a thread and a barrier separates the three; on the host they are loops.
FUND_HD unsigned long long fundamental_pivot_key(float a, int t, int k)
{
  const int r = t / 9, c = t % 9;
  const float v = fabsf(a);
  if (r < k || c < k || v != v) return 0ull;
  unsigned u;
  __builtin_memcpy(&u, &v, sizeof u);
  return ((unsigned long long)u << 32) | (unsigned long long)(0xffffffffu - (unsigned)t);
}

FUND_HD unsigned long long fundamental_row_key(const unsigned long long *key, int r)
{
  unsigned long long best = 0ull;
#pragma unroll
  for (int c = 0; c < 9; c++) best = key[9 * r + c] > best ? key[9 * r + c] : best;
  return best;
}

FUND_HD float fundamental_lane_step(const float *sA, const unsigned long long *rowkey, int t, int k, int &pc, float &piv)
{
  unsigned long long best = 0ull;
#pragma unroll
  for (int j = 0; j < 9; j++) best = rowkey[j] > best ? rowkey[j] : best;
  int pr = k;
  pc = k;
  if (best != 0ull) {
    const int i = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
    pr = i / 9;
    pc = i % 9;
  }
  const int r = t / 9, c = t % 9;
  const int sr = r == k ? pr : (r == pr ? k : r), sc = c == k ? pc : (c == pc ? k : c);
  float a = sA[9 * sr + sc];                   // rows k <-> pr, columns k <-> pc
  piv = sA[9 * pr + pc];
  if (r > k && c > k) {
    const float f = sA[9 * sr + pc] / piv;
    a = a - f * sA[9 * pr + sc];
  }
  return a;
}

// the lanes one after another, for the host: what misift_test_fundamental_solve9 holds against fundamental_eliminate<9>
inline bool fundamental_eliminate_lanes(const float *M81, float (&n)[9])
{
  float a[81], sA[81];
  unsigned long long key[81], rowkey[9];
  int col[9];
  for (int j = 0; j < 9; j++) col[j] = j;
  for (int t = 0; t < 81; t++) a[t] = M81[t];
  bool ok = true;
  for (int k = 0; k < 8; k++) {
    int pc = k;
    float piv = 0.0f;
    for (int t = 0; t < 81; t++) { sA[t] = a[t]; key[t] = fundamental_pivot_key(a[t], t, k); }
    for (int r = 0; r < 9; r++) rowkey[r] = fundamental_row_key(key, r);
    for (int t = 0; t < 81; t++) a[t] = fundamental_lane_step(sA, rowkey, t, k, pc, piv);
    ok = ok && piv != 0.0f && fundamental_finite(piv);
    fundamental_swap_columns(col, k, pc);
  }
  const FundamentalSquareMat m{a};
  fundamental_back_substitute(m, col, n);
  return ok;
}

// The rounds of the definition.  Recs: bool load(r, x1, y1, x2, y2) hands out record r's coordinates and returns whether
// it passes the gate.  Exec runs the 256 slots (threads of a workgroup, or a loop):
//   sum<K>(n, v, out)   the sum of the call of v's K values over its members, the same out[] in every slot
//   count(n, pred)      how many r < n satisfy pred
//   solve(M, c1x .. s2, F')   the 9x9 solve of the 45 moments and the denormalisation; returns whether F' is valid
// On entry F is the start; on return F, c = |inl(F)| and the rounds accepted.
template <class Exec, class Recs>
FUND_HD void fundamental_refine(Exec &ex, const Recs &recs, int n, float thresh2, int num_loops, float (&F)[9], int &c,
                                int &rounds)
{
  const auto member = [&](const float (&G)[9], int r, float &x1, float &y1, float &x2, float &y2) {
    const bool gate = recs.load(r, x1, y1, x2, y2);
    float den;
    const float e2 = fundamental_sampson(G, x1, y1, x2, y2, den);
    return gate && fundamental_inlier(e2, den, thresh2);
  };
  const auto inlier_of = [&](const float (&G)[9]) {
    return ex.count(n, [&](int r) {
      float x1, y1, x2, y2;
      return member(G, r, x1, y1, x2, y2);
    });
  };
  c = inlier_of(F);
  rounds = 0;
  for (int loop = 0; loop < num_loops; loop++) {
    if (c < 8) break;
    const float fc = (float)c;
    float s4[4];                               // centroids over S = inl(F)
    auto coords = [&](int r, float (&x)[4]) { return member(F, r, x[0], x[1], x[2], x[3]); };
    ex.template sum<4>(n, coords, s4);
    const float c1x = s4[0] / fc, c1y = s4[1] / fc, c2x = s4[2] / fc, c2y = s4[3] / fc;
    float d2[2];                               // distances to them
    auto dists = [&](int r, float (&x)[2]) {
      float x1, y1, x2, y2;
      if (!member(F, r, x1, y1, x2, y2)) return false;
      const float dx1 = x1 - c1x, dy1 = y1 - c1y, dx2 = x2 - c2x, dy2 = y2 - c2y;
      x[0] = sqrtf(dx1 * dx1 + dy1 * dy1);
      x[1] = sqrtf(dx2 * dx2 + dy2 * dy2);
      return true;
    };
    ex.template sum<2>(n, dists, d2);
    const float s1 = (fc * 1.41421354f) / d2[0], s2 = (fc * 1.41421354f) / d2[1];
    float M[FUND_MOMENTS];                     // M[r][c'] = SUM(a[r] * a[c']), r <= c'
    auto moments = [&](int r, float (&x)[FUND_MOMENTS]) {
      float x1, y1, x2, y2;
      if (!member(F, r, x1, y1, x2, y2)) return false;
      float a[9];
      fundamental_row((x1 - c1x) * s1, (y1 - c1y) * s1, (x2 - c2x) * s2, (y2 - c2y) * s2, a);
      int i = 0;
#pragma unroll
      for (int p = 0; p < 9; p++)
#pragma unroll
        for (int q = p; q < 9; q++) x[i++] = a[p] * a[q];
      return true;
    };
    ex.template sum<FUND_MOMENTS>(n, moments, M);
    float Fp[9];                               // the 9x9 solve and the denormalisation
    if (!ex.solve(M, c1x, c1y, s1, c2x, c2y, s2, Fp)) break;     // an invalid solve: F is kept
    const int cp = inlier_of(Fp);
    if (cp < c) break;                         // fewer inliers: F is kept
#pragma unroll
    for (int j = 0; j < 9; j++) F[j] = Fp[j];
    c = cp;
    rounds++;
  }
}

// the host's Exec and Recs: plain arrays, the slots one after another
struct FundamentalHostExec {
  float p[FUND_MOMENTS * FUND_SLOTS], m[81];
  template <int K, class V>
  void sum(int n, V &v, float (&out)[K])
  {
    for (int t = 0; t < FUND_SLOTS; t++) {
      float acc[K];
      fundamental_slot_partial<K>(t, n, v, acc);
      for (int k = 0; k < K; k++) p[k * FUND_SLOTS + t] = acc[k];
    }
    for (int off = FUND_SLOTS / 2; off > 0; off >>= 1)
      for (int t = 0; t < off; t++) fundamental_tree_step<K>(p, t, off);
    for (int k = 0; k < K; k++) out[k] = p[k * FUND_SLOTS];
  }
  template <class P>
  int count(int n, P pred)
  {
    int c = 0;
    for (int r = 0; r < n; r++) c += pred(r) ? 1 : 0;
    return c;
  }
  bool solve(const float (&M)[FUND_MOMENTS], float c1x, float c1y, float s1, float c2x, float c2y, float s2,
             float (&Fp)[9])
  {
    FundamentalSquareMat mat{m};
    fundamental_fill_moments(mat, M);
    float nf[9];
    const bool ok = fundamental_eliminate_lanes(m, nf);          // the kernel's form, its lanes one after another
    return fundamental_denormalise(nf, c1x, c1y, s1, c2x, c2y, s2, Fp) && ok;
  }
};

struct FundamentalHostRecs {
  const float *xy;                             // n x 4: x1 y1 x2 y2
  const unsigned char *gate;                   // n
  bool load(int r, float &x1, float &y1, float &x2, float &y2) const
  {
    x1 = xy[4 * r]; y1 = xy[4 * r + 1]; x2 = xy[4 * r + 2]; y2 = xy[4 * r + 3];
    return gate[r] != 0;
  }
};

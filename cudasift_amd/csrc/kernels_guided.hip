// kernels_guided.hip — homography-guided and epipolar-guided matching of many frame pairs of a device-resident batch
// (misift_match_guided_batch, misift_match_epipolar_batch; the second is described after the first).
//
// The reference runs this step only as a host diagnostic (MatchAll, mainSift.cpp:95-147): for every point of set 1 it
// projects (x, y) through H and scores only the points of set 2 that lie within a radius of the projection.  Here the
// candidates' exact top-2 takes the place of the global one that misift_match_batch writes.
//
// Two launches whatever the number of pairs:
//   bin    one 1024-thread workgroup per distinct set-2 frame (the host dedupes them from the pairs): the bounding box of
//          the frame's finite positions (an LDS reduction), a grid of at most 64 x 64 cells each at least r' wide where
//          the box allows it, then a counting sort in LDS (cell counts by LDS atomics, a scan, a scatter) into a
//          compact cell-ordered array of (x2, y2, j) and the cells' starts.  Records with a non-finite position are
//          left out: their gate error is never finite, so they are never candidates.  One extra workgroup reads the
//          pairs' counts on the device and writes the work list: (pair, 64-row group) items, numbered by an
//          exclusive prefix sum (block_scan), as misift_match_batch's plan does, and zeroes (or sets to -1) num_found.
//   match  a persistent grid of one-wave workgroups over the items.  Each lane projects one row and walks the entries
//          of the cells its disc can reach, one entry per step, testing the exact gate.  The passing (row, candidate)
//          pairs are compacted through a wave prefix sum into an LDS queue; every 64 of them, each lane computes one
//          full 128-term fmaf chain (float4 loads) and the scores are merged into the rows' top-2 kept in LDS, in
//          rounds that give each row at most one writer.
//
// Conservative gather: a candidate passes fl(fl(dx*dx) + fl(dy*dy)) < fl(r*r), so |px - x2| < r(1 + 2^-21) + 2^-70
// (rounding of dx, dx*dx, the sum and r*r, and the underflow of dx*dx), and r' = r(1 + 2^-10) + 1e-20 exceeds that.
// The cell of a coordinate p is gm_cell((p - p0) * inv) in double, a non-decreasing function of p, and a row visits the
// cells of fl(px - r') .. fl(px + r'), so every candidate's cell is visited whatever the cell size; the exact gate then
// decides.  The top-2 merge (score descending, index ascending; only scores > 0 count; a second copy of the best
// score is the runner-up) uses comparisons only, so the result does not depend on the order of the candidates.
//
// Epipolar-guided matching (misift_match_epipolar_batch) is the same two launches with another gather: the bin kernel
// as it is, then epipolar_match_kernel, which shares the queue, the scoring, the merge and the write-back with
// guided_match_kernel (the gm_* functions below) and differs only in which entries a lane tests.  A lane owns one row
// and its epipolar line a0 x2 + a1 y2 + a2 = 0 (epipolar_core.hpp).  It walks the grid rows cy that the band around
// the line can reach inside the bounding box, and in each row the contiguous entries starts[cy gx + cx0] ..
// starts[cy gx + cx1 + 1] of the cell span [cx0, cx1] that the band covers inside that row's y-slab, testing the exact
// gate on each.  The gate decides; the walk only has to be conservative, for every finite input:
//
//   1. What the gate admits.  With u = 2^-24, S = |a0| X + |a1| Y + |a2| (X, Y the largest |x2|, |y2| of the box),
//      n = sqrt(a0^2 + a1^2) and E = a0 x2 + a1 y2 + a2 in real arithmetic on the fp32 values, the gate computes
//      e = fl(fl(fl(x2 a0) + fl(y2 a1)) + a2), so |e - E| <= 3u(1 + u)^2 S + 3 * 2^-150 < 2^-22 S + 2^-148: an ABSOLUTE
//      error, of the size of the disc's whole margin when coordinates are thousands of pixels, so the band needs an
//      absolute slack on top of r' n.  A record passes iff fl(e e) < fl(r2 n2), where fl(e e) >= e^2 (1 - u) - 2^-150,
//      r2 = fl(r r) <= r^2 (1 + u) + 2^-150 and n2 <= n^2 (1 + u)^2 + 3 * 2^-150.  Taking roots term by term
//      (sqrt(p + q) <= sqrt(p) + sqrt(q)): |e| < (r (1 + u) + 2^-75)(n (1 + u) + 2^-74)(1 + u)^2 + 2^-75.  So a passing
//      record has |E| < w_need = (r (1 + 2^-21) + 2^-74)(n + 2^-73) + 2^-22 S + 2^-74, and the band's half-width
//          w = r' (n + 2^-70) + 2^-20 S + 2^-70,  r' = r (1 + 2^-10) + 1e-20
//      exceeds it term by term, each by a factor of at least 1 + 2^-11: w_need <= w (1 - 2^-12).  A right-hand side that
//      overflows to +inf admits every finite e e, i.e. |e| < 2^64; then r^2 n^2 (1 + u)^4 >= 2^128 (1 - u), so
//      r' n > 2^64 and the same w covers it; r = +inf gives w = +inf.  Rows with a non-finite a0, a1, a2 or n2, or with
//      n2 == 0, have no candidate at all and walk nothing, so n > 0 and w is finite or +inf, never a NaN.
//   2. Box coordinates.  The bin puts a record into cell (gm_cell(fl(uf ix)), gm_cell(fl(vf iy))) with uf = fl(x2 - x0),
//      vf = fl(y2 - y0) in double; 0 <= uf <= rx and 0 <= vf <= ry, the box's extents as the grid function computes them
//      (the same subtraction of the extreme record).  The walk works on (uf, vf): the band is |a uf + b vf + c| <= w with
//      c = fl(a0 x0 + a1 y0 + a2) in double.  Replacing (x2 - x0, y2 - y0) by (uf, vf) and the real c by the computed
//      one moves E by at most 2^-50 S.
//   3. Extents (epipolar_extent).  Over an interval of one coordinate the other's range in the band is an interval
//      whose ends are attained at the interval's ends with -w / +w, because the numerator is linear.  The double
//      arithmetic of those ends (two products, two sums, a product with the rounded reciprocal) errs by at most
//      2^-49 (3 S + w) / |k|, k the coefficient divided by.  Items 2 and 3 together cost less than 2^-48 (3 S + w) in E,
//      and the slack w - w_need >= 2^-12 w >= 2^-13 w + 2^-33 S is larger.  An end that overflows lies beyond the box
//      on its true side; k == 0 (an exactly horizontal or vertical line) yields +-inf ends by the numerators' signs,
//      i.e. the whole axis when the band meets the interval and nothing when it misses; a NaN end (0 * inf) is taken
//      as the whole axis.  No case needs a branch of its own.
//   4. Rows.  Every record has uf in [0, rx], so its vf lies in the extent over [0, rx]; gm_cell(fl(v iy)) is a
//      non-decreasing function of v, so its row lies in [cell(lo), cell(hi)].  An extent wholly outside [0, ry] means
//      the line misses the box and the row visits nothing.  A near-horizontal line gets the few rows it touches.
//   5. Slabs.  A record of row 0 < cy < gy - 1 has cy <= fl(vf iy) < cy + 1, so vf lies in
//      [(cy - 2^-20) ch, (cy + 1 + 2^-20) ch] with ch = fl(1 / iy): the 2^-20 of a cell swallows the 2^-51 relative
//      error of the two roundings (cy <= 63).  Row 0 starts at 0 and row gy - 1 ends at ry, whatever the cell height,
//      so clamping in gm_cell needs no argument.  The record's uf lies in the extent over that slab, and by the same
//      monotonicity its column in [cell(lo), cell(hi)]; an extent outside [0, rx] skips the row.  With r' = +inf the
//      grid is one cell (ix = iy = 0: inf * 0 is a NaN, which gm_cell maps to cell 0) and everything is visited.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "epipolar_core.hpp"

namespace {

constexpr int GM_GRID = 64;                         // cells per axis at most
constexpr int GM_STARTS = GM_GRID * GM_GRID + 4;    // cell starts per frame (4096 + 1, rounded up to 16 bytes)
constexpr int GM_ITEMS_PER_CU = 16;                 // one-wave workgroups per CU of the match grid

struct GmGrid {                  // one per distinct set-2 frame, written by the bin kernel
  double x0, y0, ix, iy;         // cell of (x, y): gm_cell((x - x0) * ix, gx), gm_cell((y - y0) * iy, gy)
  long long base2;               // first record of the frame
  int gx, gy;
  double x1, y1;                 // the far corner of the bounding box; rx = x1 - x0, ry = y1 - y0
};
struct GmPair {                  // one per pair, written by the plan workgroup
  long long base1;               // first record of the set-1 frame
  int n1, d;                     // set-1 records; index of the pair's set-2 frame among the distinct ones
};

struct GmArgs {
  BatchLayout set1, set2;
  const int *pairs;              // pinned host: npairs x 2, then pair_d[npairs], then distinct[nd]
  const int *pair_d, *distinct;
  int npairs, nd, max_pts;
  double rp;                     // r', the gather's half-width
  float r2;                      // fl(radius * radius), the gate
  const float *H;                // npairs x 9: the homographies, or the fundamental matrices of the epipolar call
  int *num_found;                // npairs, or NULL
  // temp
  int *item0;                    // npairs + 1: first item of each pair, item0[npairs] = items in all
  GmPair *pinfo;
  GmGrid *grid;
  int *starts;                   // nd x GM_STARTS
  float4 *entries;               // nd x max_pts: (x2, y2, j as int bits, 0)
};

__host__ __device__ __forceinline__ int gm_cell(double v, int g)
{
  return v >= (double)(g - 1) ? g - 1 : (v > 0.0 ? (int)v : 0);   // NaN -> 0; (int) of a positive v is its floor
}

// The grid of a frame whose finite positions span [xmin, xmax] x [ymin, ymax] (xmin > xmax: none): cells at least r'
// wide, at most 64 per axis.  The bin kernel and the host-only gather hook build it from this one function.
__host__ __device__ __forceinline__ GmGrid gm_make_grid(float xmin, float xmax, float ymin, float ymax, double rp,
                                                        long long base2)
{
  GmGrid G;
  const bool any = xmin <= xmax;
  G.x0 = any ? (double)xmin : 0.0;
  G.y0 = any ? (double)ymin : 0.0;
  const double rx = any ? (double)xmax - G.x0 : 0.0, ry = any ? (double)ymax - G.y0 : 0.0;
  const double cw = fmax(rx / GM_GRID, rp), ch = fmax(ry / GM_GRID, rp);           // > 0: r' > 0
  G.gx = (int)(rx / cw) + 1 < GM_GRID ? (int)(rx / cw) + 1 : GM_GRID;
  G.gy = (int)(ry / ch) + 1 < GM_GRID ? (int)(ry / ch) + 1 : GM_GRID;
  G.ix = 1.0 / cw;                                                                 // r' = inf: 0, one cell
  G.iy = 1.0 / ch;
  G.base2 = base2;
  G.x1 = any ? (double)xmax : 0.0;
  G.y1 = any ? (double)ymax : 0.0;
  return G;
}

__host__ __device__ __forceinline__ bool gm_finite(float v) { return __builtin_isfinite(v); }

// The disc walk of the homography-guided call: the cell rectangle [cx0, cx1] x [cy0, cy1] of fl(px - r') .. fl(px + r')
// (cx1 < cx0 and cy1 < cy0, an empty range, and false for a non-finite projection).  The match kernel and the host-only
// gather hook walk the rectangle this one function gives.
__host__ __device__ __forceinline__ bool gm_disc(const GmGrid &G, float px, float py, double rp, int &cx0, int &cx1,
                                                 int &cy0, int &cy1)
{
  cx0 = 0; cx1 = -1; cy0 = 0; cy1 = -1;
  if (!(gm_finite(px) && gm_finite(py))) return false;
  const double dx = (double)px, dy = (double)py;
  cx0 = gm_cell((dx - rp - G.x0) * G.ix, G.gx);
  cx1 = gm_cell((dx + rp - G.x0) * G.ix, G.gx);
  cy0 = gm_cell((dy - rp - G.y0) * G.iy, G.gy);
  cy1 = gm_cell((dy + rp - G.y0) * G.iy, G.gy);
  return true;
}

// The work list: item0[p] = first (pair, 64-row group) item of pair p.  A pair over max_pts on either side gets
// num_found -1 and no items, a pair with an empty side 0 and no items.
__device__ void gm_plan(const GmArgs &A)
{
  __shared__ int s_scan[16][1];
  const int tid = threadIdx.x;
  int carry = 0;
  for (int base = 0; base < A.npairs; base += 1024) {
    const int p = base + tid;
    int items[1] = {0};
    if (p < A.npairs) {
      const int f1 = A.pairs[2 * p], f2 = A.pairs[2 * p + 1];
      const int n1 = max(A.set1.counts[f1], 0), n2 = max(A.set2.counts[f2], 0);
      const bool over = n1 > A.max_pts || n2 > A.max_pts;
      if (!over && n1 > 0 && n2 > 0) items[0] = (n1 + 63) / 64;
      GmPair P;
      P.base1 = A.set1.base(f1);
      P.n1 = n1;
      P.d = A.pair_d[p];
      A.pinfo[p] = P;
      if (A.num_found) A.num_found[p] = over ? -1 : 0;
    }
    int tot[1];
    block_scan(items, tot, s_scan);
    if (p < A.npairs) A.item0[p] = carry + items[0];
    carry += tot[0];
  }
  if (tid == 0) A.item0[A.npairs] = carry;
}

__global__ __launch_bounds__(1024) void guided_bin_kernel(GmArgs A)
{
  if ((int)blockIdx.x == A.nd) {
    gm_plan(A);
    return;
  }
  __shared__ int s_cnt[GM_GRID * GM_GRID];
  __shared__ float s_red[4][16];
  __shared__ int s_scan[16][1];
  __shared__ double s_g[4];
  __shared__ int s_gi[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = blockIdx.x, f = A.distinct[d];
  const int n2 = max(A.set2.counts[f], 0);
  if (n2 == 0 || n2 > A.max_pts) return;            // no pair of this frame has items
  const long long base2 = A.set2.base(f);
  const SiftPointD *rec = A.set2.recs + base2;
  // 1. bounding box of the finite positions
  float xmin = __builtin_inff(), ymin = __builtin_inff(), xmax = -__builtin_inff(), ymax = -__builtin_inff();
  for (int j = tid; j < n2; j += 1024) {
    const float x = rec[j].xpos, y = rec[j].ypos;
    if (gm_finite(x) && gm_finite(y)) {
      xmin = fminf(xmin, x); xmax = fmaxf(xmax, x);
      ymin = fminf(ymin, y); ymax = fmaxf(ymax, y);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    xmin = fminf(xmin, __shfl_xor(xmin, o, 64)); xmax = fmaxf(xmax, __shfl_xor(xmax, o, 64));
    ymin = fminf(ymin, __shfl_xor(ymin, o, 64)); ymax = fmaxf(ymax, __shfl_xor(ymax, o, 64));
  }
  if (lane == 0) { s_red[0][wave] = xmin; s_red[1][wave] = xmax; s_red[2][wave] = ymin; s_red[3][wave] = ymax; }
  for (int c = tid; c < GM_GRID * GM_GRID; c += 1024) s_cnt[c] = 0;
  __syncthreads();
  // 2. the grid: cells at least r' wide, at most 64 per axis
  if (tid == 0) {
    for (int w = 1; w < 16; w++) {
      s_red[0][0] = fminf(s_red[0][0], s_red[0][w]); s_red[1][0] = fmaxf(s_red[1][0], s_red[1][w]);
      s_red[2][0] = fminf(s_red[2][0], s_red[2][w]); s_red[3][0] = fmaxf(s_red[3][0], s_red[3][w]);
    }
    const GmGrid G = gm_make_grid(s_red[0][0], s_red[1][0], s_red[2][0], s_red[3][0], A.rp, base2);
    A.grid[d] = G;
    s_g[0] = G.x0; s_g[1] = G.y0; s_g[2] = G.ix; s_g[3] = G.iy;
    s_gi[0] = G.gx; s_gi[1] = G.gy;
  }
  __syncthreads();
  const double x0 = s_g[0], y0 = s_g[1], ix = s_g[2], iy = s_g[3];
  const int gx = s_gi[0], gy = s_gi[1], ncell = gx * gy;
  // 3. counting sort: counts, scan, scatter
  for (int j = tid; j < n2; j += 1024) {
    const float x = rec[j].xpos, y = rec[j].ypos;
    if (gm_finite(x) && gm_finite(y))
      atomicAdd(&s_cnt[gm_cell(((double)y - y0) * iy, gy) * gx + gm_cell(((double)x - x0) * ix, gx)], 1);
  }
  __syncthreads();
  int *starts = A.starts + (size_t)d * GM_STARTS;
  int v[4], run[1] = {0};
  for (int k = 0; k < 4; k++) {
    const int c = 4 * tid + k;
    v[k] = c < ncell ? s_cnt[c] : 0;
    run[0] += v[k];
  }
  int tot[1];
  block_scan(run, tot, s_scan);
  for (int k = 0; k < 4; k++) {
    const int c = 4 * tid + k;
    if (c < ncell) { starts[c] = run[0]; s_cnt[c] = run[0]; }
    run[0] += v[k];
  }
  if (tid == 0) starts[ncell] = tot[0];
  __syncthreads();
  float4 *ent = A.entries + (size_t)d * A.max_pts;
  for (int j = tid; j < n2; j += 1024) {
    const float x = rec[j].xpos, y = rec[j].ypos;
    if (gm_finite(x) && gm_finite(y)) {
      const int c = gm_cell(((double)y - y0) * iy, gy) * gx + gm_cell(((double)x - x0) * ix, gx);
      const int pos = atomicAdd(&s_cnt[c], 1);       // < tot <= n2 <= max_pts
      ent[pos] = make_float4(x, y, __int_as_float(j), 0.0f);
    }
  }
}

// merge one candidate (score sc > 0, index j) into a row's top-2
__device__ __forceinline__ void gm_merge(float &b, float &s, int &i, float sc, int j)
{
  if (sc > b) { s = b; b = sc; i = j; }
  else if (sc == b) { s = sc; i = min(i, j); }
  else if (sc > s) s = sc;
}

// ---- what the two match kernels share: the work item, the LDS queue, the scoring, the merge and the write-back

struct GmLds {                                       // 3 KB per one-wave workgroup
  int q_row[128], q_j[128];                          // queue of (row lane, candidate) pairs, < 128 between batches
  float best[64], sec[64];
  int idx[64], own[64];
};

// the last pair whose first item is <= it
__device__ __forceinline__ int gm_item_pair(const GmArgs &A, int it)
{
  int lo = 0, hi = A.npairs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (A.item0[mid] <= it) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ void gm_reset_rows(GmLds &S, int lane)
{
  S.best[lane] = 0.0f; S.sec[lane] = 0.0f; S.idx[lane] = 0x7fffffff;
}

// append the passing lanes' (row lane, candidate) pairs, compacted through a wave prefix sum; returns the new length
__device__ __forceinline__ int gm_enqueue(GmLds &S, int qn, bool pass, int lane, int j)
{
  const unsigned long long m = __ballot(pass);
  if (pass) {
    const int k = qn + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    S.q_row[k] = lane;
    S.q_j[k] = j;
  }
  return qn + __popcll(m);
}

// score 64 queued pairs (fewer at the end), one per lane, and merge them into the rows' top-2; returns the new length
__device__ __forceinline__ int gm_score_merge(GmLds &S, int qn, int lane, const SiftPointD *rows, const SiftPointD *rec2)
{
  __syncthreads();
  const int take = min(qn, 64);
  int rl = 0, cj = 0;
  float sc = 0.0f;
  if (lane < take) {
    rl = S.q_row[lane];
    cj = S.q_j[lane];
    const float4 *a = reinterpret_cast<const float4 *>(rows[rl].data);
    const float4 *b = reinterpret_cast<const float4 *>(rec2[cj].data);
    for (int k = 0; k < 32; k++) {                 // orc_dot128: k = 0..127 in order
      const float4 u = a[k], w = b[k];
      sc = __builtin_fmaf(u.x, w.x, sc);
      sc = __builtin_fmaf(u.y, w.y, sc);
      sc = __builtin_fmaf(u.z, w.z, sc);
      sc = __builtin_fmaf(u.w, w.w, sc);
    }
  }
  bool pend = lane < take && sc > 0.0f;
  __syncthreads();
  if (lane + 64 < qn) { S.q_row[lane] = S.q_row[lane + 64]; S.q_j[lane] = S.q_j[lane + 64]; }
  // each round one writer per row: the last lane to claim it
  while (__any(pend)) {
    if (pend) S.own[rl] = lane;
    __syncthreads();
    if (pend && S.own[rl] == lane) {
      float b = S.best[rl], s = S.sec[rl];
      int i = S.idx[rl];
      gm_merge(b, s, i, sc, cj);
      S.best[rl] = b; S.sec[rl] = s; S.idx[rl] = i;
      pend = false;
    }
    __syncthreads();
  }
  return qn - take;
}

// the five match fields of the item's rows and the pair's num_found
__device__ __forceinline__ void gm_write_rows(const GmArgs &A, GmLds &S, int p, bool active, int lane, SiftPointD *rows,
                                              const SiftPointD *rec2)
{
  __syncthreads();
  bool found = false;
  if (active) {
    SiftPointD &o = rows[lane];
    const float b = S.best[lane], s = S.sec[lane];
    const int i = S.idx[lane];
    found = i != 0x7fffffff;
    o.score = b;
    o.ambiguity = s / (b + 1e-6f);
    o.match = found ? i : -1;
    o.match_xpos = found ? rec2[i].xpos : 0.0f;
    o.match_ypos = found ? rec2[i].ypos : 0.0f;
  }
  const int nf = __popcll(__ballot(found));
  if (lane == 0 && nf > 0 && A.num_found) atomicAdd(&A.num_found[p], nf);
  __syncthreads();
}

__global__ __launch_bounds__(64) void guided_match_kernel(GmArgs A)
{
  __shared__ GmLds S;
  const int lane = threadIdx.x;
  const int nitems = A.item0[A.npairs];
  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    const int p = gm_item_pair(A, it);
    const GmPair P = A.pinfo[p];
    const GmGrid G = A.grid[P.d];
    const int r = (it - A.item0[p]) * 64 + lane;
    const bool active = r < P.n1;
    SiftPointD *rows = A.set1.recs + P.base1 + (it - A.item0[p]) * 64;
    const SiftPointD *rec2 = A.set2.recs + G.base2;
    const int *starts = A.starts + (size_t)P.d * GM_STARTS;
    const float4 *ent = A.entries + (size_t)P.d * A.max_pts;
    // projection, in MatchAll's order (mainSift.cpp:109-111), no contraction
    float px = 0.0f, py = 0.0f;
    if (active) {
      const float *h = A.H + 9 * (size_t)p;
      const float x = rows[lane].xpos, y = rows[lane].ypos;
      const float den = h[6] * x + h[7] * y + h[8];
      px = (h[0] * x + h[1] * y + h[2]) / den;
      py = (h[3] * x + h[4] * y + h[5]) / den;
    }
    // the cells of fl(px - r') .. fl(px + r') (an empty range for an inactive row or a non-finite projection)
    int cx0 = 0, cx1 = -1, cy = 0, cy1 = -1, pos = 0, end = 0;
    if (active && gm_disc(G, px, py, A.rp, cx0, cx1, cy, cy1)) {
      pos = starts[cy * G.gx + cx0];
      end = starts[cy * G.gx + cx1 + 1];
    }
    gm_reset_rows(S, lane);
    int qn = 0;
    const float r2 = A.r2;
    for (;;) {
      while (pos == end && cy < cy1) {
        cy++;
        pos = starts[cy * G.gx + cx0];
        end = starts[cy * G.gx + cx1 + 1];
      }
      const bool more = pos < end;
      if (!__any(more) && qn == 0) break;
      bool pass = false;
      int j = 0;
      if (more) {
        const float4 e = ent[pos++];
        const float ddx = px - e.x, ddy = py - e.y;
        pass = ddx * ddx + ddy * ddy < r2;
        j = __float_as_int(e.z);
      }
      qn = gm_enqueue(S, qn, pass, lane, j);
      const bool last = !__any(pos < end || cy < cy1);
      if (qn < 64 && !(last && qn > 0)) continue;
      qn = gm_score_merge(S, qn, lane, rows, rec2);
    }
    gm_write_rows(A, S, p, active, lane, rows, rec2);
  }
}

// ---- the epipolar gather (the header comment proves that it is conservative)

// the grid rows [cy0, cy1] that the band can reach over the box's u range (cy1 < cy0: none)
__host__ __device__ __forceinline__ void ep_rows(const GmGrid &G, const EpipolarBand &B, int &cy0, int &cy1)
{
  double lo = 0.0, hi = 0.0;
  const int k = epipolar_extent(B.binv, B.a, B.c, B.w, 0.0, G.x1 - G.x0, G.y1 - G.y0, lo, hi);
  cy0 = 0;
  cy1 = k == 0 ? -1 : G.gy - 1;
  if (k == 1) {
    cy0 = gm_cell(lo * G.iy, G.gy);
    cy1 = gm_cell(hi * G.iy, G.gy);
  }
}

// the cells [cx0, cx1] of grid row cy that the band can reach inside the row's slab (cx1 < cx0: none); ch = 1 / G.iy
__host__ __device__ __forceinline__ void ep_cols(const GmGrid &G, const EpipolarBand &B, double ch, int cy, int &cx0,
                                                 int &cx1)
{
  const double ry = G.y1 - G.y0;
  const double v0 = cy == 0 ? 0.0 : ((double)cy - 0x1p-20) * ch;
  const double v1 = cy == G.gy - 1 ? ry : fmin(((double)(cy + 1) + 0x1p-20) * ch, ry);
  double lo = 0.0, hi = 0.0;
  const int k = epipolar_extent(B.ainv, B.b, B.c, B.w, v0, v1, G.x1 - G.x0, lo, hi);
  cx0 = 0;
  cx1 = k == 0 ? -1 : G.gx - 1;
  if (k == 1) {
    cx0 = gm_cell(lo * G.ix, G.gx);
    cx1 = gm_cell(hi * G.ix, G.gx);
  }
}

__host__ __device__ __forceinline__ EpipolarBand ep_band(const GmGrid &G, const EpipolarLine &L, double rp)
{
  return epipolar_band(L, rp, G.x0, G.y0, fmax(fabs(G.x0), fabs(G.x1)), fmax(fabs(G.y0), fabs(G.y1)));
}

// a row walks its band only if its line can have a candidate at all
__host__ __device__ __forceinline__ bool ep_walks(const EpipolarLine &L) { return epipolar_line_ok(L) && L.n2 > 0.0f; }

__global__ __launch_bounds__(64) void epipolar_match_kernel(GmArgs A)
{
  __shared__ GmLds S;
  const int lane = threadIdx.x;
  const int nitems = A.item0[A.npairs];
  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    const int p = gm_item_pair(A, it);
    const GmPair P = A.pinfo[p];
    const GmGrid G = A.grid[P.d];
    const int r = (it - A.item0[p]) * 64 + lane;
    const bool active = r < P.n1;
    SiftPointD *rows = A.set1.recs + P.base1 + (it - A.item0[p]) * 64;
    const SiftPointD *rec2 = A.set2.recs + G.base2;
    const int *starts = A.starts + (size_t)P.d * GM_STARTS;
    const float4 *ent = A.entries + (size_t)P.d * A.max_pts;
    const double ch = 1.0 / G.iy;
    EpipolarLine L = {0.0f, 0.0f, 0.0f, 0.0f};
    if (active) L = epipolar_line(A.H + 9 * (size_t)p, rows[lane].xpos, rows[lane].ypos);
    const EpipolarBand B = ep_band(G, L, A.rp);
    // before the first row of the band: the loop below steps into it (no row for an inactive lane or a dead line)
    int cy = 0, cy1 = -1, pos = 0, end = 0;
    if (active && ep_walks(L)) {
      ep_rows(G, B, cy, cy1);
      cy--;
    }
    gm_reset_rows(S, lane);
    int qn = 0;
    const float r2 = A.r2;
    for (;;) {
      while (pos == end && cy < cy1) {
        cy++;
        int cx0, cx1;
        ep_cols(G, B, ch, cy, cx0, cx1);
        if (cx0 <= cx1) {
          pos = starts[cy * G.gx + cx0];
          end = starts[cy * G.gx + cx1 + 1];
        }
      }
      const bool more = pos < end;
      if (!__any(more) && qn == 0) break;
      bool pass = false;
      int j = 0;
      if (more) {
        const float4 e = ent[pos++];
        pass = epipolar_gate(L, e.x, e.y, r2);
        j = __float_as_int(e.z);
      }
      qn = gm_enqueue(S, qn, pass, lane, j);
      const bool last = !__any(pos < end || cy < cy1);
      if (qn < 64 && !(last && qn > 0)) continue;
      qn = gm_score_merge(S, qn, lane, rows, rec2);
    }
    gm_write_rows(A, S, p, active, lane, rows, rec2);
  }
}

size_t align16(size_t v) { return (v + 15) / 16 * 16; }

}  // namespace

size_t match_guided_batch_tmp_bytes(int npairs, int nd, int max_pts)
{
  return align16(sizeof(int) * ((size_t)npairs + 1)) + sizeof(GmPair) * (size_t)npairs + sizeof(GmGrid) * (size_t)nd +
         sizeof(int) * GM_STARTS * (size_t)nd + sizeof(float4) * (size_t)nd * (size_t)max_pts;
}

// both calls: M = the homographies (epipolar false) or the fundamental matrices (true)
static int launch_gm(misift_ctx *ctx, bool epipolar, int npairs, const int *h_pairs, const int *h_pair_d,
                     const int *h_distinct, int nd, const BatchLayout &set1, const BatchLayout &set2, const float *M,
                     float radius, int max_pts, int *num_found)
{
  int rc = misift_ensure_tmp(ctx, match_guided_batch_tmp_bytes(npairs, nd, max_pts));
  if (rc) return rc;
  GmArgs A;
  A.set1 = set1; A.set2 = set2;
  A.pairs = h_pairs; A.pair_d = h_pair_d; A.distinct = h_distinct;
  A.npairs = npairs; A.nd = nd; A.max_pts = max_pts;
  A.rp = (double)radius * (1.0 + 1.0 / 1024) + 1e-20;
  A.r2 = radius * radius;
  A.H = M; A.num_found = num_found;
  char *t = reinterpret_cast<char *>(ctx->d_match_tmp);
  A.item0 = reinterpret_cast<int *>(t);
  t += align16(sizeof(int) * ((size_t)npairs + 1));
  A.pinfo = reinterpret_cast<GmPair *>(t);
  t += sizeof(GmPair) * (size_t)npairs;
  A.grid = reinterpret_cast<GmGrid *>(t);
  t += sizeof(GmGrid) * (size_t)nd;
  A.starts = reinterpret_cast<int *>(t);
  t += sizeof(int) * GM_STARTS * (size_t)nd;
  A.entries = reinterpret_cast<float4 *>(t);
  {
    LaunchScope ls(ctx, "guided_bin");
    hipLaunchKernelGGL(guided_bin_kernel, dim3(nd + 1), dim3(1024), 0, ctx->stream, A);
    rc = ls.finish();
    if (rc) return rc;
  }
  // items: at most npairs x ceil(max_pts / 64), known here; the grid strides over the device's count
  const long long bound = (long long)npairs * ((max_pts + 63) / 64);
  const long long cap = (long long)GM_ITEMS_PER_CU * (ctx->num_cus > 0 ? ctx->num_cus : 256);
  const int grid = (int)(bound < cap ? bound : cap);
  LaunchScope ls(ctx, epipolar ? "epipolar_match" : "guided_match");
  if (epipolar) hipLaunchKernelGGL(epipolar_match_kernel, dim3(grid), dim3(64), 0, ctx->stream, A);
  else hipLaunchKernelGGL(guided_match_kernel, dim3(grid), dim3(64), 0, ctx->stream, A);
  return ls.finish();
}

int launch_match_guided_batch(misift_ctx *ctx, int npairs, const int *h_pairs, const int *h_pair_d,
                              const int *h_distinct, int nd, const BatchLayout &set1, const BatchLayout &set2,
                              const float *H, float radius, int max_pts, int *num_found)
{
  return launch_gm(ctx, false, npairs, h_pairs, h_pair_d, h_distinct, nd, set1, set2, H, radius, max_pts, num_found);
}

int launch_match_epipolar_batch(misift_ctx *ctx, int npairs, const int *h_pairs, const int *h_pair_d,
                                const int *h_distinct, int nd, const BatchLayout &set1, const BatchLayout &set2,
                                const float *F, float radius, int max_pts, int *num_found)
{
  return launch_gm(ctx, true, npairs, h_pairs, h_pair_d, h_distinct, nd, set1, set2, F, radius, max_pts, num_found);
}

// Test-only, host-only: the gate and the gather of misift_match_guided_batch as the device runs them (gm_make_grid,
// gm_cell, gm_disc; the gate is the match kernel's, operation by operation).
extern "C" int misift_test_guided_gather(const float *H9, const float *xy1, int n1, const float *xy2, int n2,
                                         float radius, unsigned char *pass, unsigned char *visited, int *grid2)
{
  if (!H9 || n1 < 0 || n2 < 0 || (n1 > 0 && !xy1) || (n2 > 0 && !xy2) ||
      (n1 > 0 && n2 > 0 && (!pass || !visited)) || !grid2 || !(radius > 0.0f)) {
    misift_set_error("misift_test_guided_gather: invalid argument");
    return MISIFT_EINVAL;
  }
  // the bin: bounding box of the finite positions, the grid, each record's cell (-1: left out)
  float xmin = INFINITY, ymin = INFINITY, xmax = -INFINITY, ymax = -INFINITY;
  for (int j = 0; j < n2; j++) {
    const float x = xy2[2 * j], y = xy2[2 * j + 1];
    if (gm_finite(x) && gm_finite(y)) {
      xmin = fminf(xmin, x); xmax = fmaxf(xmax, x);
      ymin = fminf(ymin, y); ymax = fmaxf(ymax, y);
    }
  }
  const double rp = (double)radius * (1.0 + 1.0 / 1024) + 1e-20;
  const float r2 = radius * radius;
  const GmGrid G = gm_make_grid(xmin, xmax, ymin, ymax, rp, 0);
  grid2[0] = G.gx;
  grid2[1] = G.gy;
  std::vector<int> ccx((size_t)n2, -1), ccy((size_t)n2, -1);
  for (int j = 0; j < n2; j++) {
    const float x = xy2[2 * j], y = xy2[2 * j + 1];
    if (gm_finite(x) && gm_finite(y)) {
      ccx[j] = gm_cell(((double)x - G.x0) * G.ix, G.gx);
      ccy[j] = gm_cell(((double)y - G.y0) * G.iy, G.gy);
    }
  }
  for (int i = 0; i < n1; i++) {
    // projection, in MatchAll's order, no contraction
    const float x = xy1[2 * i], y = xy1[2 * i + 1];
    const float den = H9[6] * x + H9[7] * y + H9[8];
    const float px = (H9[0] * x + H9[1] * y + H9[2]) / den;
    const float py = (H9[3] * x + H9[4] * y + H9[5]) / den;
    int cx0, cx1, cy0, cy1;
    gm_disc(G, px, py, rp, cx0, cx1, cy0, cy1);
    for (int j = 0; j < n2; j++) {
      const float ddx = px - xy2[2 * j], ddy = py - xy2[2 * j + 1];
      pass[(size_t)i * n2 + j] = ddx * ddx + ddy * ddy < r2 ? 1 : 0;
      visited[(size_t)i * n2 + j] = ccx[j] >= cx0 && ccx[j] <= cx1 && ccy[j] >= cy0 && ccy[j] <= cy1 ? 1 : 0;
    }
  }
  return MISIFT_OK;
}

// Test-only, host-only: the gate and the gather of misift_match_epipolar_batch as the device runs them
// (epipolar_core.hpp, gm_make_grid, ep_rows / ep_cols).
extern "C" int misift_test_epipolar_gate(const float *F9, const float *xy1, int n1, const float *xy2, int n2,
                                         float radius, unsigned char *pass)
{
  if (!F9 || n1 < 0 || n2 < 0 || (n1 > 0 && !xy1) || (n2 > 0 && !xy2) || (n1 > 0 && n2 > 0 && !pass)) {
    misift_set_error("misift_test_epipolar_gate: invalid argument");
    return MISIFT_EINVAL;
  }
  const float r2 = radius * radius;
  for (int i = 0; i < n1; i++) {
    const EpipolarLine L = epipolar_line(F9, xy1[2 * i], xy1[2 * i + 1]);
    const bool ok = epipolar_line_ok(L);
    for (int j = 0; j < n2; j++)
      pass[(size_t)i * n2 + j] = ok && epipolar_gate(L, xy2[2 * j], xy2[2 * j + 1], r2) ? 1 : 0;
  }
  return MISIFT_OK;
}

extern "C" int misift_test_epipolar_gather(const float *F9, const float *xy1, int n1, const float *xy2, int n2,
                                           float radius, unsigned char *visited, int *grid2)
{
  if (!F9 || n1 < 0 || n2 < 0 || (n1 > 0 && !xy1) || (n2 > 0 && !xy2) || (n1 > 0 && n2 > 0 && !visited) || !grid2 ||
      !(radius > 0.0f)) {
    misift_set_error("misift_test_epipolar_gather: invalid argument");
    return MISIFT_EINVAL;
  }
  // the bin: bounding box of the finite positions, the grid, each record's cell (-1: left out)
  float xmin = INFINITY, ymin = INFINITY, xmax = -INFINITY, ymax = -INFINITY;
  for (int j = 0; j < n2; j++) {
    const float x = xy2[2 * j], y = xy2[2 * j + 1];
    if (epipolar_finite(x) && epipolar_finite(y)) {
      xmin = fminf(xmin, x); xmax = fmaxf(xmax, x);
      ymin = fminf(ymin, y); ymax = fmaxf(ymax, y);
    }
  }
  const double rp = (double)radius * (1.0 + 1.0 / 1024) + 1e-20;
  const GmGrid G = gm_make_grid(xmin, xmax, ymin, ymax, rp, 0);
  grid2[0] = G.gx;
  grid2[1] = G.gy;
  std::vector<int> cell((size_t)n2, -1);
  for (int j = 0; j < n2; j++) {
    const float x = xy2[2 * j], y = xy2[2 * j + 1];
    if (epipolar_finite(x) && epipolar_finite(y))
      cell[j] = gm_cell(((double)y - G.y0) * G.iy, G.gy) * G.gx + gm_cell(((double)x - G.x0) * G.ix, G.gx);
  }
  // the walk of every row: the cells it visits
  const double ch = 1.0 / G.iy;
  std::vector<unsigned char> seen((size_t)G.gx * G.gy);
  for (int i = 0; i < n1; i++) {
    std::fill(seen.begin(), seen.end(), 0);
    const EpipolarLine L = epipolar_line(F9, xy1[2 * i], xy1[2 * i + 1]);
    if (ep_walks(L)) {
      const EpipolarBand B = ep_band(G, L, rp);
      int cy0, cy1;
      ep_rows(G, B, cy0, cy1);
      for (int cy = cy0; cy <= cy1; cy++) {
        int cx0, cx1;
        ep_cols(G, B, ch, cy, cx0, cx1);
        for (int cx = cx0; cx <= cx1; cx++) seen[(size_t)cy * G.gx + cx] = 1;
      }
    }
    for (int j = 0; j < n2; j++) visited[(size_t)i * n2 + j] = cell[j] >= 0 ? seen[cell[j]] : 0;
  }
  return MISIFT_OK;
}

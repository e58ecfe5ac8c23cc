// kernels_guided.hip — homography-guided matching of many frame pairs of a device-resident batch
// (misift_match_guided_batch).
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
#include "common.hpp"

namespace {

constexpr int GM_GRID = 64;                         // cells per axis at most
constexpr int GM_STARTS = GM_GRID * GM_GRID + 4;    // cell starts per frame (4096 + 1, rounded up to 16 bytes)
constexpr int GM_ITEMS_PER_CU = 16;                 // one-wave workgroups per CU of the match grid

struct GmGrid {                  // one per distinct set-2 frame, written by the bin kernel
  double x0, y0, ix, iy;         // cell of (x, y): gm_cell((x - x0) * ix, gx), gm_cell((y - y0) * iy, gy)
  long long base2;               // first record of the frame
  int gx, gy;
  int pad[4];
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
  const float *H;                // npairs x 9
  int *num_found;                // npairs, or NULL
  // temp
  int *item0;                    // npairs + 1: first item of each pair, item0[npairs] = items in all
  GmPair *pinfo;
  GmGrid *grid;
  int *starts;                   // nd x GM_STARTS
  float4 *entries;               // nd x max_pts: (x2, y2, j as int bits, 0)
};

__device__ __forceinline__ int gm_cell(double v, int g)
{
  return v >= (double)(g - 1) ? g - 1 : (v > 0.0 ? (int)v : 0);   // NaN -> 0; (int) of a positive v is its floor
}

__device__ __forceinline__ bool gm_finite(float v) { return __builtin_isfinite(v); }

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
    GmGrid G;
    const bool any = s_red[0][0] <= s_red[1][0];
    G.x0 = any ? (double)s_red[0][0] : 0.0;
    G.y0 = any ? (double)s_red[2][0] : 0.0;
    const double rx = any ? (double)s_red[1][0] - G.x0 : 0.0, ry = any ? (double)s_red[3][0] - G.y0 : 0.0;
    const double cw = fmax(rx / GM_GRID, A.rp), ch = fmax(ry / GM_GRID, A.rp);   // > 0: r' > 0
    G.gx = min(GM_GRID, (int)(rx / cw) + 1);
    G.gy = min(GM_GRID, (int)(ry / ch) + 1);
    G.ix = 1.0 / cw;                                                               // r' = inf: 0, one cell
    G.iy = 1.0 / ch;
    G.base2 = base2;
    G.pad[0] = G.pad[1] = G.pad[2] = G.pad[3] = 0;
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

__global__ __launch_bounds__(64) void guided_match_kernel(GmArgs A)
{
  __shared__ int q_row[128], q_j[128];               // queue of (row lane, candidate) pairs, < 128 between batches
  __shared__ float s_best[64], s_sec[64];
  __shared__ int s_idx[64], s_own[64];
  const int lane = threadIdx.x;
  const int nitems = A.item0[A.npairs];
  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    int lo = 0, hi = A.npairs - 1;                   // the last pair whose first item is <= it
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (A.item0[mid] <= it) lo = mid; else hi = mid - 1;
    }
    const int p = lo;
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
    if (active && gm_finite(px) && gm_finite(py)) {
      const double dx = (double)px, dy = (double)py;
      cx0 = gm_cell((dx - A.rp - G.x0) * G.ix, G.gx);
      cx1 = gm_cell((dx + A.rp - G.x0) * G.ix, G.gx);
      cy = gm_cell((dy - A.rp - G.y0) * G.iy, G.gy);
      cy1 = gm_cell((dy + A.rp - G.y0) * G.iy, G.gy);
      pos = starts[cy * G.gx + cx0];
      end = starts[cy * G.gx + cx1 + 1];
    }
    s_best[lane] = 0.0f; s_sec[lane] = 0.0f; s_idx[lane] = 0x7fffffff;
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
      const unsigned long long m = __ballot(pass);
      if (pass) {
        const int k = qn + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        q_row[k] = lane;
        q_j[k] = j;
      }
      qn += __popcll(m);
      const bool last = !__any(pos < end || cy < cy1);
      if (qn < 64 && !(last && qn > 0)) continue;
      // score 64 queued pairs (fewer at the end), one per lane
      __syncthreads();
      const int take = min(qn, 64);
      int rl = 0, cj = 0;
      float sc = 0.0f;
      if (lane < take) {
        rl = q_row[lane];
        cj = q_j[lane];
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
      if (lane + 64 < qn) { q_row[lane] = q_row[lane + 64]; q_j[lane] = q_j[lane + 64]; }
      qn -= take;
      // each round one writer per row: the last lane to claim it
      while (__any(pend)) {
        if (pend) s_own[rl] = lane;
        __syncthreads();
        if (pend && s_own[rl] == lane) {
          float b = s_best[rl], s = s_sec[rl];
          int i = s_idx[rl];
          gm_merge(b, s, i, sc, cj);
          s_best[rl] = b; s_sec[rl] = s; s_idx[rl] = i;
          pend = false;
        }
        __syncthreads();
      }
    }
    __syncthreads();
    bool found = false;
    if (active) {
      SiftPointD &o = rows[lane];
      const float b = s_best[lane], s = s_sec[lane];
      const int i = s_idx[lane];
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
}

size_t align16(size_t v) { return (v + 15) / 16 * 16; }

}  // namespace

size_t match_guided_batch_tmp_bytes(int npairs, int nd, int max_pts)
{
  return align16(sizeof(int) * ((size_t)npairs + 1)) + sizeof(GmPair) * (size_t)npairs + sizeof(GmGrid) * (size_t)nd +
         sizeof(int) * GM_STARTS * (size_t)nd + sizeof(float4) * (size_t)nd * (size_t)max_pts;
}

int launch_match_guided_batch(misift_ctx *ctx, int npairs, const int *h_pairs, const int *h_pair_d,
                              const int *h_distinct, int nd, const BatchLayout &set1, const BatchLayout &set2,
                              const float *H, float radius, int max_pts, int *num_found)
{
  int rc = misift_ensure_tmp(ctx, match_guided_batch_tmp_bytes(npairs, nd, max_pts));
  if (rc) return rc;
  GmArgs A;
  A.set1 = set1; A.set2 = set2;
  A.pairs = h_pairs; A.pair_d = h_pair_d; A.distinct = h_distinct;
  A.npairs = npairs; A.nd = nd; A.max_pts = max_pts;
  A.rp = (double)radius * (1.0 + 1.0 / 1024) + 1e-20;
  A.r2 = radius * radius;
  A.H = H; A.num_found = num_found;
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
  LaunchScope ls(ctx, "guided_match");
  hipLaunchKernelGGL(guided_match_kernel, dim3(grid), dim3(64), 0, ctx->stream, A);
  return ls.finish();
}

// kernels_match_i8.hip — 8-bit descriptors and brute-force matching of many frame pairs on the int8 matrix cores of gfx950
// (misift_quantize_batch, misift_match_batch_i8).
//
// quantize_i8_kernel   one launch: q[r] = quantize_i8(data of record r) (quantize_i8.hpp), 128 bytes at d_q + 128 r, for
//                      every record of every frame; eight lanes per record, 16 bytes each.
// pair_plan_kernel     the work list of misift_match_batch (pair_plan.hpp), here with 128-row blocks and 32-column tiles
//                      and every column taking part.
// match_i8_kernel      persistent grid, two waves per workgroup, 64 rows per wave (128-row blocks).  A wave keeps its
//                      rows' q in VGPRs (two 32-row A tiles x 128 bytes) and sweeps 32-column tiles of set 2, loaded
//                      straight from global memory one tile ahead: per tile 2 x 4 v_mfma_i32_32x32x32_i8 give the exact
//                      int32 scores of 64 rows x 32 columns.  Each lane keeps, per row register, the top two of the packed
//                      keys  key = S * 512 + 2^30 + (511 - t)  (t = the tile within a window of 512 tiles), unsigned:
//                          b2 = med3(b1, b2, key),  b1 = max(b1, key)       — 3 VALU ops per score, v_lshl_add + v_med3 +
//                      v_max.  |S| <= 128 * 128^2 = 2^21, so keys stay in [0, 2^31 + 511]; a key encodes S > 0 iff it is
//                      >= 2^30 + 512, and for equal S the earlier tile (the smaller column of that lane) is the larger key.
//                      At the end of a window the lanes' keys go through LDS to one lane per row, which decodes them into
//                      (score, frame-local column) and merges them under "score descending, column ascending".
//                      With one column chunk per row block the wave writes its rows; otherwise it stores (best, index,
//                      second) per row and chunk, and
// match_i8_merge_kernel merges them over the chunks (it returns at once when nothing was chunked).
// Columns are cut into chunks only when the row blocks of the call do not fill I8_TARGET_ROUNDS rounds of the grid.
//
// The A and B fragments of the i8 MFMA are loaded by the same code (lane l: row / column l & 31, bytes 64 (l >> 5) + 16 s
// of k-step s), so the sum over k is right whatever order the hardware pairs the bytes of one k-step in; integer sums do
// not depend on order.
#include <stdint.h>
#include "common.hpp"
#include "pair_plan.hpp"
#include "quantize_i8.hpp"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int I8_WAVES = 2;                      // waves per workgroup
constexpr int I8_ROWS = 64 * I8_WAVES;           // rows per work item
constexpr int I8_TILE = 32;                      // columns per tile
constexpr int I8_WIN = 512;                      // tiles per key window (9 bits of the key)
constexpr unsigned I8_OFF = 1u << 30;            // key of S = 0, t = 511
constexpr unsigned I8_VALID = I8_OFF + 512u;     // smallest key with S >= 1
constexpr int I8_WG_PER_CU = 4;                  // workgroups per CU of the persistent grid (8 waves)
constexpr int I8_TARGET_ROUNDS = 4;              // items a call is cut into when its row blocks are few, in grid rounds

struct I8Args {
  SiftPointD *recs1;
  const SiftPointD *recs2;
  const int8_t *q1, *q2;
  const int *hdr;
  const PairPlan *plan;
  int npairs;
  int4 *partial;                 // items x I8_ROWS x (best, index, second, 0), chunked calls only
};

__host__ __device__ __forceinline__ int i8_grid(int ncu) { return I8_WG_PER_CU * (ncu > 0 ? ncu : 256); }
// the plan's shape: 128-row blocks, 32-column tiles, every column
PairShape i8_shape(int ncu)
{
  return PairShape{I8_ROWS, I8_TILE, 1, I8_TARGET_ROUNDS * i8_grid(ncu)};
}

// (m, i, s) <- the top two of (m, i, s) and (mo, io, so): score descending, index ascending; a tie of the best scores
// makes the loser's score the runner-up.  "None" is (0, -1, 0); real entries have m > 0.
__device__ __forceinline__ void i8_take(int &m, int &i, int &s, int mo, int io, int so)
{
  const bool take = mo > m || (mo == m && (unsigned)io < (unsigned)i);
  const int ns = take ? max(so, m) : max(s, mo);
  if (take) { m = mo; i = io; }
  s = ns;
}

__device__ __forceinline__ void i8_write_row(SiftPointD *o, const SiftPointD *set2, int m, int i, int s)
{
  const float score = (float)m * 0x1p-16f;               // exact: m < 2^22
  o->score = score;
  o->match = i;
  o->match_xpos = i >= 0 ? set2[i].xpos : 0.0f;
  o->match_ypos = i >= 0 ? set2[i].ypos : 0.0f;
  o->ambiguity = ((float)s * 0x1p-16f) / (score + 1e-6f);
}

__device__ __forceinline__ unsigned i8_pack4(float4 v)
{
  return (unsigned)(uint8_t)quantize_i8(v.x) | (unsigned)(uint8_t)quantize_i8(v.y) << 8 |
         (unsigned)(uint8_t)quantize_i8(v.z) << 16 | (unsigned)(uint8_t)quantize_i8(v.w) << 24;
}

}  // namespace

__global__ __launch_bounds__(256) void quantize_i8_kernel(BatchLayout set, int nframes, int8_t *__restrict__ q)
{
  const SiftPointD *__restrict__ recs = set.recs;
  const int sub = threadIdx.x & 7;
  for (int f = blockIdx.y; f < nframes; f += gridDim.y) {
    const int n = max(set.counts[f], 0);
    const long long base = set.base(f);
    for (int r = blockIdx.x * 32 + (threadIdx.x >> 3); r < n; r += gridDim.x * 32) {
      const float4 *src = reinterpret_cast<const float4 *>(recs[base + r].data) + 4 * sub;
      int4 w;
      w.x = (int)i8_pack4(src[0]);
      w.y = (int)i8_pack4(src[1]);
      w.z = (int)i8_pack4(src[2]);
      w.w = (int)i8_pack4(src[3]);
      reinterpret_cast<int4 *>(q + (base + r) * 128)[sub] = w;
    }
  }
}

// recs1 / recs2 may be the same array, and q1 / q2 too: the kernel reads q and set 2's xpos / ypos, and writes only the
// five match fields of set-1 rows.
__global__ __launch_bounds__(64 * I8_WAVES) void match_i8_kernel(I8Args A)
{
  __shared__ uint2 red[I8_WAVES][32][64];        // per wave: (b1, b2) of row register rr of lane l at [rr][l]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int nitems = A.hdr[0], C = A.hdr[1];
  // the row this lane owns in the fold and the output: row register c & 15 of A tile c >> 4, lane half h
  const int own = 32 * (c >> 4) + (c & 3) + 8 * ((c & 15) >> 2) + 4 * h;
  for (int it = (int)xcd_remap(blockIdx.x, gridDim.x); it < nitems; it += gridDim.x) {
    PairPlan P = A.plan[pair_find<false>(A.plan, A.npairs, it)];
    // wave-uniform: keep the loop bounds and the key constant in SGPRs
    P.n1 = __builtin_amdgcn_readfirstlane(P.n1); P.n2 = __builtin_amdgcn_readfirstlane(P.n2);
    P.off1 = __builtin_amdgcn_readfirstlane(P.off1); P.off2 = __builtin_amdgcn_readfirstlane(P.off2);
    P.ntiles = __builtin_amdgcn_readfirstlane(P.ntiles); P.nchunks = __builtin_amdgcn_readfirstlane(P.nchunks);
    P.tpc = __builtin_amdgcn_readfirstlane(P.tpc); P.item0 = __builtin_amdgcn_readfirstlane(P.item0);
    const int local = it - P.item0, rb = local / P.nchunks, chunk = local - rb * P.nchunks;
    const int t0 = chunk * P.tpc, t1 = min(t0 + P.tpc, P.ntiles);
    const int row0 = rb * I8_ROWS + wave * 64;
    v4i a[2][4];
#pragma unroll
    for (int ai = 0; ai < 2; ai++) {
      const int row = row0 + 32 * ai + c;
      if (row < P.n1) {
        const v4i *p = reinterpret_cast<const v4i *>(A.q1 + ((size_t)P.off1 + row) * 128 + 64 * h);
#pragma unroll
        for (int s = 0; s < 4; s++) a[ai][s] = p[s];
      } else {
#pragma unroll
        for (int s = 0; s < 4; s++) a[ai][s] = (v4i){0, 0, 0, 0};
      }
    }
    const int8_t *q2 = A.q2 + (size_t)P.off2 * 128 + 64 * h;
    int M = 0, I = -1, S2 = 0;
    for (int w0 = t0; w0 < t1; w0 += I8_WIN) {
      const int w1 = min(w0 + I8_WIN, t1);
      unsigned b1[2][16], b2[2][16];
#pragma unroll
      for (int ai = 0; ai < 2; ai++)
#pragma unroll
        for (int r = 0; r < 16; r++) { b1[ai][r] = 0u; b2[ai][r] = 0u; }
      // set-2 tiles ping-pong between two register sets, each loaded one tile ahead of its use.  Only the pair's last
      // tile can be partial: it runs on its own after the loop, its lanes past the last column zeroed (S = 0 never counts).
      v4i bA[4], bB[4];
      auto load = [&](v4i (&b)[4], int t) {
        const v4i *p = reinterpret_cast<const v4i *>(q2 + (size_t)(t * I8_TILE + c) * 128);
#pragma unroll
        for (int s = 0; s < 4; s++) b[s] = p[s];
      };
      auto tile = [&](v4i (&b)[4], int t) {
        v16i acc0 = {}, acc1 = {};
#pragma unroll
        for (int s = 0; s < 4; s++) {
          acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[0][s], b[s], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[1][s], b[s], acc1, 0, 0, 0);
        }
        const unsigned kc = __builtin_amdgcn_readfirstlane(I8_OFF + (unsigned)(I8_WIN - 1 - (t - w0)));
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const unsigned k0 = ((unsigned)acc0[r] << 9) + kc, k1 = ((unsigned)acc1[r] << 9) + kc;
          b2[0][r] = max(min(b1[0][r], b2[0][r]), min(max(b1[0][r], b2[0][r]), k0));
          b1[0][r] = max(b1[0][r], k0);
          b2[1][r] = max(min(b1[1][r], b2[1][r]), min(max(b1[1][r], b2[1][r]), k1));
          b1[1][r] = max(b1[1][r], k1);
        }
      };
      const int wf = min(w1, P.n2 / I8_TILE);             // tiles [w0, wf) are full
      if (w0 < wf) load(bA, w0);
      for (int t = w0; t < wf; t += 2) {           // unconditional loads (the last ones repeat tile wf - 1): static vmcnt
        load(bB, min(t + 1, wf - 1));
        tile(bA, t);
        if (t + 1 >= wf) break;
        load(bA, min(t + 2, wf - 1));
        tile(bB, t + 1);
      }
      if (wf < w1) {
        const bool live = wf * I8_TILE + c < P.n2;
        if (live) load(bA, wf);
        else {
#pragma unroll
          for (int s = 0; s < 4; s++) bA[s] = (v4i){0, 0, 0, 0};
        }
        tile(bA, wf);
      }
      // fold the window: lane (c, h) reads row register c of the 32 lanes of its half
#pragma unroll
      for (int ai = 0; ai < 2; ai++)
#pragma unroll
        for (int r = 0; r < 16; r++) red[wave][16 * ai + r][lane] = make_uint2(b1[ai][r], b2[ai][r]);
      __syncthreads();
      for (int l = 0; l < 32; l++) {
        const uint2 e = red[wave][c][32 * h + l];
        const bool v1 = e.x >= I8_VALID;
        const int s1 = v1 ? (int)((e.x - I8_OFF) >> 9) : 0;
        const int j1 = v1 ? (w0 + I8_WIN - 1 - (int)(e.x & (I8_WIN - 1))) * I8_TILE + l : -1;
        const int s2 = e.y >= I8_VALID ? (int)((e.y - I8_OFF) >> 9) : 0;
        i8_take(M, I, S2, s1, j1, s2);
      }
      __syncthreads();                           // red is rewritten by the next window / item
    }
    const int row = row0 + own;
    if (row < P.n1) {
      if (C == 1) i8_write_row(A.recs1 + P.off1 + row, A.recs2 + P.off2, M, I, S2);
      else A.partial[(size_t)it * I8_ROWS + wave * 64 + own] = make_int4(M, I, S2, 0);
    }
  }
}

// Chunked calls only: one thread per row of a row block merges the row over the pair's chunks.
__global__ __launch_bounds__(I8_ROWS) void match_i8_merge_kernel(I8Args A)
{
  if (A.hdr[1] <= 1) return;
  const int nrbs = A.hdr[2];
  for (int g = blockIdx.x; g < nrbs; g += gridDim.x) {
    const PairPlan P = A.plan[pair_find<true>(A.plan, A.npairs, g)];
    const int rb = g - P.rb0, row = rb * I8_ROWS + threadIdx.x;
    if (row >= P.n1) continue;
    int M = 0, I = -1, S2 = 0;
    const int4 *q = A.partial + (size_t)(P.item0 + rb * P.nchunks) * I8_ROWS + threadIdx.x;
    for (int ch = 0; ch < P.nchunks; ch++, q += I8_ROWS) {
      const int4 v = *q;
      i8_take(M, I, S2, v.x, v.y, v.z);
    }
    i8_write_row(A.recs1 + P.off1 + row, A.recs2 + P.off2, M, I, S2);
  }
}

// host-only test hook: the quantisation rule the kernel applies
extern "C" int misift_test_quantize(const float *src, long n, int8_t *dst)
{
  if (n < 0 || (n > 0 && (!src || !dst))) return MISIFT_EINVAL;
  for (long i = 0; i < n; i++) dst[i] = quantize_i8(src[i]);
  return MISIFT_OK;
}

// host-only test hook (no device needed): the plan misift_match_batch_i8 makes for pairs of n1[i] x n2[i] records on a
// chip of num_cus CUs (pair_plan_host; tiles are 32 columns)
extern "C" int misift_test_match_i8_plan(int num_cus, int npairs, const int *n1, const int *n2, int *plan5, int *nitems,
                                         int *chunks, int *partial_items_bound)
{
  return pair_plan_host(i8_shape(num_cus), npairs, n1, n2, plan5, nitems, chunks, partial_items_bound);
}

int launch_quantize_batch(misift_ctx *ctx, const BatchLayout &set, int nframes, int8_t *q)
{
  if (nframes <= 0) return MISIFT_OK;
  // counts live on the device: enough workgroups per frame to cover the largest frame of a big call in a few strides
  const int ncu = ctx->num_cus > 0 ? ctx->num_cus : 256;
  const int gy = nframes < 65535 ? nframes : 65535;
  int gx = 8 * ncu / gy;
  gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
  LaunchScope ls(ctx, "quantize_i8");
  hipLaunchKernelGGL(quantize_i8_kernel, dim3(gx, gy), dim3(256), 0, ctx->stream, set, nframes, q);
  return ls.finish();
}

int launch_match_batch_i8(misift_ctx *ctx, int npairs, const int *h_pairs, void *d_plan, const BatchLayout &set1,
                          const int8_t *q1, const BatchLayout &set2, const int8_t *q2)
{
  if (npairs <= 0) return MISIFT_OK;
  const PairShape S = i8_shape(ctx->num_cus);
  int rc = misift_ensure_tmp(ctx, (size_t)pair_partial_items(S) * I8_ROWS * sizeof(int4));
  if (rc) return rc;
  rc = launch_pair_plan(ctx, "match_i8_plan", S, npairs, h_pairs, set1, set2, d_plan);
  if (rc) return rc;
  I8Args A;
  A.recs1 = set1.recs; A.recs2 = set2.recs; A.q1 = q1; A.q2 = q2;
  A.hdr = reinterpret_cast<const int *>(d_plan);
  A.plan = reinterpret_cast<const PairPlan *>(A.hdr + PAIR_HDR_INTS);
  A.npairs = npairs;
  A.partial = reinterpret_cast<int4 *>(ctx->d_match_tmp);
  const int grid = i8_grid(ctx->num_cus);
  {
    LaunchScope ls(ctx, "match_i8_mfma");
    hipLaunchKernelGGL(match_i8_kernel, dim3(grid), dim3(64 * I8_WAVES), 0, ctx->stream, A);
    rc = ls.finish();
    if (rc) return rc;
  }
  LaunchScope ls(ctx, "match_i8_merge");
  hipLaunchKernelGGL(match_i8_merge_kernel, dim3(grid), dim3(I8_ROWS), 0, ctx->stream, A);
  return ls.finish();
}

// kernels_match_i8.hip — 8-bit descriptors and brute-force matching of many frame pairs on the int8 matrix cores of gfx950
// (misift_quantize_batch, misift_match_batch_i8, misift_match_pairs_batch_i8).
//
// quantize_i8_kernel   one launch: q[r] = quantize_i8(data of record r) (quantize_i8.hpp), 128 bytes at d_q + 128 r, for
//                      every record of every frame; eight lanes per record, 16 bytes each.
// pair_plan_kernel     the work list of misift_match_batch (pair_plan.hpp), here with 128-row blocks and 32-column tiles
//                      and every column taking part; pair-indexed calls run pair_plan_capped_kernel (oversized pairs get
//                      no work), and mutual ones then set the column keys of every (pair, column) to 0.
// match_i8_kernel<MODE> persistent grid, two waves per workgroup, 64 rows per wave (128-row blocks).  A wave keeps its
//                      rows' q in VGPRs (two 32-row A tiles x 128 bytes) and sweeps 32-column tiles of set 2, loaded
//                      straight from global memory one tile ahead: per tile 2 x 4 v_mfma_i32_32x32x32_i8 give the exact
//                      int32 scores of 64 rows x 32 columns.  Each lane keeps, per row register, the top two of the packed
//                      keys  key = S * 512 + 2^30 + (511 - t)  (t = the tile within a window of 512 tiles), unsigned:
//                          b2 = med3(b1, b2, key),  b1 = max(b1, key)       — 3 VALU ops per score, v_lshl_add + v_med3 +
//                      v_max.  |S| <= 128 * 128^2 = 2^21, so keys stay in [0, 2^31 + 511]; a key encodes S > 0 iff it is
//                      >= 2^30 + 512, and for equal S the earlier tile (the smaller column of that lane) is the larger key.
//                      At the end of a window the lanes' keys go through LDS to one lane per row, which decodes them into
//                      (score, frame-local column) and merges them under "score descending, column ascending".
//                      With one column chunk per row block the wave writes its rows: in place the five match fields of
//                      set 1 (PairOut, common.hpp), pair-indexed the seven output fields of out[i * max_pts + row], so
//                      that frames may repeat across pairs (counted unless mutual).  Otherwise it stores (best, index,
//                      second) per row and chunk.  Mutual: it maintains the column keys (i8_colkey_tile).
// match_i8_merge_kernel in place: merges them over the chunks (it returns at once when nothing was chunked).
// match_pairs_i8_final_kernel  pair-indexed, per (pair, row): the chunk merge or the row the sweep wrote, the mutual test
//                      against the key of its match (only the rows that are also their column's best row keep their
//                      match), the final row, d_num_matched and d_out_counts.
// Columns are cut into chunks only when the row blocks of the call do not fill I8_TARGET_ROUNDS rounds of the grid.
// The tile loop is match_i8_sweep.inc.
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

// recs1 / recs2 and q1 / q2 are read only; each pair may be the same array.  In place, `out` is recs1 again: the rows
// written are the five match fields of set-1 rows, which the kernels do not read.
struct I8Args {
  const SiftPointD *recs1, *recs2;
  const int8_t *q1, *q2;
  const int *hdr;
  const PairPlan *plan;
  int npairs, max_pts;           // max_pts: pair-indexed calls only, as keys and num_matched
  SiftPointD *out;               // in place: set 1; pair-indexed: the rows of pair i at out + i * max_pts
  unsigned long long *keys;      // npairs x max_pts column keys, mutual calls only
  int *num_matched;              // may be NULL
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

// wave-uniform: keep the loop bounds and the key constant in SGPRs
__device__ __forceinline__ void i8_uniform(PairPlan &P)
{
  P.n1 = __builtin_amdgcn_readfirstlane(P.n1); P.n2 = __builtin_amdgcn_readfirstlane(P.n2);
  P.off1 = __builtin_amdgcn_readfirstlane(P.off1); P.off2 = __builtin_amdgcn_readfirstlane(P.off2);
  P.ntiles = __builtin_amdgcn_readfirstlane(P.ntiles); P.nchunks = __builtin_amdgcn_readfirstlane(P.nchunks);
  P.tpc = __builtin_amdgcn_readfirstlane(P.tpc); P.item0 = __builtin_amdgcn_readfirstlane(P.item0);
}

// row rr of row block rb of the pair merged over the pair's chunks, in ascending order
__device__ __forceinline__ void i8_merge_chunks(const int4 *partial, const PairPlan &P, int rb, int rr, int &M, int &I,
                                                int &S2)
{
  const int4 *q = partial + (size_t)(P.item0 + rb * P.nchunks) * I8_ROWS + rr;
  for (int ch = 0; ch < P.nchunks; ch++, q += I8_ROWS) {
    const int4 v = *q;
    i8_take(M, I, S2, v.x, v.y, v.z);
  }
}

// Column keys of misift_match_pairs_batch_i8's mutual check (the design of colkey_* in kernels_match.hip on integer
// scores): key = (S << 32) | (0xFFFFFFFF - row), so that for S > 0 the unsigned order of keys is (larger S, then smaller
// row), and an atomic max over any cut of the rows and columns leaves the column's best row: the match
// misift_match_batch_i8 with the sets swapped writes.  0 = no row with S > 0.
// Of one tile a lane holds 32 scores of its column, acc0[r] and acc1[r], whose rows ascend with k = 16 ai + r (row =
// row0 + 32 ai + (r & 3) + 8 (r >> 2) + 4 h).  Its best is the maximum of the packed (S << 5) | (31 - k), S <= 2^21: the
// smaller k of equal S is the larger.  S <= 0 packs to at most 31 or to a negative number and decodes to "none"; rows at
// or above n1 have zero q, so S = 0.  The two lane halves are combined as (S << 6) | (63 - row within the wave), and the
// 32 lanes of half 0 issue one 8-byte atomic each: 32 consecutive columns, 256 contiguous bytes.
__device__ __forceinline__ void i8_colkey_tile(unsigned long long *key, const v16i &acc0, const v16i &acc1, int row0,
                                               int h)
{
  int pk = 0;
#pragma unroll
  for (int r = 0; r < 16; r++)
    pk = max(pk, max((int)((unsigned)acc0[r] << 5) | (31 - r), (int)((unsigned)acc1[r] << 5) | (15 - r)));
  const int s = pk >> 5, k = 31 - (pk & 31);
  const int rl = 32 * (k >> 4) + (k & 3) + 8 * ((k & 15) >> 2) + 4 * h;
  const unsigned mine = s > 0 ? ((unsigned)s << 6) | (unsigned)(63 - rl) : 0u;
  const auto sw = __builtin_amdgcn_permlane32_swap(mine, mine, false, false);   // [1] in lanes 0-31: lane + 32's value
  const unsigned best = max(mine, (unsigned)sw[1]);
  if (h == 0 && best != 0u) {
    const unsigned row = (unsigned)row0 + 63u - (best & 63u);
    __hip_atomic_fetch_max(key, ((unsigned long long)(best >> 6) << 32) | (0xFFFFFFFFu - row), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  }
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

template <int MODE>
__global__ __launch_bounds__(64 * I8_WAVES) void match_i8_kernel(I8Args A)
{
  __shared__ uint2 red[I8_WAVES][32][64];        // per wave: (b1, b2) of row register rr of lane l at [rr][l]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 31, h = lane >> 5;
  const int nitems = A.hdr[0], C = A.hdr[1];
  // the row this lane owns in the fold and the output: row register c & 15 of A tile c >> 4, lane half h
  const int own = 32 * (c >> 4) + (c & 3) + 8 * ((c & 15) >> 2) + 4 * h;
  for (int it = (int)xcd_remap(blockIdx.x, gridDim.x); it < nitems; it += gridDim.x) {
    const int pi = __builtin_amdgcn_readfirstlane(pair_find<false>(A.plan, A.npairs, it));
    PairPlan P = A.plan[pi];
    i8_uniform(P);
    const int local = it - P.item0, rb = local / P.nchunks, chunk = local - rb * P.nchunks;
    const int t0 = chunk * P.tpc, t1 = min(t0 + P.tpc, P.ntiles);
    const int row0 = rb * I8_ROWS + wave * 64;
    unsigned long long *const ck_keys = A.keys + (size_t)pi * A.max_pts;
#define I8_COL_KEYS(t, acc0, acc1) \
  if constexpr (MODE == PAIR_OUT_MUTUAL) i8_colkey_tile(ck_keys + (size_t)(t) * I8_TILE + c, acc0, acc1, row0, h)
#include "match_i8_sweep.inc"
#undef I8_COL_KEYS
    const int row = row0 + own;
    bool matched = false;            // unchunked, no filter: the row's final match is known here, and counted here
    if (row < P.n1) {
      if (C == 1) {
        SiftPointD *o = MODE == PAIR_OUT_INPLACE ? A.out + P.off1 + row : A.out + (size_t)pi * A.max_pts + row;
        if constexpr (MODE != PAIR_OUT_INPLACE) {
          o->xpos = A.recs1[P.off1 + row].xpos;
          o->ypos = A.recs1[P.off1 + row].ypos;
        }
        i8_write_row(o, A.recs2 + P.off2, M, I, S2);
        matched = MODE == PAIR_OUT_INDEXED && I >= 0;
      } else {
        A.partial[(size_t)it * I8_ROWS + wave * 64 + own] = make_int4(M, I, S2, 0);
      }
    }
    if constexpr (MODE == PAIR_OUT_INDEXED)
      if (C == 1 && A.num_matched) {
        const int n = __popcll(__ballot(matched));
        if (lane == 0 && n > 0) atomicAdd(A.num_matched + pi, n);
      }
  }
}

// In place, chunked calls only: one thread per row of a row block merges the row over the pair's chunks.
__global__ __launch_bounds__(I8_ROWS) void match_i8_merge_kernel(I8Args A)
{
  if (A.hdr[1] <= 1) return;
  const int nrbs = A.hdr[2];
  for (int g = blockIdx.x; g < nrbs; g += gridDim.x) {
    const PairPlan P = A.plan[pair_find<true>(A.plan, A.npairs, g)];
    const int rb = g - P.rb0, row = rb * I8_ROWS + threadIdx.x;
    if (row >= P.n1) continue;
    int M = 0, I = -1, S2 = 0;
    i8_merge_chunks(A.partial, P, rb, threadIdx.x, M, I, S2);
    i8_write_row(A.out + P.off1 + row, A.recs2 + P.off2, M, I, S2);
  }
}

// Pair-indexed: a unit is 256 rows of one pair, one thread per row; units of rows at or above n1 and of oversized pairs
// only write the pair's count.
__global__ __launch_bounds__(256) void match_pairs_i8_final_kernel(I8Args A, int mutual, int *__restrict__ out_counts)
{
  const int C = A.hdr[1];
  const int groups = (A.max_pts + 255) / 256;
  const long long nunits = (long long)A.npairs * groups;
  for (long long u = blockIdx.x; u < nunits; u += gridDim.x) {
    const int pi = (int)(u / groups), g = (int)(u - (long long)pi * groups);
    const PairPlan P = A.plan[pi];
    if (g == 0 && threadIdx.x == 0) out_counts[pi] = P.pad ? -1 : P.n1;
    if (P.pad || g * 256 >= P.n1) continue;                       // uniform over the workgroup
    if (!mutual && C == 1 && P.n2 > 0) continue;                  // the sweep wrote and counted these rows
    const int row = g * 256 + threadIdx.x;
    bool matched = false;
    if (row < P.n1) {
      SiftPointD *o = A.out + (size_t)pi * A.max_pts + row;
      if (P.n2 == 0) {                                            // no column: a no-match row
        o->xpos = A.recs1[P.off1 + row].xpos;
        o->ypos = A.recs1[P.off1 + row].ypos;
        write_no_match(o);
      } else {
        int M = 0, I = -1, S2 = 0;
        if (C > 1) i8_merge_chunks(A.partial, P, row / I8_ROWS, row % I8_ROWS, M, I, S2);
        else I = o->match;                                        // the row match_i8_kernel wrote
        // the mutual test: the column's key names its best row (0 cannot occur here: S of this row and its match is > 0)
        const bool reject =
            mutual && I >= 0 && 0xFFFFFFFFu - (unsigned)A.keys[(size_t)pi * A.max_pts + I] != (unsigned)row;
        if (C > 1) {
          o->xpos = A.recs1[P.off1 + row].xpos;
          o->ypos = A.recs1[P.off1 + row].ypos;
          if (reject) write_no_match(o);
          else i8_write_row(o, A.recs2 + P.off2, M, I, S2);
        } else if (reject) {
          write_no_match(o);                                      // unchunked: xpos / ypos are the sweep's
        }
        matched = I >= 0 && !reject;
      }
    }
    const int n = __syncthreads_count(matched);
    if (A.num_matched && threadIdx.x == 0 && n > 0) atomicAdd(A.num_matched + pi, n);
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

// Enqueue misift_match_batch_i8 (in place; `rows` unused) or misift_match_pairs_batch_i8 on the context stream
// (common.hpp): plan, (mutual) key memset, sweep, finish.
int launch_match_batch_i8(misift_ctx *ctx, PairOut mode, int npairs, const int *h_pairs, void *d_plan,
                          const BatchLayout &set1, const int8_t *q1, const BatchLayout &set2, const int8_t *q2,
                          const PairRows &rows)
{
  if (npairs <= 0) return MISIFT_OK;
  const bool inplace = mode == PAIR_OUT_INPLACE;
  const PairShape S = i8_shape(ctx->num_cus);
  I8Args A;
  int rc = launch_pair_head(ctx, inplace ? "match_i8_plan" : "match_pairs_i8_plan", S, mode,
                            (size_t)pair_partial_items(S) * I8_ROWS * sizeof(int4), npairs, h_pairs, set1, set2, rows,
                            d_plan, &A.keys);
  if (rc) return rc;
  A.recs1 = set1.recs; A.recs2 = set2.recs; A.q1 = q1; A.q2 = q2;
  A.hdr = reinterpret_cast<const int *>(d_plan);
  A.plan = reinterpret_cast<const PairPlan *>(A.hdr + PAIR_HDR_INTS);
  A.npairs = npairs; A.max_pts = rows.max_pts;
  A.out = inplace ? set1.recs : reinterpret_cast<SiftPointD *>(rows.out);
  A.num_matched = rows.num_matched;
  A.partial = reinterpret_cast<int4 *>(ctx->d_match_tmp);
  const int grid = i8_grid(ctx->num_cus);
  {
    LaunchScope ls(ctx, inplace ? "match_i8_mfma" : "match_pairs_i8_mfma");
    const auto sweep = inplace                    ? match_i8_kernel<PAIR_OUT_INPLACE>
                       : mode == PAIR_OUT_MUTUAL ? match_i8_kernel<PAIR_OUT_MUTUAL>
                                                 : match_i8_kernel<PAIR_OUT_INDEXED>;
    hipLaunchKernelGGL(sweep, dim3(grid), dim3(64 * I8_WAVES), 0, ctx->stream, A);
    rc = ls.finish();
    if (rc) return rc;
  }
  LaunchScope ls(ctx, inplace ? "match_i8_merge" : "match_pairs_i8_final");
  if (inplace) hipLaunchKernelGGL(match_i8_merge_kernel, dim3(grid), dim3(I8_ROWS), 0, ctx->stream, A);
  else
    hipLaunchKernelGGL(match_pairs_i8_final_kernel, dim3(grid), dim3(256), 0, ctx->stream, A,
                       (int)(mode == PAIR_OUT_MUTUAL), rows.out_counts);
  return ls.finish();
}

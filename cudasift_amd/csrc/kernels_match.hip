// kernels_match.hip — brute-force descriptor matching on the fp32 matrix cores of gfx950.
//
//   match_kernel + match_merge_kernel replace CleanMatches (reference matching.cu:289-293)
//   and FindMaxCorr10 (matching.cu:301-397), host MatchSiftData (matching.cu:1090-1206).
//
// The only dense contraction of the pipeline: S = D1 (n1 x 128) * D2^T (128 x n2), then a
// per-row (max, second max, argmax).  Each wavefront keeps its 32 rows of D1 for the whole
// K = 128 in VGPRs (64 registers) and sweeps 64-column super-tiles of D2 staged through
// double-buffered LDS as TWO interleaved accumulator chains, one v_mfma_f32_32x32x2_f32 per k-pair and chain with
// k ascending — so every
// score is bit-identical to the reference's sequential fp32 FMA chain (matching.cu:343-346;
// MI355X f32 MFMA == k-ordered fmaf chain).  The running top-2 is kept per lane, i.e. per
// column residue (p2 mod 32); residues 4c..4c+3 form the reference's "class" c = (p2 mod 32)/4
// (thread row iy of FindMaxCorr10), so the reference's lossy 8-class runner-up merge
// (matching.cu:375-390) can be reproduced exactly — or replaced by the exact second best.
// Columns are split into chunks across workgroups to fill 256 CUs; a small merge kernel
// combines the per-chunk class triples and writes score/match/ambiguity/match_xpos/ypos.
// match_batch_kernel<MODE> + match_batch_merge_kernel / match_pairs_final_kernel: the same sweep over many independent
// frame pairs whose sizes only the device knows, into set 1 itself (misift_match_batch) or into pair-indexed output
// rows with an optional mutual check (misift_match_pairs_batch); pair_plan_kernel / pair_plan_capped_kernel: their
// work list, and the int8 matchers'.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "common.hpp"
#include "pair_plan.hpp"

typedef float floatx16 __attribute__((ext_vector_type(16)));

#ifndef MT_WG_WAVES
#define MT_WG_WAVES 4              // wavefronts per workgroup (experiment: 8 = 256 rows share a staged tile, one workgroup per CU)
#endif
#define MT_ROWS_PER_BLOCK (32 * MT_WG_WAVES)
#define MT_STAGE (32 / MT_WG_WAVES)   // float4 loads per thread and super-tile
// LDS image of a 32-column tile of D2: column-major, each column split into its even-k and odd-k halves
// ([col][half][64]) so that lane (col, half) — which feeds k = 2t + half to MFMA t — reads its 64 operands
// as 16 contiguous ds_read_b128.  Column stride 132 floats: a b128 lane group (16 columns) then starts on
// 16 distinct multiples of 4 banks => conflict-free.
#define MT_BSTRIDE 132
#define MT_TILE 32

struct MatchGeom {
  int row_begin, row_count;      // rows of set 1 handled by this launch
  int n1_total;
  int n2, ncols;                 // set-2 size, columns that take part (32*floor(n2/32) or n2)
  int ntiles, nchunks, tiles_per_chunk;   // super-tiles / chunks of THIS launch
  // A launch sweeps a run of `ntiles` VIRTUAL super-tiles: virtual tile v is actual tile tile_base + v, plus hole_len
  // from v >= hole_begin on (the sharded matcher sweeps its own shard's tiles while the rest of set 2 is still on the
  // wire, then everything around them: multigpu.hip).  Chunk c of this launch is chunk chunk_base + c of nchunks_total.
  int tile_base, hole_begin, hole_len;
  int chunk_base, nchunks_total;
  // set-2 element layout, in floats: SiftPoint records (stride 144, descriptor at 16, xpos/ypos at 0) or the packed
  // match columns the sharded matcher ships (MISIFT_MATCH_COLUMN_BYTES = 528: stride 132, descriptor at 0, xy at 128)
  int stride2, data_off2, xy_off2;
};
__device__ __forceinline__ int tile_col0(const MatchGeom &G, int v)       // first column of virtual super-tile v
{
  return (G.tile_base + v + (v >= G.hole_begin ? G.hole_len : 0)) * 64;
}

// partial results: [row][class][chunk][3] : max, second, index — one contiguous run of chunks per (row, class), which is
// what a thread of match_merge_kernel reads
#define MT_PART_WORDS 24

__device__ __forceinline__ void top2_update(float sc, int p2, float &mx, float &sec, int &ix)
{
  // reference update rule (matching.cu:352-360): `if (sc > mx) {sec = mx; mx = sc; ix = p2;} else if (sc > sec)
  // sec = sc;` — strict '>' so the earliest column wins ties.  With sec <= mx always, the new (sec, mx) is the
  // top two of {sec, mx, sc}: sec' = median of the three (one v_med3_f32), mx' = sc or mx.  4 VALU per score
  // (compare, median, two selects) instead of 8 with fmaxf (which also costs canonicalising v_max x,x pairs).
  const bool gt = sc > mx;
  sec = __builtin_amdgcn_fmed3f(sec, mx, sc);
  ix = gt ? p2 : ix;
  mx = gt ? sc : mx;
}

// exact merge of two top-2 summaries of disjoint column sets (ties -> smaller column index,
// which is what one ascending scan over the union would produce)
// (selects, not branches: as an if/else every merge became two exec-mask regions behind its own operand wait, and the
//  32 merges at the end of match_kernel ran as one serial chain — 4.4 us of a 24 us launch, tools/match_stamps.py)
__device__ __forceinline__ void top2_merge(float &mx, float &sec, int &ix, float omx, float osec, int oix)
{
  const bool take = (omx > mx) | ((omx == mx) & (oix >= 0) & ((ix < 0) | (oix < ix)));
  const float sec_take = fmaxf(mx, osec), sec_keep = fmaxf(sec, omx);
  sec = take ? sec_take : sec_keep;
  mx = take ? omx : mx;
  ix = take ? oix : ix;
}
// The final combination of the eight class summaries of one row: the reference's lossy merge, literally
// (matching.cu:375-390), or the exact second best under match_exact_top2.
__device__ __forceinline__ void mb_combine(int exact_top2, const float (&cmax)[8], const float (&csec)[8],
                                           const int (&cidx)[8], float &max_score, float &sec_score, int &index)
{
  if (exact_top2) {
    max_score = cmax[0]; sec_score = csec[0]; index = cidx[0];
#pragma unroll
    for (int c = 1; c < 8; c++) top2_merge(max_score, sec_score, index, cmax[c], csec[c], cidx[c]);
  } else {
    max_score = cmax[0]; sec_score = csec[0]; index = cidx[0];
#pragma unroll
    for (int y = 0; y < 8; y++)
      if (index != cidx[y]) {
        if (cmax[y] > max_score) {
          sec_score = fmaxf(max_score, sec_score);
          max_score = cmax[y];
          index = cidx[y];
        } else if (cmax[y] > sec_score)
          sec_score = cmax[y];
      }
  }
}
// lane ^ 1 / lane ^ 2 within a quad: one DPP move each (quad_perm [1,0,3,2] = 0xB1, [2,3,0,1] = 0x4E), no LDS round trip
template <int CTRL> __device__ __forceinline__ int quad_xchg(int v)
{
  return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true);
}
template <int CTRL> __device__ __forceinline__ float quad_xchg(float v)
{
  return __builtin_bit_cast(float, quad_xchg<CTRL>(__builtin_bit_cast(int, v)));
}

// Column keys of misift_match_pairs_batch's mutual check (match_sweep.inc under MT_COL_KEYS): key = (fp32 bits of S) << 32
// | (0xFFFFFFFF - row), so that for S > 0 the unsigned order of keys is (larger S, then smaller row) and an atomic max
// over any cut of the rows and columns leaves the reversed match of the column: what misift_match with the sets swapped
// finds in match_full + match_exact_top2 mode.  0 = no row with S > 0.
// colkey_step over a lane's accumulator registers in ascending order (rows ascend with the register, match_sweep.inc):
// strict '>' keeps the smallest row of a tie; NaN and S <= 0 never enter.
__device__ __forceinline__ void colkey_step(float s, int r, float &kb, int &kr)
{
  const bool gt = s > kb;
  kb = gt ? s : kb;
  kr = gt ? r : kr;
}
// The lane's key for its column, combined with lane ^ 32 (the other 16 rows of the wavefront's 32), and one atomic max
// per column from the lanes of half 0: 32 consecutive columns, 256 contiguous bytes.  A padded row (>= n1) is a copy of
// row n1 - 1 (match_sweep.inc clamps the fetch), so its score is bit-identical to that row's: clamping its index to
// last = n1 - 1 makes its key that row's key.
__device__ __forceinline__ void colkey_flush(unsigned long long *key, float kb, int kr, int row0, int last, int half)
{
  const int row = min(row0 + (kr & 3) + 8 * (kr >> 2), last);
  const unsigned hi = kb > 0.0f ? __float_as_uint(kb) : 0u, lo = kb > 0.0f ? 0xFFFFFFFFu - (unsigned)row : 0u;
  const auto h2 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);     // [1] in lanes 0-31: lane + 32's value
  const auto l2 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const unsigned long long mine = ((unsigned long long)hi << 32) | lo;
  const unsigned long long other = ((unsigned long long)(unsigned)h2[1] << 32) | (unsigned)l2[1];
  const unsigned long long k = mine > other ? mine : other;
  if (half == 0 && k != 0ull) __hip_atomic_fetch_max(key, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class V>
__device__ __forceinline__ void colkey_tile(unsigned long long *key, const V &acc, int row0, int last, int half)
{
  float kb = 0.0f;
  int kr = 0;
#pragma unroll
  for (int r = 0; r < 16; r++) colkey_step(acc[r], r, kb, kr);
  colkey_flush(key, kb, kr, row0, last, half);
}

// One workgroup = 4 wavefronts = 128 rows of set 1; it sweeps a chunk of 64-column super-tiles of set 2.
// Per super-tile every wavefront runs TWO independent accumulator chains (columns 0-31 and 32-63) of
// 64 dependent v_mfma_f32_32x32x2_f32 each, interleaved, so the 64-cycle dependent-issue latency of one
// chain is covered by the other (and by the second wavefront resident on the SIMD).
#define MT_SUPER 64
#ifndef MT_A_SWAP
#define MT_A_SWAP 1
#endif
#ifndef MT_STAMPS
#define MT_STAMPS 0              // developer build (tools/variants.sh -DMT_STAMPS=1): 100 MHz time stamps, tools/match_stamps.py
#endif
#if MT_STAMPS
__device__ unsigned g_mt_stamp[16];
#define MT_STAMP_MAX(slot) do { if (threadIdx.x == 0) atomicMax(&g_mt_stamp[slot], (unsigned)wall_clock64()); } while (0)
#define MT_STAMP_MIN(slot) do { if (threadIdx.x == 0) atomicMin(&g_mt_stamp[slot], (unsigned)wall_clock64()); } while (0)
extern "C" int misift_debug_match_stamps(unsigned *out16)
{
  unsigned init[16];
  for (int i = 0; i < 16; i++) init[i] = (i == 0 || i == 8) ? 0xffffffffu : 0u;
  HIP_TRY(hipDeviceSynchronize());
  if (out16) HIP_TRY(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_mt_stamp), sizeof(init)));
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_mt_stamp), init, sizeof(init)));
  return MISIFT_OK;
}
#else
#define MT_STAMP_MAX(slot) do { } while (0)
#define MT_STAMP_MIN(slot) do { } while (0)
#endif
__global__ __launch_bounds__(64 * MT_WG_WAVES, 8 / MT_WG_WAVES) void match_kernel(const SiftPointD *__restrict__ pts1,
                                                       const float *__restrict__ set2, MatchGeom G,
                                                       float *__restrict__ partial)
{
  __shared__ float Bs[2][MT_SUPER * MT_BSTRIDE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5, col = lane & 31;
  const unsigned item = xcd_remap(blockIdx.x, gridDim.x);
  // chunk-major: the workgroups resident on one XCD work on the same chunk of set 2 (it stays in that L2)
  const int nrb = (G.row_count + MT_ROWS_PER_BLOCK - 1) / MT_ROWS_PER_BLOCK;
  const int chunk = item / nrb, rb = item % nrb;
  const int st0 = chunk * G.tiles_per_chunk;                       // super-tile range of this chunk
  const int st1 = min(st0 + G.tiles_per_chunk, G.ntiles);
  MT_STAMP_MIN(0);                 // first workgroup starts
  MT_STAMP_MAX(1);                 // last workgroup starts

  // the sweep (match_sweep.inc, shared with match_batch_kernel): leaves mx / sec / ix
#include "match_sweep.inc"
  if ((lane & 3) == 0) {
    const int cls = col >> 2;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int rl = rb * MT_ROWS_PER_BLOCK + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (rl < G.row_count) {
        float *p = partial + (((size_t)rl * 8 + cls) * G.nchunks_total + G.chunk_base + chunk) * 3;
        p[0] = mx[r];
        p[1] = sec[r];
        reinterpret_cast<int *>(p)[2] = ix[r];
      }
    }
  }
  MT_STAMP_MAX(5);                 // partial results stored
}

// Eight threads per row, one per class: each merges its class over the chunks (a contiguous run of 12-byte triples; r02
// had one thread per row walk a strided [chunk][24] table — 0.34 ms for 12 500 rows x 126 chunks, 13 % of that sweep),
// then the eight classes are combined in every lane of the group exactly as before and lane 0 writes the row.
__global__ __launch_bounds__(256) void match_merge_kernel(SiftPointD *__restrict__ pts1,
                                                          const float *__restrict__ set2, MatchGeom G,
                                                          const float *__restrict__ partial, int exact_top2,
                                                          unsigned *__restrict__ ticket, unsigned *__restrict__ host_flag,
                                                          unsigned host_seq)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int rl = t >> 3;
  const bool live = rl < G.row_count;
  MT_STAMP_MIN(8);
  MT_STAMP_MAX(9);
  float m = 0.0f, sd = 0.0f;
  int ixm = -1;
  if (live) {
    const float *p = partial + (size_t)t * G.nchunks_total * 3;
    int ch = 0;
    for (; ch + 4 <= G.nchunks_total; ch += 4) {                  // four triples in flight
      float a[12];
#pragma unroll
      for (int k = 0; k < 12; k++) a[k] = p[3 * ch + k];
#pragma unroll
      for (int k = 0; k < 4; k++) top2_merge(m, sd, ixm, a[3 * k], a[3 * k + 1], __float_as_int(a[3 * k + 2]));
    }
    for (; ch < G.nchunks_total; ch++) top2_merge(m, sd, ixm, p[3 * ch], p[3 * ch + 1], __float_as_int(p[3 * ch + 2]));
  }
  float cmax[8], csec[8];
  int cidx[8];
#pragma unroll
  for (int c = 0; c < 8; c++) {
    cmax[c] = __shfl(m, c, 8);
    csec[c] = __shfl(sd, c, 8);
    cidx[c] = __shfl(ixm, c, 8);
  }
  if (live && (t & 7) == 0) {
    float max_score, sec_score;
    int index;
    mb_combine(exact_top2, cmax, csec, cidx, max_score, sec_score, index);
    SiftPointD *o = &pts1[G.row_begin + rl];
    o->score = max_score;
    o->match = index;
    const float *m2 = set2 + (size_t)(index >= 0 ? index : 0) * G.stride2 + G.xy_off2;
    o->match_xpos = index >= 0 ? m2[0] : 0.0f;              // never reads sift2[-1] (Appendix B #9)
    o->match_ypos = index >= 0 ? m2[1] : 0.0f;
    o->ambiguity = sec_score / (max_score + 1e-6f);
  }
  // Synchronous callers (misift_match): the workgroup that draws the last ticket stores the call's sequence number in
  // pinned host memory, which the host polls instead of synchronising the stream (r04 single-call budget: ~5 us of the
  // 39 us a 2000 x 2000 MatchSiftData took).  The ticket word is left at zero for the next call.
  MT_STAMP_MAX(10);                // rows written
  if (!host_flag) return;
  __shared__ unsigned s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // vmcnt(0): this wavefront's row stores are acknowledged BEFORE the ticket is
                                             // drawn (the workgroup-scope fence alone waits for lgkmcnt only; advisor r04)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (s_last && threadIdx.x == 0) {
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(host_flag, host_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    MT_STAMP_MAX(11);              // flag on its way to the host
  }
}

// Column chunks for a launch of `ntiles` super-tiles over nrb row blocks.  Measured (r03, tools/match_chunks.py,
// profiles/r03_match_chunks.json): a CU works its workgroups off at a fixed rate, two resident at a time, so the launch
// takes ceil(workgroups / CUs) "CU rounds" of one chunk each plus ~3/4 of a super-tile of prologue/epilogue per workgroup,
// and what hurts is a chunk count that leaves the last round nearly empty (12 500 rows: 42 chunks = 16.08 rounds is the
// worst of 14 counts tried, 26 chunks = 9.95 rounds the best) — r02's fixed "24 workgroups per slot" gave 2-3 tiles per
// chunk at 16 384 x 16 384 (0.78 ms; 10 chunks: 0.61 ms).  So: the count that minimises rounds x (tiles per chunk + 3/4).
static int match_plan_param(const char *name, int dflt)
{
  const char *e = getenv(name);
  const int v = e ? atoi(e) : 0;
  return v > 0 ? v : dflt;
}
static void plan_chunks_cus(int ncu, int nrb, int ntiles, int &nchunks, int &tiles_per_chunk)
{
  static const int forced = match_plan_param("MISIFT_MATCH_CHUNKS", 0);       // experiments only
  nchunks = 1; tiles_per_chunk = ntiles > 0 ? ntiles : 1;
  if (ntiles <= 0 || nrb <= 0) return;
  if (ncu <= 0) ncu = 256;
  const int cmax = ntiles < 256 ? ntiles : 256;
  double best = 0.0;
  for (int c = 1; c <= cmax; c++) {
    const int tpc = (ntiles + c - 1) / c;
    if ((ntiles + tpc - 1) / tpc != c) continue;                    // the same cut as a smaller count
    const long long m = ((long long)nrb * c + ncu - 1) / ncu;      // workgroups of the most loaded CU; two run side by side,
    const double rounds = 2.0 * (m / 2) + 1.35 * (m & 1);           // one alone does not keep the matrix pipe full
    const double cost = rounds * (tpc + 0.75);
    if (c == 1 || cost < best * 0.999) { best = cost; nchunks = c; tiles_per_chunk = tpc; }
  }
  if (forced) {
    nchunks = forced < ntiles ? forced : ntiles;
    tiles_per_chunk = (ntiles + nchunks - 1) / nchunks;
    nchunks = (ntiles + tiles_per_chunk - 1) / tiles_per_chunk;
  }
}

static void plan_chunks(const misift_ctx *ctx, int nrb, int ntiles, int &nchunks, int &tiles_per_chunk)
{
  plan_chunks_cus(ctx->num_cus, nrb, ntiles, nchunks, tiles_per_chunk);
}
// host-only test hook (no device needed): the chunk plan for n1 rows x n2 columns on a chip of `num_cus` CUs
extern "C" int misift_test_match_plan(int num_cus, int n1, int n2, int *nchunks, int *tiles_per_chunk, int *ntiles)
{
  if (!nchunks || !tiles_per_chunk || !ntiles || n1 < 0 || n2 < 0) return MISIFT_EINVAL;
  const int ncols = MT_TILE * (n2 / MT_TILE);
  *ntiles = (ncols + MT_SUPER - 1) / MT_SUPER;
  plan_chunks_cus(num_cus, (n1 + MT_ROWS_PER_BLOCK - 1) / MT_ROWS_PER_BLOCK, *ntiles, *nchunks, *tiles_per_chunk);
  return MISIFT_OK;
}

// The sweep in up to two launches: first the super-tiles [own_t0, own_t1) read through `pts2_own` (a pointer such that
// pts2_own[column] is valid for exactly those tiles' columns: the rank's own shard of set 2, wherever it lies), then —
// behind `rest_ready` on the context stream — every other super-tile from pts2; one merge over the chunks of both.  The
// per-class top-2 summaries and their exact merge do not depend on how the columns are cut (top2_merge: ties go to
// the smaller column), so the result is the single sweep's, bit for bit.  own_t0 == own_t1: the plain single launch.
// `phase` lets the caller post its exchange between the two launches (the chunk plan is a pure function of the arguments).
int launch_match_split(misift_ctx *ctx, SiftPointD *pts1, int row_begin, int row_count, const SiftPointD *pts2, int n2,
                       const SiftPointD *pts2_own, int own_t0, int own_t1, hipEvent_t rest_ready, int phase, int packed2)
{
  if (row_count <= 0 || n2 <= 0) return MISIFT_OK;
  MatchGeom G;
  memset(&G, 0, sizeof(G));                    // (phases that skip a launch still pass G by value to the merge)
  G.row_begin = row_begin; G.row_count = row_count; G.n1_total = row_begin + row_count;
  G.n2 = n2;
  if (packed2) { G.stride2 = MISIFT_MATCH_COLUMN_BYTES / 4; G.data_off2 = 0; G.xy_off2 = 128; }
  else { G.stride2 = MISIFT_POINT_BYTES / 4; G.data_off2 = 16; G.xy_off2 = 0; }
  const float *f2 = reinterpret_cast<const float *>(pts2), *f2_own = reinterpret_cast<const float *>(pts2_own);
  G.ncols = ctx->opt.match_full ? n2 : MT_TILE * (n2 / MT_TILE);
  const int ntiles_all = (G.ncols + MT_SUPER - 1) / MT_SUPER;                 // 64-column super-tiles
  const int nrb = (row_count + MT_ROWS_PER_BLOCK - 1) / MT_ROWS_PER_BLOCK;
  if (own_t1 > ntiles_all) own_t1 = ntiles_all;
  if (own_t0 < 0) own_t0 = 0;
  const int n_own = own_t1 > own_t0 ? own_t1 - own_t0 : 0, n_rest = ntiles_all - n_own;
  int ch_own = 0, tpc_own = 1, ch_rest = 0, tpc_rest = 1;
  if (n_own) plan_chunks(ctx, nrb, n_own, ch_own, tpc_own);
  if (n_rest || !n_own) plan_chunks(ctx, nrb, n_rest, ch_rest, tpc_rest);
  G.nchunks_total = ch_own + ch_rest;
  const size_t need = (size_t)row_count * G.nchunks_total * MT_PART_WORDS * sizeof(float);
  {
    int rc = misift_ensure_tmp(ctx, need);
    if (rc) return rc;
  }
  float *partial = reinterpret_cast<float *>(ctx->d_match_tmp);
  if (n_own && phase != MATCH_PHASE_REST) {
    G.ntiles = n_own; G.nchunks = ch_own; G.tiles_per_chunk = tpc_own;
    G.tile_base = own_t0; G.hole_begin = 0x7fffffff; G.hole_len = 0; G.chunk_base = 0;
    LaunchScope ls(ctx, "match_mfma");
    hipLaunchKernelGGL(match_kernel, dim3(nrb * ch_own), dim3(64 * MT_WG_WAVES), 0, ctx->stream, pts1, f2_own, G, partial);
    int rc = ls.finish();
    if (rc) return rc;
  }
  if (phase == MATCH_PHASE_OWN) return MISIFT_OK;
  if (rest_ready) HIP_TRY(hipStreamWaitEvent(ctx->stream, rest_ready, 0));
  if (ch_rest) {
    G.ntiles = n_rest; G.nchunks = ch_rest; G.tiles_per_chunk = tpc_rest;
    G.tile_base = 0; G.hole_begin = n_own ? own_t0 : 0x7fffffff; G.hole_len = n_own; G.chunk_base = ch_own;
    LaunchScope ls(ctx, "match_mfma");
    hipLaunchKernelGGL(match_kernel, dim3(nrb * ch_rest), dim3(64 * MT_WG_WAVES), 0, ctx->stream, pts1, f2, G, partial);
    int rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, "match_merge");
    unsigned *host_flag = nullptr;
    if (ctx->want_match_flag && ctx->h_flags && ctx->d_flags) {
      host_flag = ctx->h_flags;
      ctx->match_seq++;
      ctx->match_flagged = 1;
    }
    hipLaunchKernelGGL(match_merge_kernel, dim3((row_count * 8 + 255) / 256), dim3(256), 0, ctx->stream, pts1, f2,
                       G, partial, ctx->opt.match_exact_top2, ctx->d_flags, host_flag, ctx->match_seq);
    return ls.finish();
  }
}

int launch_match(misift_ctx *ctx, SiftPointD *pts1, int row_begin, int row_count, const SiftPointD *pts2, int n2)
{
  return launch_match_split(ctx, pts1, row_begin, row_count, pts2, n2, nullptr, 0, 0, nullptr, MATCH_PHASE_ALL, 0);
}

// ============================================================================ batched pair matching
// (misift_match_batch, misift_match_pairs_batch)
// MatchSiftData of many independent (frame of set 1, frame of set 2) pairs, with the frames' sizes known on the device
// only.  The rows go into set 1 itself (in place: a frame of set 1 in at most one pair), or pair-indexed to
// out[i * max_pts + row], where frames may repeat across pairs, and with `mutual` only the rows that are also their
// column's reversed match keep their match (PairOut, pair_plan.hpp).
//   pair_plan_kernel          one workgroup: the work list of the pairs (pair_plan.hpp), here with 128-row blocks and
//   pair_plan_capped_kernel   64-column super-tiles; they serve the int8 matchers too.  Capped (pair-indexed): oversized
//                             pairs get no work;
//   (mutual) memset           the column keys of every (pair, column) to 0;
//   match_batch_kernel<MODE>  persistent grid of two workgroups per CU; each takes items in a fixed stride and runs the
//                             same sweep as match_kernel (match_sweep.inc) on them.  With one chunk per row block the
//                             workgroup merges the eight classes and writes its rows itself (pair-indexed: all seven
//                             output fields, counted unless mutual); otherwise it stores the per-class triples of the
//                             item.  Mutual: it maintains the column keys;
//   match_batch_merge_kernel  in place: merges the triples over the chunks (it returns at once when nothing was chunked);
//   match_pairs_final_kernel  pair-indexed, per (pair, row): the chunk merge or the row the sweep wrote, the mutual test
//                             against the key of its match, the final row, d_num_matched and d_out_counts.
// Columns are cut into chunks only when the row blocks of the whole call do not fill one round (two workgroups per CU).
#define MB_PART_FLOATS (MT_ROWS_PER_BLOCK * 8 * 3)     // per-class (max, second, index) of an item's 128 rows

// one round = two workgroups per CU (match_kernel's occupancy); columns 32 * floor(n2 / 32) unless match_full
static PairShape mb_shape(int ncu, int full)
{
  return PairShape{MT_ROWS_PER_BLOCK, MT_SUPER, full ? 1 : MT_TILE, 2 * (ncu > 0 ? ncu : 256)};
}

__global__ __launch_bounds__(1024) void pair_plan_kernel(const int *__restrict__ pairs, int npairs, BatchLayout set1,
                                                         BatchLayout set2, PairShape S, int *__restrict__ hdr,
                                                         PairPlan *__restrict__ plan)
{
#define PAIR_PLAN_CAPPED 0
#include "pair_plan_body.inc"
#undef PAIR_PLAN_CAPPED
}
// the pair-indexed matchers: oversized pairs get no work
__global__ __launch_bounds__(1024) void pair_plan_capped_kernel(const int *__restrict__ pairs, int npairs,
                                                                BatchLayout set1, BatchLayout set2, PairShape S,
                                                                int max_pts, int *__restrict__ num_matched,
                                                                int *__restrict__ hdr, PairPlan *__restrict__ plan)
{
#define PAIR_PLAN_CAPPED 1
#include "pair_plan_body.inc"
#undef PAIR_PLAN_CAPPED
}

size_t pair_plan_bytes(int npairs) { return sizeof(int) * PAIR_HDR_INTS + sizeof(PairPlan) * ((size_t)npairs + 1); }

int launch_pair_head(misift_ctx *ctx, const char *plan_name, const PairShape &S, PairOut mode, size_t part_bytes,
                     int npairs, const int *h_pairs, const BatchLayout &set1, const BatchLayout &set2,
                     const PairRows &rows, void *d_plan, unsigned long long **keys)
{
  const size_t key_bytes = mode == PAIR_OUT_MUTUAL ? sizeof(unsigned long long) * (size_t)npairs * rows.max_pts : 0;
  int rc = misift_ensure_tmp(ctx, part_bytes + key_bytes);
  if (rc) return rc;
  *keys = key_bytes ? reinterpret_cast<unsigned long long *>((char *)ctx->d_match_tmp + part_bytes) : nullptr;
  int *hdr = reinterpret_cast<int *>(d_plan);
  PairPlan *plan = reinterpret_cast<PairPlan *>(hdr + PAIR_HDR_INTS);
  {
    LaunchScope ls(ctx, plan_name);
    if (mode == PAIR_OUT_INPLACE)
      hipLaunchKernelGGL(pair_plan_kernel, dim3(1), dim3(1024), 0, ctx->stream, h_pairs, npairs, set1, set2, S, hdr, plan);
    else
      hipLaunchKernelGGL(pair_plan_capped_kernel, dim3(1), dim3(1024), 0, ctx->stream, h_pairs, npairs, set1, set2, S,
                         rows.max_pts, rows.num_matched, hdr, plan);
    rc = ls.finish();
    if (rc) return rc;
  }
  if (key_bytes) HIP_TRY(hipMemsetAsync(*keys, 0, key_bytes, ctx->stream));
  return MISIFT_OK;
}

int pair_plan_host(const PairShape &S, int npairs, const int *n1, const int *n2, int *plan5, int *nitems, int *chunks,
                   int *partial_items_bound)
{
  if (npairs < 0 || (npairs > 0 && (!n1 || !n2 || !plan5)) || !nitems || !chunks || !partial_items_bound)
    return MISIFT_EINVAL;
  std::vector<int> ntiles(npairs), nrb(npairs);
  long long R = 0;
  for (int p = 0; p < npairs; p++) {
    int ncols;
    pair_shape(S, n1[p] > 0 ? n1[p] : 0, n2[p] > 0 ? n2[p] : 0, ncols, ntiles[p], nrb[p]);
    R += nrb[p];
  }
  const int C = pair_batch_chunks(S, R);
  long long items = 0;
  for (int p = 0; p < npairs; p++) {
    int nch, tpc;
    pair_chunks(ntiles[p], C, nch, tpc);
    int *o = plan5 + 5 * (size_t)p;
    o[0] = (int)items; o[1] = nrb[p]; o[2] = ntiles[p]; o[3] = nch; o[4] = tpc;
    items += (long long)nrb[p] * nch;
  }
  *nitems = (int)items;
  *chunks = C;
  *partial_items_bound = pair_partial_items(S);
  return MISIFT_OK;
}

// the sweep's geometry of one pair: all its rows, its own chunks, SiftPoint records
__device__ __forceinline__ MatchGeom mb_geom(const PairPlan &P)
{
  MatchGeom G;
  G.row_begin = 0; G.row_count = P.n1; G.n1_total = P.n1;
  G.n2 = P.n2; G.ncols = P.ncols;
  G.ntiles = P.ntiles; G.nchunks = P.nchunks; G.tiles_per_chunk = P.tpc;
  G.tile_base = 0; G.hole_begin = 0x7fffffff; G.hole_len = 0;
  G.chunk_base = 0; G.nchunks_total = P.nchunks;
  G.stride2 = MISIFT_POINT_BYTES / 4; G.data_off2 = 16; G.xy_off2 = 0;
  return G;
}
// The five match fields of a row from its combined summary — what match_merge_kernel stores for a row of misift_match.
// set2: the pair's set-2 records.
__device__ __forceinline__ void mb_store_row(SiftPointD *o, const float *set2, float max_score, float sec_score, int index)
{
  o->score = max_score;
  o->match = index;
  const float *m2 = set2 + (size_t)(index >= 0 ? index : 0) * (MISIFT_POINT_BYTES / 4);
  o->match_xpos = index >= 0 ? m2[0] : 0.0f;              // never reads sift2[-1]
  o->match_ypos = index >= 0 ? m2[1] : 0.0f;
  o->ambiguity = sec_score / (max_score + 1e-6f);
}
__device__ __forceinline__ void mb_write_row(SiftPointD *o, const float *set2, int exact_top2, const float (&cmax)[8],
                                             const float (&csec)[8], const int (&cidx)[8])
{
  float max_score, sec_score;
  int index;
  mb_combine(exact_top2, cmax, csec, cidx, max_score, sec_score, index);
  mb_store_row(o, set2, max_score, sec_score, index);
}
// Eight threads per row, one per class: this thread's class merged over the pair's chunks in ascending order, as
// match_merge_kernel does, then the eight classes of the row in every lane of the group.  q: the class's triple in the
// row block's first chunk; dead rows (!live) read nothing.
__device__ __forceinline__ void mb_merge_chunks(bool live, const float *q, int nchunks, float (&cmax)[8],
                                                float (&csec)[8], int (&cidx)[8])
{
  float m = 0.0f, sd = 0.0f;
  int ixm = -1;
  if (live)
    for (int ch = 0; ch < nchunks; ch++, q += MB_PART_FLOATS) top2_merge(m, sd, ixm, q[0], q[1], __float_as_int(q[2]));
#pragma unroll
  for (int c = 0; c < 8; c++) {
    cmax[c] = __shfl(m, c, 8);
    csec[c] = __shfl(sd, c, 8);
    cidx[c] = __shfl(ixm, c, 8);
  }
}

// recs1 / recs2 are read only (descriptors, xpos / ypos) and may be the same array.  In place, `out` is recs1 again
// (frame f against frame f + 1 of one packed batch): the rows written are the five match fields — never bytes the sweep
// reads — so no pointer to the records is __restrict__.
template <int MODE>
__global__ __launch_bounds__(64 * MT_WG_WAVES, 8 / MT_WG_WAVES) void match_batch_kernel(const SiftPointD *recs1,
                                                                                        const float *recs2,
                                                                                        const int *__restrict__ hdr,
                                                                                        const PairPlan *__restrict__ plan,
                                                                                        int npairs, int exact_top2,
                                                                                        int max_pts, SiftPointD *out,
                                                                                        unsigned long long *keys,
                                                                                        int *num_matched,
                                                                                        float *__restrict__ partial)
{
  __shared__ float Bs[2][MT_SUPER * MT_BSTRIDE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5, col = lane & 31;
  const int nitems = hdr[0], C = hdr[1];
  // consecutive items (the row blocks of one pair) go to the workgroups of one XCD: that pair's set 2 stays in its L2
  for (int it = (int)xcd_remap(blockIdx.x, gridDim.x); it < nitems; it += gridDim.x) {
    const int pi = pair_find<false>(plan, npairs, it);
    const PairPlan P = plan[pi];
    const int local = it - P.item0, rb = local / P.nchunks, chunk = local - rb * P.nchunks;
    const int st0 = chunk * P.tpc, st1 = min(st0 + P.tpc, P.ntiles);
    const MatchGeom G = mb_geom(P);
    const SiftPointD *pts1 = recs1 + P.off1;
    const float *set2 = recs2 + (size_t)P.off2 * (MISIFT_POINT_BYTES / 4);
    unsigned long long *const ck_keys = keys + (size_t)pi * max_pts;
    const int ck_row0 = rb * MT_ROWS_PER_BLOCK + wave * 32 + 4 * half, ck_last = P.n1 - 1;
    // the sweep of match_kernel (match_sweep.inc): leaves mx / sec / ix
#define MT_COL_KEYS (MODE == PAIR_OUT_MUTUAL)
#include "match_sweep.inc"
#undef MT_COL_KEYS
    bool matched = false;            // unchunked, no filter: the row's final match is known here, and counted here
    if (C == 1) {
      // the item covers all columns: merge the eight classes here, through the first LDS buffer (free after the sweep)
      float *T = &Bs[0][0];
      if ((lane & 3) == 0) {
        const int cls = col >> 2;
#pragma unroll
        for (int r = 0; r < 16; r++) {
          float *q = T + ((wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * 8 + cls) * 3;
          q[0] = mx[r];
          q[1] = sec[r];
          q[2] = __int_as_float(ix[r]);
        }
      }
      __syncthreads();
      const int row = rb * MT_ROWS_PER_BLOCK + tid;
      if (tid < MT_ROWS_PER_BLOCK && row < P.n1) {
        float cmax[8], csec[8];
        int cidx[8];
#pragma unroll
        for (int c = 0; c < 8; c++) {
          const float *q = T + (tid * 8 + c) * 3;
          float m = 0.0f, sd = 0.0f;                 // as match_merge_kernel: the one chunk merged into (0, 0, -1)
          int ixm = -1;
          top2_merge(m, sd, ixm, q[0], q[1], __float_as_int(q[2]));
          cmax[c] = m; csec[c] = sd; cidx[c] = ixm;
        }
        SiftPointD *o = MODE == PAIR_OUT_INPLACE ? out + P.off1 + row : out + (size_t)pi * max_pts + row;
        if constexpr (MODE != PAIR_OUT_INPLACE) {
          o->xpos = pts1[row].xpos;
          o->ypos = pts1[row].ypos;
        }
        mb_write_row(o, set2, exact_top2, cmax, csec, cidx);
        if constexpr (MODE == PAIR_OUT_INDEXED) matched = o->match >= 0;
      }
    } else if ((lane & 3) == 0) {
      float *pb = partial + (size_t)it * MB_PART_FLOATS;
      const int cls = col >> 2;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int rl = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (rb * MT_ROWS_PER_BLOCK + rl < P.n1) {
          float *q = pb + (rl * 8 + cls) * 3;
          q[0] = mx[r];
          q[1] = sec[r];
          reinterpret_cast<int *>(q)[2] = ix[r];
        }
      }
    }
    // T / Bs are read no more before the next item's first staging store
    if constexpr (MODE == PAIR_OUT_INDEXED) {
      const int n = __syncthreads_count(matched);
      if (tid == 0 && n > 0 && num_matched) atomicAdd(num_matched + pi, n);
    } else {
      __syncthreads();
    }
  }
}

// In place, chunked calls only: a unit is 32 rows of one row block, eight threads per row.
__global__ __launch_bounds__(256) void match_batch_merge_kernel(SiftPointD *recs1, const float *recs2,
                                                                const int *__restrict__ hdr,
                                                                const PairPlan *__restrict__ plan, int npairs,
                                                                int exact_top2, const float *__restrict__ partial)
{
  if (hdr[1] <= 1) return;
  const int nunits = hdr[2] * (MT_ROWS_PER_BLOCK / 32);
  for (int u = blockIdx.x; u < nunits; u += gridDim.x) {
    const int grb = u / (MT_ROWS_PER_BLOCK / 32);
    const PairPlan P = plan[pair_find<true>(plan, npairs, grb)];
    const int rb = grb - P.rb0;
    const int rl = (u % (MT_ROWS_PER_BLOCK / 32)) * 32 + (threadIdx.x >> 3), cls = threadIdx.x & 7;
    const int row = rb * MT_ROWS_PER_BLOCK + rl;
    const bool live = row < P.n1;
    float cmax[8], csec[8];
    int cidx[8];
    mb_merge_chunks(live, partial + (size_t)(P.item0 + rb * P.nchunks) * MB_PART_FLOATS + (rl * 8 + cls) * 3, P.nchunks,
                    cmax, csec, cidx);
    if (live && cls == 0)
      mb_write_row(recs1 + P.off1 + row, recs2 + (size_t)P.off2 * (MISIFT_POINT_BYTES / 4), exact_top2, cmax, csec, cidx);
  }
}

// Pair-indexed: a unit is 32 rows of one pair, eight threads per row; units of rows at or above n1 and of oversized
// pairs only write the pair's count.
__global__ __launch_bounds__(256) void match_pairs_final_kernel(const SiftPointD *recs1, const float *recs2,
                                                                const int *__restrict__ hdr,
                                                                const PairPlan *__restrict__ plan, int npairs,
                                                                int exact_top2, int max_pts, int mutual,
                                                                SiftPointD *out, int *__restrict__ out_counts,
                                                                int *__restrict__ num_matched,
                                                                const unsigned long long *__restrict__ keys,
                                                                const float *__restrict__ partial)
{
  const int C = hdr[1];
  const int groups = (max_pts + 31) / 32;
  const long long nunits = (long long)npairs * groups;
  const int rl = threadIdx.x >> 3, cls = threadIdx.x & 7;
  for (long long u = blockIdx.x; u < nunits; u += gridDim.x) {
    const int pi = (int)(u / groups), g = (int)(u - (long long)pi * groups);
    const PairPlan P = plan[pi];
    if (g == 0 && threadIdx.x == 0) out_counts[pi] = P.pad ? -1 : P.n1;
    if (P.pad || g * 32 >= P.n1) continue;                       // uniform over the workgroup
    if (!mutual && C == 1 && P.n2 > 0) continue;                 // the sweep wrote and counted these rows
    const int row = g * 32 + rl;
    const bool live = row < P.n1;
    SiftPointD *o = out + (size_t)pi * max_pts + row;
    const float *set2 = recs2 + (size_t)P.off2 * (MISIFT_POINT_BYTES / 4);
    int index = -1;
    float max_score = 0.0f, sec_score = 0.0f;
    const bool lead = live && cls == 0;                           // the thread that writes the row
    if (P.n2 == 0) {
      if (lead) {                                                 // no column: a no-match row
        o->xpos = recs1[P.off1 + row].xpos;
        o->ypos = recs1[P.off1 + row].ypos;
        write_no_match(o);
      }
    } else if (C > 1) {
      const int rb = row / MT_ROWS_PER_BLOCK, rr = row % MT_ROWS_PER_BLOCK;
      float cmax[8], csec[8];
      int cidx[8];
      mb_merge_chunks(live, partial + (size_t)(P.item0 + rb * P.nchunks) * MB_PART_FLOATS + (rr * 8 + cls) * 3, P.nchunks,
                      cmax, csec, cidx);
      if (lead) mb_combine(exact_top2, cmax, csec, cidx, max_score, sec_score, index);
    } else if (lead) {
      index = o->match;                                           // the row match_batch_kernel wrote
    }
    // the mutual test: the column's key names its best row (0 cannot occur here: S of this row and its match is > 0)
    const bool reject = mutual && index >= 0 && 0xFFFFFFFFu - (unsigned)keys[(size_t)pi * max_pts + index] != (unsigned)row;
    if (reject) index = -1;
    if (lead && P.n2 > 0 && C > 1) {
      o->xpos = recs1[P.off1 + row].xpos;
      o->ypos = recs1[P.off1 + row].ypos;
      if (reject) write_no_match(o);
      else mb_store_row(o, set2, max_score, sec_score, index);
    } else if (reject) {
      write_no_match(o);                                          // unchunked: xpos / ypos are the sweep's
    }
    const int n = __syncthreads_count(lead && index >= 0);
    if (num_matched && threadIdx.x == 0 && n > 0) atomicAdd(num_matched + pi, n);
  }
}

// host-only test hook (no device needed): the plan misift_match_batch makes for pairs of n1[i] x n2[i] records on a chip
// of num_cus CUs (pair_plan_host; tiles are 64-column super-tiles)
extern "C" int misift_test_match_batch_plan(int num_cus, int match_full, int npairs, const int *n1, const int *n2,
                                            int *plan5, int *nitems, int *chunks, int *partial_items_bound)
{
  return pair_plan_host(mb_shape(num_cus, match_full), npairs, n1, n2, plan5, nitems, chunks, partial_items_bound);
}

// Enqueue misift_match_batch (in place; `rows` unused) or misift_match_pairs_batch on the context stream (common.hpp):
// plan, (mutual) key memset, sweep, finish.
int launch_match_batch(misift_ctx *ctx, PairOut mode, int npairs, const int *h_pairs, void *d_plan,
                       const BatchLayout &set1, const BatchLayout &set2, const PairRows &rows)
{
  if (npairs <= 0) return MISIFT_OK;
  const bool inplace = mode == PAIR_OUT_INPLACE;
  const PairShape S = mb_shape(ctx->num_cus, ctx->opt.match_full);
  unsigned long long *keys;
  int rc = launch_pair_head(ctx, inplace ? "match_batch_plan" : "match_pairs_plan", S, mode,
                            (size_t)pair_partial_items(S) * MB_PART_FLOATS * sizeof(float), npairs, h_pairs, set1, set2,
                            rows, d_plan, &keys);
  if (rc) return rc;
  const int *hdr = reinterpret_cast<const int *>(d_plan);
  const PairPlan *plan = reinterpret_cast<const PairPlan *>(hdr + PAIR_HDR_INTS);
  float *partial = reinterpret_cast<float *>(ctx->d_match_tmp);
  const float *f2 = reinterpret_cast<const float *>(set2.recs);
  SiftPointD *out = inplace ? set1.recs : reinterpret_cast<SiftPointD *>(rows.out);
  const int grid = S.target;
  {
    LaunchScope ls(ctx, inplace ? "match_batch_mfma" : "match_pairs_mfma");
    const auto sweep = inplace                    ? match_batch_kernel<PAIR_OUT_INPLACE>
                       : mode == PAIR_OUT_MUTUAL ? match_batch_kernel<PAIR_OUT_MUTUAL>
                                                 : match_batch_kernel<PAIR_OUT_INDEXED>;
    hipLaunchKernelGGL(sweep, dim3(grid), dim3(64 * MT_WG_WAVES), 0, ctx->stream, set1.recs, f2, hdr, plan, npairs,
                       ctx->opt.match_exact_top2, rows.max_pts, out, keys, rows.num_matched, partial);
    rc = ls.finish();
    if (rc) return rc;
  }
  LaunchScope ls(ctx, inplace ? "match_batch_merge" : "match_pairs_final");
  if (inplace)
    hipLaunchKernelGGL(match_batch_merge_kernel, dim3(grid), dim3(256), 0, ctx->stream, out, f2, hdr, plan, npairs,
                       ctx->opt.match_exact_top2, partial);
  else
    hipLaunchKernelGGL(match_pairs_final_kernel, dim3(grid), dim3(256), 0, ctx->stream, set1.recs, f2, hdr, plan, npairs,
                       ctx->opt.match_exact_top2, rows.max_pts, (int)(mode == PAIR_OUT_MUTUAL), out, rows.out_counts,
                       rows.num_matched, keys, partial);
  return ls.finish();
}

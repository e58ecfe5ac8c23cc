// kernels_select.hip — preemptive matching: which frame pairs of a device-resident batch are worth matching
// (misift_select_pairs_batch).  The rules are select_core.hpp; the host hook misift_test_select_pairs at the end of this
// file applies them with plain loops.
//
// select_gather_kernel  one workgroup per frame: the min(n, top) records with the largest keys by an exact radix select
//                       (four passes of 8 bits over a 256-bin LDS histogram give the key T of the last chosen record and
//                       how many of the records with key == T belong; those are taken in ascending index by an ordered
//                       scan), ranked among themselves by "key descending, index ascending", written to d_sel, and their
//                       128-byte q rows copied to the compact temp array qsel[frame][hp][128], hp = top rounded up to 32;
//                       rows at or past the frame's count are zero, so their scores are 0 and never count.
// select_votes_kernel   the hot path.  Workgroup (a, strip) holds the rows of frame a as A fragments in VGPRs (one wave
//                       per 64 rows, as match_i8_kernel) and walks the frames b of its strip: b's hp x 128 bytes are
//                       staged once in LDS (rows 144 bytes apart: conflict-free 16-byte fragment reads) for all waves,
//                       from registers loaded one frame ahead, so the global loads fly under the frame before;
//                       per 32-column tile 2 x 4 v_mfma_i32_32x32x32_i8 give 64 x 32 exact int32 scores, each lane keeps
//                       the top two packed keys  S * 512 + 2^30 + (511 - t)  per row register (med3 + max, the design of
//                       match_i8_sweep.inc) and the best row of its column among the wave's 64 (the packing of
//                       i8_colkey_tile), stored per wave in LDS.  Then the row keys are folded through LDS (two lanes
//                       per row, 16 entries each), the owner of a row looks up its match's column in the waves' column
//                       keys, applies select_vote, and the votes are counted with a ballot.  One lane writes V[a][b] and
//                       V[b][a].  Integer arithmetic throughout: no ordering rule is needed.
// select_pick_kernel    one workgroup per frame: the first k of its row of V under the neighbour order (the same radix
//                       select on two passes: V <= 256), one keep byte per (f, g).
// select_count_kernel   per row a: how many b > a have keep[a][b] | keep[b][a].
// select_scan_kernel    one workgroup: exclusive prefix sum of those counts, and the summary.
// select_emit_kernel    per row a: its pairs at their places, in ascending b, while they fit max_pairs.
// No workgroup waits for another: six launches.
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "common.hpp"
#include "select_core.hpp"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int SEL_WG = 256;                      // threads of the per-frame kernels (= the bins of a radix pass)
constexpr int SEL_KEY_CACHE = 8192;              // keys of a frame kept in LDS by select_gather_kernel (the rest is re-read)
constexpr int VOTE_ROW = 144;                    // bytes between staged descriptors in LDS
constexpr int VOTE_RED = 65;                     // uint2 between the row registers of the fold
constexpr int VOTE_WIN = 512;                    // tiles a packed key can tell apart (9 bits), as I8_WIN
constexpr unsigned VOTE_OFF = 1u << 30;          // key of S = 0, t = 511
constexpr unsigned VOTE_VALID = VOTE_OFF + 512u; // smallest key with S >= 1
constexpr int VOTE_MAX_STRIP = 32;               // frames b per workgroup at most
constexpr int VOTE_WG_PER_CU = 2;                // what the strip length is planned for

struct SelArgs {
  BatchLayout set;
  const int8_t *q;
  int nframes, top, hp, strip;
  float min_score, max_ambiguity;
  int min_votes, k, max_pairs;
  int *sel, *sel_counts, *votes, *pairs, *pair_votes, *summary;
  int8_t *qsel;                  // nframes x hp x 128
  uint8_t *keep;                 // nframes x nframes
  int4 *meta;                    // per frame: (has records and no neighbour, max of its row of V, more than top records, 0)
  int *rowcount, *rowoff;        // per frame a: selected pairs (a, b > a), and how many lie before them
};

// The thread's place among the workgroup's raised flags in thread order, and their number.  wsum: 4 ints of LDS.
__device__ __forceinline__ int block_rank(bool flag, int *wsum, int &total)
{
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                               // wsum of the previous round has been read
  if (lane == 0) wsum[wave] = __popcll(m);
  __syncthreads();
  int before = __popcll(m & ((1ull << lane) - 1ull));
  total = 0;
#pragma unroll
  for (int w = 0; w < SEL_WG / 64; w++) {
    const int c = wsum[w];
    if (w < wave) before += c;
    total += c;
  }
  return before;
}

// T = the h-th largest (1 <= h <= n) of the keys key_of(0 .. n - 1), which vary in their low 8 * PASSES bits only, and
// need = how many of the keys equal to T are among the h largest.  hist: 256 words of LDS, bc: 2.  Exact: counts only.
template <int PASSES, class KeyOf>
__device__ __forceinline__ void block_threshold(KeyOf key_of, int n, int h, unsigned *hist, unsigned *bc, unsigned &T,
                                                int &need)
{
  unsigned prefix = 0;
  int remaining = h;
  for (int p = PASSES - 1; p >= 0; p--) {
    const int shift = 8 * p;
    const unsigned himask = shift + 8 >= 32 ? 0u : ~0u << (shift + 8);
    __syncthreads();
    hist[threadIdx.x] = 0u;
    __syncthreads();
    for (int r = threadIdx.x; r < n; r += SEL_WG) {
      const unsigned k = key_of(r);
      if ((k & himask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int acc = 0, b = 255;
      for (; b > 0; b--) {
        if (acc + (int)hist[b] >= remaining) break;
        acc += (int)hist[b];
      }
      bc[0] = (unsigned)b;
      bc[1] = (unsigned)(remaining - acc);
    }
    __syncthreads();
    prefix |= bc[0] << shift;
    remaining = (int)bc[1];
  }
  T = prefix;
  need = remaining;
}

// take(r, key) for the h largest: every key above T, and the first `need` of the keys equal to T in ascending index.
template <class KeyOf, class Take>
__device__ __forceinline__ void block_take(KeyOf key_of, int n, unsigned T, int need, int *wsum, Take take)
{
  int eq_before = 0;
  for (int base = 0; base < n; base += SEL_WG) {
    const int r = base + threadIdx.x;
    const bool in = r < n;
    const unsigned k = in ? key_of(r) : 0u;
    const bool eq = in && k == T;
    int total;
    const int rank = eq_before + block_rank(eq, wsum, total);
    if (in && (k > T || (eq && rank < need))) take(r, k);
    eq_before += total;
  }
}

// (m, i, s) <- the top two of (m, i, s) and (mo, io, so): score descending, index ascending; a tie of the best scores
// makes the loser's score the runner-up.  "None" is (0, -1, 0).  The rule of i8_take (kernels_match_i8.hip).
__device__ __forceinline__ void vote_take(int &m, int &i, int &s, int mo, int io, int so)
{
  const bool take = mo > m || (mo == m && (unsigned)io < (unsigned)i);
  const int ns = take ? max(so, m) : max(s, mo);
  if (take) { m = mo; i = io; }
  s = ns;
}

}  // namespace

__global__ __launch_bounds__(SEL_WG) void select_gather_kernel(SelArgs A)
{
  __shared__ unsigned skey[SEL_KEY_CACHE];
  __shared__ unsigned hist[256], bc[2], ckey[SELECT_MAX_TOP];
  __shared__ int wsum[SEL_WG / 64], cidx[SELECT_MAX_TOP], sidx[SELECT_MAX_TOP], ccount;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = max(A.set.counts[f], 0);
  const long long base = A.set.base(f);
  const SiftPointD *__restrict__ recs = A.set.recs + base;
  const int h = min(n, A.top);
  for (int r = tid; r < min(n, SEL_KEY_CACHE); r += SEL_WG) skey[r] = select_key(recs[r].scale);
  if (tid == 0) ccount = 0;
  __syncthreads();
  auto key_of = [&](int r) { return r < SEL_KEY_CACHE ? skey[r] : select_key(recs[r].scale); };
  if (h > 0) {                                   // uniform over the workgroup
    unsigned T;
    int need;
    block_threshold<4>(key_of, n, h, hist, bc, T, need);
    block_take(key_of, n, T, need, wsum, [&](int r, unsigned k) {
      const int p = atomicAdd(&ccount, 1);       // any order: the ranks below put them in place
      ckey[p] = k;
      cidx[p] = r;
    });
  }
  __syncthreads();
  if (tid < h) {
    const unsigned k = ckey[tid];
    const int i = cidx[tid];
    int rank = 0;
    for (int j = 0; j < h; j++) rank += select_before(ckey[j], cidx[j], k, i) ? 1 : 0;
    sidx[rank] = i;
  }
  __syncthreads();
  if (tid < A.top) A.sel[(size_t)f * A.top + tid] = tid < h ? sidx[tid] : -1;
  if (tid == 0) {
    A.sel_counts[f] = h;
    A.votes[(size_t)f * A.nframes + f] = 0;
  }
  int4 *__restrict__ dst = reinterpret_cast<int4 *>(A.qsel + (size_t)f * A.hp * 128);
  for (int c = tid; c < A.hp * 8; c += SEL_WG) {
    const int row = c >> 3;
    int4 v = make_int4(0, 0, 0, 0);
    if (row < h) v = reinterpret_cast<const int4 *>(A.q + (base + sidx[row]) * 128)[c & 7];
    dst[c] = v;
  }
}

// blockDim.x = 64 * ceil(hp / 64): one wave per 64 rows of frame a = blockIdx.x; blockIdx.y = the strip of frames b.
__global__ __launch_bounds__(256) void select_votes_kernel(SelArgs A)
{
  __shared__ __attribute__((aligned(16))) unsigned char sB[SELECT_MAX_TOP * VOTE_ROW];   // b's rows, then the fold
  __shared__ unsigned colk[4][SELECT_MAX_TOP];   // per wave and column: (S << 6) | (63 - row within the wave), 0 = none
  __shared__ int wcnt[4];
  static_assert(4 * 16 * VOTE_RED * sizeof(uint2) <= sizeof(sB), "the fold fits the staging buffer");
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  const int N = A.nframes, hp = A.hp, nt = hp >> 5, nthreads = blockDim.x, nw = nthreads >> 6;
  const int a = blockIdx.x;
  const int b0 = a + 1 + blockIdx.y * A.strip, b1 = min(b0 + A.strip, N);
  if (b0 >= N) return;                           // uniform
  const int row0 = wave * 64;
  v4i af[2][4];
#pragma unroll
  for (int ai = 0; ai < 2; ai++) {
    const int row = row0 + 32 * ai + c;
    if (row < hp) {
      const v4i *p = reinterpret_cast<const v4i *>(A.qsel + ((size_t)a * hp + row) * 128 + 64 * h);
#pragma unroll
      for (int s = 0; s < 4; s++) af[ai][s] = p[s];
    } else {
#pragma unroll
      for (int s = 0; s < 4; s++) af[ai][s] = (v4i){0, 0, 0, 0};
    }
  }
  uint2 *const red = reinterpret_cast<uint2 *>(sB) + wave * 16 * VOTE_RED;
  // a frame's hp * 8 chunks of 16 bytes, at most 8 per thread, are fetched into registers one frame ahead, so that the
  // loads are in flight under the sweep and the fold of the frame before (a chunk past the end repeats the last one)
  v4i pre[8];
#define VOTE_FETCH(b)                                                                                      \
  {                                                                                                        \
    const v4i *__restrict__ src = reinterpret_cast<const v4i *>(A.qsel + (size_t)(b) * hp * 128);         \
    _Pragma("unroll") for (int i = 0; i < 8; i++) pre[i] = src[min(tid + i * nthreads, hp * 8 - 1)];       \
  }
  VOTE_FETCH(b0);
  for (int b = b0; b < b1; b++) {
    __syncthreads();                             // the previous frame's fold and counts have been read
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int q = tid + i * nthreads;
      if (q < hp * 8) *reinterpret_cast<v4i *>(sB + (q >> 3) * VOTE_ROW + (q & 7) * 16) = pre[i];
    }
    if (b + 1 < b1) VOTE_FETCH(b + 1);
    __syncthreads();
    unsigned k1[2][16], k2[2][16];
#pragma unroll
    for (int ai = 0; ai < 2; ai++)
#pragma unroll
      for (int r = 0; r < 16; r++) { k1[ai][r] = 0u; k2[ai][r] = 0u; }
    for (int t = 0; t < nt; t++) {
      const unsigned char *p = sB + (t * 32 + c) * VOTE_ROW + 64 * h;
      v4i bf[4];
#pragma unroll
      for (int s = 0; s < 4; s++) bf[s] = *reinterpret_cast<const v4i *>(p + 16 * s);
      v16i acc0 = {}, acc1 = {};
#pragma unroll
      for (int s = 0; s < 4; s++) {
        acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[0][s], bf[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[1][s], bf[s], acc1, 0, 0, 0);
      }
      const unsigned kc = VOTE_OFF + (unsigned)(VOTE_WIN - 1 - t);
      int pk = 0;                                // the column's best of the lane's 32 rows: (S << 5) | (31 - k)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const unsigned key0 = ((unsigned)acc0[r] << 9) + kc, key1 = ((unsigned)acc1[r] << 9) + kc;
        k2[0][r] = max(min(k1[0][r], k2[0][r]), min(max(k1[0][r], k2[0][r]), key0));
        k1[0][r] = max(k1[0][r], key0);
        k2[1][r] = max(min(k1[1][r], k2[1][r]), min(max(k1[1][r], k2[1][r]), key1));
        k1[1][r] = max(k1[1][r], key1);
        pk = max(pk, max((int)((unsigned)acc0[r] << 5) | (31 - r), (int)((unsigned)acc1[r] << 5) | (15 - r)));
      }
      const int s = pk >> 5, kk = 31 - (pk & 31);
      const int rl = 32 * (kk >> 4) + (kk & 3) + 8 * ((kk & 15) >> 2) + 4 * h;
      const unsigned mine = s > 0 ? ((unsigned)s << 6) | (unsigned)(63 - rl) : 0u;
      const unsigned other = (unsigned)__shfl_xor((int)mine, 32);
      if (h == 0) colk[wave][t * 32 + c] = max(mine, other);
    }
    __syncthreads();                             // every wave is through with sB; the column keys are complete
    int nvote = 0;
#pragma unroll
    for (int ai = 0; ai < 2; ai++) {
#pragma unroll
      for (int r = 0; r < 16; r++) red[r * VOTE_RED + lane] = make_uint2(k1[ai][r], k2[ai][r]);
      __syncthreads();
      // two lanes per row: lane l folds the columns 16 (l & 1) ... + 15 of every tile for row register (l >> 1) & 15 of
      // lane half l >> 5
      const int rowid = lane >> 1, part = lane & 1, r = rowid & 15, hh = rowid >> 4;
      int M = 0, I = -1, S2 = 0;
      for (int e = 0; e < 16; e++) {
        const int cl = 16 * part + e;
        const uint2 v = red[r * VOTE_RED + 32 * hh + cl];
        const bool v1 = v.x >= VOTE_VALID;
        const int s1 = v1 ? (int)((v.x - VOTE_OFF) >> 9) : 0;
        const int j1 = v1 ? (VOTE_WIN - 1 - (int)(v.x & (VOTE_WIN - 1))) * 32 + cl : -1;
        const int s2 = v.y >= VOTE_VALID ? (int)((v.y - VOTE_OFF) >> 9) : 0;
        vote_take(M, I, S2, s1, j1, s2);
      }
      const int Mo = __shfl_xor(M, 1), Io = __shfl_xor(I, 1), So = __shfl_xor(S2, 1);
      vote_take(M, I, S2, Mo, Io, So);
      const int gi = row0 + 32 * ai + (r & 3) + 8 * (r >> 2) + 4 * hh;       // the row within frame a's chosen records
      bool vote = false;
      if (part == 0 && I >= 0) {
        unsigned best = 0u;                      // (S << 8) | (255 - row): larger S, then the smaller row
        for (int w = 0; w < nw; w++) {
          const unsigned kw = colk[w][I];
          if (kw != 0u) best = max(best, ((kw >> 6) << 8) | (unsigned)(255 - (64 * w + 63 - (int)(kw & 63u))));
        }
        vote = 255 - (int)(best & 255u) == gi && select_vote(M, S2, A.min_score, A.max_ambiguity);
      }
      nvote += __popcll(__ballot(vote));
      __syncthreads();                           // red is rewritten by the second half / the next frame
    }
    if (lane == 0) wcnt[wave] = nvote;
    __syncthreads();
    if (tid == 0) {
      int v = 0;
      for (int w = 0; w < nw; w++) v += wcnt[w];
      A.votes[(size_t)a * N + b] = v;
      A.votes[(size_t)b * N + a] = v;
    }
  }
}

__global__ __launch_bounds__(SEL_WG) void select_pick_kernel(SelArgs A)
{
  __shared__ unsigned skey[SELECT_MAX_FRAMES];
  __shared__ unsigned hist[256], bc[2];
  __shared__ int wsum[SEL_WG / 64], tot[2];
  const int f = blockIdx.x, tid = threadIdx.x, N = A.nframes;
  const int *__restrict__ row = A.votes + (size_t)f * N;
  uint8_t *keep = A.keep + (size_t)f * N;
  if (tid == 0) { tot[0] = 0; tot[1] = 0; }
  __syncthreads();
  int cand = 0, vmax = 0;
  for (int g = tid; g < N; g += SEL_WG) {
    const int v = row[g];
    const unsigned key = select_neighbour_key(f, g, v, A.min_votes);
    skey[g] = key;
    cand += key != 0u ? 1 : 0;
    vmax = max(vmax, v);
    keep[g] = 0;
  }
  atomicAdd(&tot[0], cand);
  atomicMax(&tot[1], vmax);
  __syncthreads();
  const int h = min(tot[0], A.k);
  if (h > 0) {                                   // uniform over the workgroup
    auto key_of = [&](int g) { return skey[g]; };
    unsigned T;
    int need;
    block_threshold<2>(key_of, N, h, hist, bc, T, need);           // keys are votes: at most 256
    block_take(key_of, N, T, need, wsum, [&](int g, unsigned) { keep[g] = 1; });   // g's own thread cleared keep[g]
  }
  if (tid == 0) {
    const int cnt = A.set.counts[f];
    A.meta[f] = make_int4(cnt > 0 && h == 0 ? 1 : 0, tot[1], cnt > A.top ? 1 : 0, 0);
  }
}

__global__ __launch_bounds__(SEL_WG) void select_count_kernel(SelArgs A)
{
  __shared__ int tot;
  const int a = blockIdx.x, tid = threadIdx.x, N = A.nframes;
  if (tid == 0) tot = 0;
  __syncthreads();
  int cnt = 0;
  for (int b = a + 1 + tid; b < N; b += SEL_WG) cnt += (A.keep[(size_t)a * N + b] | A.keep[(size_t)b * N + a]) ? 1 : 0;
  atomicAdd(&tot, cnt);
  __syncthreads();
  if (tid == 0) A.rowcount[a] = tot;
}

__global__ __launch_bounds__(SEL_WG) void select_scan_kernel(SelArgs A)
{
  __shared__ int csum[SEL_WG], red[3];
  const int tid = threadIdx.x, N = A.nframes;
  const int per = (N + SEL_WG - 1) / SEL_WG, lo = min(tid * per, N), hi = min(lo + per, N);
  if (tid < 3) red[tid] = 0;
  __syncthreads();
  int sum = 0, lonely = 0, over = 0, vmax = 0;
  for (int f = lo; f < hi; f++) {
    const int4 m = A.meta[f];
    sum += A.rowcount[f];
    lonely += m.x;
    vmax = max(vmax, m.y);
    over += m.z;
  }
  csum[tid] = sum;
  atomicAdd(&red[0], lonely);
  atomicAdd(&red[1], over);
  atomicMax(&red[2], vmax);
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < SEL_WG; t++) {
      const int v = csum[t];
      csum[t] = run;
      run += v;
    }
    A.summary[0] = run;
    A.summary[1] = min(run, A.max_pairs);
    A.summary[2] = red[0];
    A.summary[3] = red[1];
    A.summary[4] = red[2];
    A.summary[5] = 0; A.summary[6] = 0; A.summary[7] = 0;
  }
  __syncthreads();
  int run = csum[tid];
  for (int f = lo; f < hi; f++) {
    A.rowoff[f] = run;
    run += A.rowcount[f];
  }
}

__global__ __launch_bounds__(SEL_WG) void select_emit_kernel(SelArgs A)
{
  __shared__ int wsum[SEL_WG / 64];
  const int a = blockIdx.x, tid = threadIdx.x, N = A.nframes;
  int at = A.rowoff[a];
  if (at >= A.max_pairs || A.rowcount[a] == 0) return;             // uniform: nothing of this row is written
  for (int base = a + 1; base < N; base += SEL_WG) {
    const int b = base + tid;
    const bool on = b < N && (A.keep[(size_t)a * N + b] | A.keep[(size_t)b * N + a]);
    int total;
    const int pos = at + block_rank(on, wsum, total);
    if (on && pos < A.max_pairs) {
      A.pairs[2 * (size_t)pos] = a;
      A.pairs[2 * (size_t)pos + 1] = b;
      A.pair_votes[pos] = A.votes[(size_t)a * N + b];
    }
    at += total;
  }
}

static size_t sel_align16(size_t v) { return (v + 15) / 16 * 16; }

// the temp of misift_select_pairs_batch: sized from nframes and top only
size_t select_pairs_tmp_bytes(int nframes, int top)
{
  const size_t N = (size_t)nframes, hp = (size_t)(top + 31) / 32 * 32;
  return sel_align16(N * hp * 128) + sel_align16(N * N) + 16 * N + 2 * sel_align16(4 * N) + 16;
}

// Enqueue misift_select_pairs_batch on the context stream (common.hpp): select, votes, pick, count, scan, emit.
int launch_select_pairs_batch(misift_ctx *ctx, const BatchLayout &set, const int8_t *q, int nframes, int top,
                              float min_score, float max_ambiguity, int min_votes, int k, int max_pairs, int *d_sel,
                              int *d_sel_counts, int *d_votes, int *d_pairs, int *d_pair_votes, int *d_summary)
{
  int rc = misift_ensure_tmp(ctx, select_pairs_tmp_bytes(nframes, top));
  if (rc) return rc;
  const size_t N = (size_t)nframes;
  SelArgs A;
  A.set = set; A.q = q; A.nframes = nframes; A.top = top; A.hp = (top + 31) / 32 * 32;
  A.min_score = min_score; A.max_ambiguity = max_ambiguity; A.min_votes = min_votes; A.k = k; A.max_pairs = max_pairs;
  A.sel = d_sel; A.sel_counts = d_sel_counts; A.votes = d_votes; A.pairs = d_pairs; A.pair_votes = d_pair_votes;
  A.summary = d_summary;
  char *t = reinterpret_cast<char *>(ctx->d_match_tmp);
  A.qsel = reinterpret_cast<int8_t *>(t);            t += sel_align16(N * A.hp * 128);
  A.keep = reinterpret_cast<uint8_t *>(t);           t += sel_align16(N * N);
  A.meta = reinterpret_cast<int4 *>(t);              t += 16 * N;
  A.rowcount = reinterpret_cast<int *>(t);           t += sel_align16(4 * N);
  A.rowoff = reinterpret_cast<int *>(t);
  // frames b per workgroup: long strips read frame a's rows once, short ones keep every CU busy on a small batch
  const int ncu = ctx->num_cus > 0 ? ctx->num_cus : 256;
  const long long npairs = (long long)nframes * (nframes - 1) / 2, slots = 8LL * VOTE_WG_PER_CU * ncu;
  long long strip = (npairs + slots - 1) / slots;
  A.strip = (int)(strip < 1 ? 1 : (strip > VOTE_MAX_STRIP ? VOTE_MAX_STRIP : strip));
  if (nframes > 0) {
    {
      LaunchScope ls(ctx, "select_gather");
      hipLaunchKernelGGL(select_gather_kernel, dim3(nframes), dim3(SEL_WG), 0, ctx->stream, A);
      rc = ls.finish();
      if (rc) return rc;
    }
    if (nframes > 1) {
      LaunchScope ls(ctx, "select_votes");
      const dim3 grid(nframes - 1, (nframes - 1 + A.strip - 1) / A.strip);
      hipLaunchKernelGGL(select_votes_kernel, grid, dim3(64 * ((A.hp + 63) / 64)), 0, ctx->stream, A);
      rc = ls.finish();
      if (rc) return rc;
    }
    {
      LaunchScope ls(ctx, "select_pick");
      hipLaunchKernelGGL(select_pick_kernel, dim3(nframes), dim3(SEL_WG), 0, ctx->stream, A);
      rc = ls.finish();
      if (rc) return rc;
    }
    {
      LaunchScope ls(ctx, "select_count");
      hipLaunchKernelGGL(select_count_kernel, dim3(nframes), dim3(SEL_WG), 0, ctx->stream, A);
      rc = ls.finish();
      if (rc) return rc;
    }
  }
  {
    LaunchScope ls(ctx, "select_scan");
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SEL_WG), 0, ctx->stream, A);
    rc = ls.finish();
    if (rc) return rc;
  }
  if (nframes > 1 && max_pairs > 0) {
    LaunchScope ls(ctx, "select_emit");
    hipLaunchKernelGGL(select_emit_kernel, dim3(nframes - 1), dim3(SEL_WG), 0, ctx->stream, A);
    rc = ls.finish();
  }
  return rc;
}

// host-only test hook (no device needed): misift_select_pairs_batch on host arrays, the rules of select_core.hpp applied
// with plain loops.  Writes exactly the bytes the device call writes.
extern "C" int misift_test_select_pairs(const void *recs_v, const int8_t *q, int nframes, const int *counts,
                                        const int *offsets, int stride, int top, float min_score, float max_ambiguity,
                                        int min_votes, int k, int max_pairs, int *sel, int *sel_counts, int *votes,
                                        int *pairs, int *pair_votes, int *summary)
{
  if (!recs_v || !q || !counts || !sel || !sel_counts || !votes || !pairs || !pair_votes || !summary || nframes < 0 ||
      nframes > SELECT_MAX_FRAMES || top < 1 || top > SELECT_MAX_TOP || min_votes < 1 || k < 1 || max_pairs < 0 ||
      min_score != min_score || max_ambiguity != max_ambiguity || (!offsets && stride < 0))
    return MISIFT_EINVAL;
  const SiftPointD *recs = reinterpret_cast<const SiftPointD *>(recs_v);
  const int N = nframes;
  int over = 0, lonely = 0, vmax = 0;
  // stage 1
  for (int f = 0; f < N; f++) {
    const int n = std::max(counts[f], 0);
    const long long base = offsets ? (long long)offsets[f] : (long long)f * stride;
    std::vector<int> order(n);
    for (int r = 0; r < n; r++) order[r] = r;
    std::sort(order.begin(), order.end(), [&](int x, int y) {
      return select_before(select_key(recs[base + x].scale), x, select_key(recs[base + y].scale), y);
    });
    const int h = std::min(n, top);
    for (int i = 0; i < top; i++) sel[(size_t)f * top + i] = i < h ? order[i] : -1;
    sel_counts[f] = h;
    over += n > top ? 1 : 0;
  }
  // stage 2
  std::vector<int> S((size_t)top * top);
  for (int a = 0; a < N; a++) {
    votes[(size_t)a * N + a] = 0;
    const long long base_a = offsets ? (long long)offsets[a] : (long long)a * stride;
    for (int b = a + 1; b < N; b++) {
      const long long base_b = offsets ? (long long)offsets[b] : (long long)b * stride;
      const int ha = sel_counts[a], hb = sel_counts[b];
      for (int i = 0; i < ha; i++)
        for (int j = 0; j < hb; j++) {
          const int8_t *x = q + (base_a + sel[(size_t)a * top + i]) * 128, *y = q + (base_b + sel[(size_t)b * top + j]) * 128;
          int s = 0;
          for (int d = 0; d < 128; d++) s += (int)x[d] * (int)y[d];
          S[(size_t)i * top + j] = s;
        }
      int v = 0;
      for (int i = 0; i < ha; i++) {
        int best = 0, m = -1, second = 0;
        for (int j = 0; j < hb; j++)
          if (S[(size_t)i * top + j] > best) { best = S[(size_t)i * top + j]; m = j; }
        if (m < 0) continue;
        for (int j = 0; j < hb; j++)
          if (j != m) second = std::max(second, S[(size_t)i * top + j]);
        int cbest = 0, crow = -1;                                    // column m's best row
        for (int r = 0; r < ha; r++)
          if (S[(size_t)r * top + m] > cbest) { cbest = S[(size_t)r * top + m]; crow = r; }
        if (crow == i && select_vote(best, second, min_score, max_ambiguity)) v++;
      }
      votes[(size_t)a * N + b] = v;
      votes[(size_t)b * N + a] = v;
      vmax = std::max(vmax, v);
    }
  }
  // stage 3
  std::vector<char> keep((size_t)N * N, 0);
  for (int f = 0; f < N; f++) {
    std::vector<int> order;
    for (int g = 0; g < N; g++)
      if (select_neighbour_key(f, g, votes[(size_t)f * N + g], min_votes) != 0u) order.push_back(g);
    std::sort(order.begin(), order.end(), [&](int x, int y) {
      return select_before((unsigned)votes[(size_t)f * N + x], x, (unsigned)votes[(size_t)f * N + y], y);
    });
    for (size_t i = 0; i < order.size() && i < (size_t)k; i++) keep[(size_t)f * N + order[i]] = 1;
    lonely += counts[f] > 0 && order.empty() ? 1 : 0;
  }
  int P = 0;
  for (int a = 0; a < N; a++)
    for (int b = a + 1; b < N; b++) {
      if (!(keep[(size_t)a * N + b] | keep[(size_t)b * N + a])) continue;
      if (P < max_pairs) {
        pairs[2 * (size_t)P] = a;
        pairs[2 * (size_t)P + 1] = b;
        pair_votes[P] = votes[(size_t)a * N + b];
      }
      P++;
    }
  summary[0] = P;
  summary[1] = std::min(P, max_pairs);
  summary[2] = lonely;
  summary[3] = over;
  summary[4] = vmax;
  summary[5] = summary[6] = summary[7] = 0;
  return MISIFT_OK;
}

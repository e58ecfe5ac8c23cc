// kernels_fundamental.hip — misift_find_fundamental_batch / misift_score_fundamental_batch /
// misift_improve_fundamental_batch: the epipolar counterpart of the homography batch calls (homography.hip).  Entry e
// works on frame frames[e] of a device-resident record batch (counts and offsets read on the device) and writes result
// slot e; no host round trip.  No reference counterpart: the
// reference's only geometric model is the homography.  The arithmetic is fundamental_core.hpp, shared with the host-only
// test hooks at the end of this file.
//
// Find, four launches whatever the number of entries (L = num_loops, Lp = L rounded up to 16):
//   gather  one 1024-thread workgroup per entry: the gather of homo_gather_kernel (SoA coordinates, ordered list of the
//           valid records) into the entry's temp, then wave 0 draws the entry's L x 8 sample positions from libc rand()
//           restated on the device (libc_rand.hpp), seeded with seeds[e].  Entries with fewer than 8 records, fewer than
//           8 valid records, or more than max_pts records are marked done here.
//   solve   one lane per (entry, hypothesis): the normalised 8-point solve with complete pivoting; each lane's 8x9
//           system lives in LDS (72 floats x 64 lanes = 18 KiB, word (r, c) of lane l at (9 r + c) * 64 + l: every
//           access of a wavefront hits 64 consecutive words whatever rows and columns the lanes have pivoted to).  Also
//           zeroes the entry's counts.
//   count   the hot path: one 64-lane workgroup per (entry, 64 hypotheses, 512-point chunk of the VALID records).  The
//           chunk's coordinates are staged once in LDS and read by broadcast; each lane holds one F in 9 registers and
//           tests every point of the chunk, then adds its count atomically (an integer sum: the order of the chunks does
//           not matter).
//   pick    one 1024-thread workgroup per entry: the largest count at the smallest hypothesis index -> F and the count;
//           nine zeros and 0 (or -1 over max_pts) for the entries the gather marked done.
// Score, one launch: one 256-thread workgroup per entry writes match_error of every record of the frame and counts the
// records that pass the gate and the inlier test.
// Improve, one launch: one 256-thread workgroup per entry refits F over its inliers (fundamental_refine), then writes what
// score writes under the result; see FB_STAGE below.
#include <math.h>
#include "common.hpp"
#include "fundamental_core.hpp"
#include "libc_rand.hpp"

namespace {

// what HOMO_CORE_GATHER (homography_core.inc) reads of a record
constexpr int OFF_XPOS = 0, OFF_YPOS = 1, OFF_SCORE = 6, OFF_AMBIG = 7, OFF_MXPOS = 9, OFF_MYPOS = 10;
constexpr int PT_WORDS = (int)(sizeof(SiftPointD) / sizeof(float));

constexpr int FB_CHUNK = 512;                  // valid points per count workgroup (8 KiB of LDS)
constexpr int FB_META = 4;                     // ints of meta per entry

struct FbArgs {
  BatchLayout set;
  const int *frames;                           // pinned host copies of the caller's lists
  const unsigned *seeds;
  int max_pts, mp16, num_loops, lp;            // mp16 = max_pts rounded up to 16; lp = num_loops rounded up to 16
  float min_score, max_ambiguity, thresh2;
  // temp, per entry e: coord[4 x mp16] | valid[mp16] | sample[8 x lp] | hyp[9 x lp] | hcount[lp] | meta[FB_META]
  float *coord;
  int *valid, *sample;
  float *hyp;
  int *hcount;
  int *meta;                                   // [0] valid records to count (0: entry done), [1] its result, [2] records
  float *F;                                    // out: nsel x 9
  int *num;                                    // out: nsel
};

__global__ __launch_bounds__(1024) void fund_batch_gather_kernel(FbArgs G)
{
  const int e = blockIdx.x;
  const int f = G.frames[e];
  const int n = G.set.counts[f];
  int *meta = G.meta + (size_t)FB_META * e;
  if (n < 8 || n > G.max_pts) {                // count -1 included; over max_pts: -1, nothing of the frame is read
    if (threadIdx.x == 0) { meta[0] = 0; meta[1] = n > G.max_pts ? -1 : 0; meta[2] = 0; }
    return;
  }
  const float *pts = reinterpret_cast<const float *>(G.set.recs + G.set.base(f));
  const int npts = n, stride = G.mp16;
  const float min_score = G.min_score, max_ambiguity = G.max_ambiguity;
  float *coord = G.coord + (size_t)e * 4 * G.mp16;
  int *valid = G.valid + (size_t)e * G.mp16;
#define HOMO_CORE_GATHER
#include "homography_core.inc"
#undef HOMO_CORE_GATHER
  const int num_valid = base_s;
  if (num_valid < 8) {
    if (tid == 0) { meta[0] = 0; meta[1] = 0; meta[2] = 0; }
    return;
  }
  if (tid < 64) {                              // wave 0: the entry's rand() stream, hypotheses one after another
    const int L = G.num_loops, lp = G.lp;
    int *sample = G.sample + (size_t)e * 8 * lp;
    LibcRand<LibcRandWaveRing> g;
    g.seed(G.seeds[e]);
    const FastMod31 fm((uint32_t)num_valid);
    for (int loop = 0; loop < L; loop++) {
      int p[8];
      fundamental_draw8(g, fm, p);
      if (tid == 0)
        for (int k = 0; k < 8; k++) sample[k * lp + loop] = p[k];
    }
    if (tid == 0) { meta[0] = num_valid; meta[1] = 0; meta[2] = npts; }
  }
}

// a lane's 8x9 system in LDS: word (r, c) at (9 r + c) * 64 from the lane's base
struct FundamentalLdsMat {
  float *base;
  __device__ float get(int r, int c) const { return base[(9 * r + c) * 64]; }
  __device__ void set(int r, int c, float v) { base[(9 * r + c) * 64] = v; }
};

__global__ __launch_bounds__(64) void fund_batch_solve_kernel(FbArgs G, int hblocks)
{
  __shared__ float s_m[72 * 64];
  const int e = blockIdx.x / hblocks;
  const int idx = (blockIdx.x % hblocks) * 64 + threadIdx.x;
  const int *meta = G.meta + (size_t)FB_META * e;
  const int num_valid = meta[0], npts = meta[2];
  if (num_valid == 0 || idx >= G.num_loops) return;
  const int lp = G.lp, mp = G.mp16;
  const float *coord = G.coord + (size_t)e * 4 * mp;
  const int *valid = G.valid + (size_t)e * mp;
  const int *sample = G.sample + (size_t)e * 8 * lp;
  G.hcount[(size_t)e * lp + idx] = 0;
  float x1[8], y1[8], x2[8], y2[8];
  bool in_range = true;                        // positions and record indices come from device memory: checked before use
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int pos = sample[k * lp + idx];
    const bool pos_ok = (unsigned)pos < (unsigned)num_valid;
    const int pt = valid[pos_ok ? pos : 0];
    const bool pt_ok = pos_ok && (unsigned)pt < (unsigned)npts;
    const int i = pt_ok ? pt : 0;
    in_range = in_range && pt_ok;
    x1[k] = coord[i]; y1[k] = coord[mp + i]; x2[k] = coord[2 * mp + i]; y2[k] = coord[3 * mp + i];
  }
  FundamentalLdsMat m{s_m + threadIdx.x};
  float F[9];
  fundamental_solve8(m, x1, y1, x2, y2, F);
  float *hyp = G.hyp + (size_t)e * 9 * lp;
#pragma unroll
  for (int k = 0; k < 9; k++) hyp[k * lp + idx] = in_range ? F[k] : 0.0f;
}

__global__ __launch_bounds__(64) void fund_batch_count_kernel(FbArgs G, int hblocks, int chunks)
{
  __shared__ float4 s_pt[FB_CHUNK];
  const int c = blockIdx.x % chunks, eh = blockIdx.x / chunks;
  const int e = eh / hblocks, hb = eh % hblocks;
  const int *meta = G.meta + (size_t)FB_META * e;
  const int num_valid = min(meta[0], G.mp16), npts = meta[2];
  const int i0 = c * FB_CHUNK;
  if (i0 >= num_valid) return;                 // beyond the valid records, or an entry already done (0)
  const int n = min(FB_CHUNK, num_valid - i0);
  const int lp = G.lp, mp = G.mp16;
  const float *coord = G.coord + (size_t)e * 4 * mp;
  const int *valid = G.valid + (size_t)e * mp + i0;
  for (int i = threadIdx.x; i < n; i += 64) {
    const int pt = valid[i];
    const int j = (unsigned)pt < (unsigned)npts ? pt : 0;
    s_pt[i] = make_float4(coord[j], coord[mp + j], coord[2 * mp + j], coord[3 * mp + j]);
  }
  __syncthreads();
  const int h = hb * 64 + threadIdx.x;
  if (h >= G.num_loops) return;
  const float *hyp = G.hyp + (size_t)e * 9 * lp;
  float F[9];
#pragma unroll
  for (int k = 0; k < 9; k++) F[k] = hyp[k * lp + h];
  const float thresh2 = G.thresh2;
  int cnt = 0;
  for (int i = 0; i < n; i++) {
    const float4 q = s_pt[i];
    float den;
    const float e2 = fundamental_sampson(F, q.x, q.y, q.z, q.w, den);
    cnt += fundamental_inlier(e2, den, thresh2) ? 1 : 0;
  }
  atomicAdd(&G.hcount[(size_t)e * lp + h], cnt);
}

__global__ __launch_bounds__(1024) void fund_batch_pick_kernel(FbArgs G)
{
  const int e = blockIdx.x;
  float *F = G.F + (size_t)9 * e;
  const int *meta = G.meta + (size_t)FB_META * e;
  if (meta[0] == 0) {                          // nine zeros and 0, or -1 for a frame over max_pts
    if (threadIdx.x < 9) F[threadIdx.x] = 0.0f;
    if (threadIdx.x == 0) G.num[e] = meta[1];
    return;
  }
  const int num_loops = G.num_loops;
  const int *counts = G.hcount + (size_t)e * G.lp;
#define HOMO_CORE_PICK
#include "homography_core.inc"
#undef HOMO_CORE_PICK
  if (tid == 0) {
    const int idx = 0x7fffffff - (int)(unsigned)(best & 0xffffffffull);
    const float *hyp = G.hyp + (size_t)e * 9 * G.lp;
    for (int k = 0; k < 9; k++) F[k] = hyp[k * G.lp + idx];
    G.num[e] = (int)(best >> 32);
  }
}

struct FbScoreArgs {
  BatchLayout set;
  const int *frames;                           // pinned host copy
  float min_score, max_ambiguity, thresh2;
  const float *F;                              // nsel x 9
  int *num_fit;
};

__global__ __launch_bounds__(256) void fund_batch_score_kernel(FbScoreArgs B)
{
  __shared__ int s_fit[4];
  const int e = blockIdx.x, f = B.frames[e];
  const int n = max(B.set.counts[f], 0);
  SiftPointD *pts = B.set.recs + B.set.base(f);
  float F[9];
#pragma unroll
  for (int k = 0; k < 9; k++) F[k] = B.F[(size_t)9 * e + k];
  int fit = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    SiftPointD &pt = pts[i];
    float den;
    const float e2 = fundamental_sampson(F, pt.xpos, pt.ypos, pt.match_xpos, pt.match_ypos, den);
    const bool gate = pt.score > B.min_score && pt.ambiguity < B.max_ambiguity;
    fit += gate && fundamental_inlier(e2, den, B.thresh2) ? 1 : 0;
    pt.match_error = fundamental_error(e2, den);
  }
  for (int off = 32; off > 0; off >>= 1) fit += __shfl_xor(fit, off, 64);
  if ((threadIdx.x & 63) == 0) s_fit[threadIdx.x >> 6] = fit;
  __syncthreads();
  if (threadIdx.x == 0) B.num_fit[e] = s_fit[0] + s_fit[1] + s_fit[2] + s_fit[3];
}

// Improve, one launch: one 256-thread workgroup per entry runs fundamental_refine with thread t as slot t of the call's
// sum.  The four coordinates and the gate of the frame's first FB_STAGE records are staged in LDS once (the sign of
// nothing is touched: the gate sits in a byte of its own); a record beyond them is read from global memory in every
// pass, all of it within the record's first 64 bytes.  The 9x9 solve is spread over 81 threads, one per matrix entry
// (fundamental_lane_step): on one thread with the matrix in LDS it took 52 of the 58 us of a round.
constexpr int FB_STAGE = 4096;

struct FbImproveArgs {
  BatchLayout set;
  const int *frames;                           // pinned host copy
  int num_loops;
  float min_score, max_ambiguity, thresh2;
  float *F;                                    // in/out: nsel x 9
  int *num_fit, *num_rounds;                   // num_rounds may be NULL
};

struct FbStagedRecs {
  const float4 *xy;                            // LDS: the first min(n, FB_STAGE) records
  const unsigned char *gate;
  const SiftPointD *pts;
  float min_score, max_ambiguity;
  __device__ bool load(int r, float &x1, float &y1, float &x2, float &y2) const
  {
    if (r < FB_STAGE) {
      const float4 q = xy[r];
      x1 = q.x; y1 = q.y; x2 = q.z; y2 = q.w;
      return gate[r] != 0;
    }
    const SiftPointD &pt = pts[r];
    x1 = pt.xpos; y1 = pt.ypos; x2 = pt.match_xpos; y2 = pt.match_ypos;
    return pt.score > min_score && pt.ambiguity < max_ambiguity;
  }
};

struct FbBlockExec {
  float *p;                                    // LDS: FUND_MOMENTS x FUND_SLOTS
  float *m;                                    // LDS: the 81 entries of the solve
  unsigned long long *key, *rowkey;            // LDS: 81 and 9 pivot keys
  int *cnt;                                    // LDS: 4 ints
  template <int K, class V>
  __device__ void sum(int n, V &v, float (&out)[K])
  {
    const int t = threadIdx.x;
    float acc[K];
    fundamental_slot_partial<K>(t, n, v, acc);
#pragma unroll
    for (int k = 0; k < K; k++) p[k * FUND_SLOTS + t] = acc[k];
    for (int off = FUND_SLOTS / 2; off > 0; off >>= 1) {
      __syncthreads();
      if (t < off) fundamental_tree_step<K>(p, t, off);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) out[k] = p[k * FUND_SLOTS];
    __syncthreads();                           // p is free again
  }
  template <class P>
  __device__ int count(int n, P pred)
  {
    int c = 0;
    for (int r = threadIdx.x; r < n; r += FUND_SLOTS) c += pred(r) ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    c = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    __syncthreads();
    return c;
  }
  // the 9x9 solve on 81 threads, thread t owning entry (t / 9, t % 9) in a register; every thread ends with the result
  __device__ bool solve(const float (&M)[FUND_MOMENTS], float c1x, float c1y, float s1, float c2x, float c2y, float s2,
                        float (&Fp)[9])
  {
    const int t = threadIdx.x, tt = min(t, 80);
    const int lo = min(tt / 9, tt % 9), hi = max(tt / 9, tt % 9);
    float a = 0.0f;
    {
      int i = 0;
#pragma unroll
      for (int p = 0; p < 9; p++)
#pragma unroll
        for (int q = p; q < 9; q++) {
          a = (p == lo && q == hi) ? M[i] : a;
          i++;
        }
    }
    int col[9];
#pragma unroll
    for (int j = 0; j < 9; j++) col[j] = j;
    bool ok = true;
    for (int k = 0; k < 8; k++) {
      if (t < 81) {
        m[t] = a;
        key[t] = fundamental_pivot_key(a, t, k);
      }
      __syncthreads();
      if (t < 9) rowkey[t] = fundamental_row_key(key, t);
      __syncthreads();
      int pc;
      float piv;
      a = fundamental_lane_step(m, rowkey, tt, k, pc, piv);
      ok = ok && piv != 0.0f && fundamental_finite(piv);
      fundamental_swap_columns(col, k, pc);
      __syncthreads();                         // m, key and rowkey are free again
    }
    if (t < 81) m[t] = a;
    __syncthreads();
    const FundamentalSquareMat mat{m};
    float nf[9];
    fundamental_back_substitute(mat, col, nf);
    ok = fundamental_denormalise(nf, c1x, c1y, s1, c2x, c2y, s2, Fp) && ok;
    __syncthreads();
    return ok;
  }
};

__global__ __launch_bounds__(FUND_SLOTS) void fund_batch_improve_kernel(FbImproveArgs B)
{
  __shared__ float4 s_xy[FB_STAGE];
  __shared__ unsigned char s_gate[FB_STAGE];
  __shared__ float s_p[FUND_MOMENTS * FUND_SLOTS];
  __shared__ float s_m[81];
  __shared__ unsigned long long s_key[81], s_rowkey[9];
  __shared__ int s_cnt[4];
  const int e = blockIdx.x, f = B.frames[e];
  const int n = max(B.set.counts[f], 0);
  SiftPointD *pts = B.set.recs + B.set.base(f);
  for (int i = threadIdx.x; i < min(n, FB_STAGE); i += FUND_SLOTS) {
    const SiftPointD &pt = pts[i];
    s_xy[i] = make_float4(pt.xpos, pt.ypos, pt.match_xpos, pt.match_ypos);
    s_gate[i] = pt.score > B.min_score && pt.ambiguity < B.max_ambiguity ? 1 : 0;
  }
  __syncthreads();
  float F[9];
#pragma unroll
  for (int k = 0; k < 9; k++) F[k] = B.F[(size_t)9 * e + k];
  FbBlockExec ex{s_p, s_m, s_key, s_rowkey, s_cnt};
  const FbStagedRecs recs{s_xy, s_gate, pts, B.min_score, B.max_ambiguity};
  int c, rounds;
  fundamental_refine(ex, recs, n, B.thresh2, B.num_loops, F, c, rounds);
  for (int i = threadIdx.x; i < n; i += FUND_SLOTS) {
    float x1, y1, x2, y2, den;
    recs.load(i, x1, y1, x2, y2);
    const float e2 = fundamental_sampson(F, x1, y1, x2, y2, den);
    pts[i].match_error = fundamental_error(e2, den);
  }
  if (threadIdx.x < 9) B.F[(size_t)9 * e + threadIdx.x] = F[threadIdx.x];
  if (threadIdx.x == 0) {
    B.num_fit[e] = c;
    if (B.num_rounds) B.num_rounds[e] = rounds;
  }
}

size_t round16(size_t v) { return (v + 15) / 16 * 16; }

}  // namespace

size_t find_fundamental_batch_tmp_bytes(int nsel, int max_pts, int num_loops)
{
  const size_t mp = round16((size_t)max_pts), lp = round16((size_t)num_loops);
  return (size_t)nsel * (sizeof(float) * 4 * mp + sizeof(int) * mp + sizeof(int) * 8 * lp + sizeof(float) * 9 * lp +
                         sizeof(int) * lp + sizeof(int) * FB_META);
}

int launch_find_fundamental_batch(misift_ctx *ctx, int nsel, const int *h_frames, const unsigned *h_seeds,
                                  const BatchLayout &set, int max_pts, int num_loops, float min_score,
                                  float max_ambiguity, float thresh, float *F, int *num)
{
  FbArgs G;
  G.set = set;
  G.frames = h_frames; G.seeds = h_seeds;
  G.max_pts = max_pts;
  G.mp16 = (int)round16((size_t)max_pts);
  G.num_loops = num_loops;
  G.lp = (int)round16((size_t)num_loops);
  G.min_score = min_score; G.max_ambiguity = max_ambiguity; G.thresh2 = thresh * thresh;
  const size_t mp = (size_t)G.mp16, lp = (size_t)G.lp, ns = (size_t)nsel;
  const int hblocks = (num_loops + 63) / 64, chunks = (int)((mp + FB_CHUNK - 1) / FB_CHUNK);
  if ((long long)nsel * hblocks * chunks > 0x7fffffffLL) {
    misift_set_error("misift_find_fundamental_batch: %d entries x %d loops x %d points is beyond one launch", nsel,
                     num_loops, max_pts);
    return MISIFT_EINVAL;
  }
  int rc = misift_ensure_tmp(ctx, find_fundamental_batch_tmp_bytes(nsel, max_pts, num_loops));
  if (rc) return rc;
  G.coord = reinterpret_cast<float *>(ctx->d_match_tmp);
  G.valid = reinterpret_cast<int *>(G.coord + ns * 4 * mp);
  G.sample = G.valid + ns * mp;
  G.hyp = reinterpret_cast<float *>(G.sample + ns * 8 * lp);
  G.hcount = reinterpret_cast<int *>(G.hyp + ns * 9 * lp);
  G.meta = G.hcount + ns * lp;
  G.F = F; G.num = num;
  {
    LaunchScope ls(ctx, "fund_batch_gather");
    hipLaunchKernelGGL(fund_batch_gather_kernel, dim3(nsel), dim3(1024), 0, ctx->stream, G);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, "fund_batch_solve");
    hipLaunchKernelGGL(fund_batch_solve_kernel, dim3(nsel * hblocks), dim3(64), 0, ctx->stream, G, hblocks);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, "fund_batch_count");
    hipLaunchKernelGGL(fund_batch_count_kernel, dim3(nsel * hblocks * chunks), dim3(64), 0, ctx->stream, G, hblocks,
                       chunks);
    rc = ls.finish();
    if (rc) return rc;
  }
  LaunchScope ls(ctx, "fund_batch_pick");
  hipLaunchKernelGGL(fund_batch_pick_kernel, dim3(nsel), dim3(1024), 0, ctx->stream, G);
  return ls.finish();
}

int launch_score_fundamental_batch(misift_ctx *ctx, int nsel, const int *h_frames, const BatchLayout &set,
                                   float min_score, float max_ambiguity, float thresh, const float *F, int *num_fit)
{
  FbScoreArgs B;
  B.set = set;
  B.frames = h_frames;
  B.min_score = min_score; B.max_ambiguity = max_ambiguity; B.thresh2 = thresh * thresh;
  B.F = F; B.num_fit = num_fit;
  LaunchScope ls(ctx, "fund_batch_score");
  hipLaunchKernelGGL(fund_batch_score_kernel, dim3(nsel), dim3(256), 0, ctx->stream, B);
  return ls.finish();
}

int launch_improve_fundamental_batch(misift_ctx *ctx, int nsel, const int *h_frames, const BatchLayout &set,
                                     int num_loops, float min_score, float max_ambiguity, float thresh, float *F,
                                     int *num_fit, int *num_rounds)
{
  FbImproveArgs B;
  B.set = set;
  B.frames = h_frames;
  B.num_loops = num_loops;
  B.min_score = min_score; B.max_ambiguity = max_ambiguity; B.thresh2 = thresh * thresh;
  B.F = F; B.num_fit = num_fit; B.num_rounds = num_rounds;
  LaunchScope ls(ctx, "fund_batch_improve");
  hipLaunchKernelGGL(fund_batch_improve_kernel, dim3(nsel), dim3(FUND_SLOTS), 0, ctx->stream, B);
  return ls.finish();
}

// Test-only, host-only: the sample draw, the 8-point solve, the Sampson terms and match_error as the kernels compute
// them (libc_rand.hpp, fundamental_core.hpp).
extern "C" int misift_test_fundamental_samples(unsigned seed, int num_valid, int num_loops, int *out)
{
  if (num_valid < 8 || num_loops < 0 || (num_loops > 0 && !out)) {
    misift_set_error("misift_test_fundamental_samples: invalid argument");
    return MISIFT_EINVAL;
  }
  LibcRand<LibcRandArrayRing> g;
  g.seed(seed);
  const FastMod31 fm((uint32_t)num_valid);
  for (int loop = 0; loop < num_loops; loop++) {
    int p[8];
    fundamental_draw8(g, fm, p);
    for (int k = 0; k < 8; k++) out[8 * loop + k] = p[k];
  }
  return MISIFT_OK;
}

extern "C" int misift_test_fundamental_solve(const float *xy, float *F9, int *valid)
{
  if (!xy || !F9 || !valid) {
    misift_set_error("misift_test_fundamental_solve: invalid argument");
    return MISIFT_EINVAL;
  }
  float x1[8], y1[8], x2[8], y2[8], F[9];
  for (int k = 0; k < 8; k++) { x1[k] = xy[4 * k]; y1[k] = xy[4 * k + 1]; x2[k] = xy[4 * k + 2]; y2[k] = xy[4 * k + 3]; }
  FundamentalArrayMat m;
  *valid = fundamental_solve8(m, x1, y1, x2, y2, F) ? 1 : 0;
  for (int k = 0; k < 9; k++) F9[k] = F[k];
  return MISIFT_OK;
}

extern "C" int misift_test_fundamental_sampson(const float *F9, const float *xy, int n, float *e2_out, float *den_out)
{
  if (!F9 || n < 0 || (n > 0 && (!xy || !e2_out || !den_out))) {
    misift_set_error("misift_test_fundamental_sampson: invalid argument");
    return MISIFT_EINVAL;
  }
  float F[9];
  for (int k = 0; k < 9; k++) F[k] = F9[k];
  for (int i = 0; i < n; i++)
    e2_out[i] = fundamental_sampson(F, xy[4 * i], xy[4 * i + 1], xy[4 * i + 2], xy[4 * i + 3], den_out[i]);
  return MISIFT_OK;
}

extern "C" int misift_test_fundamental_error(const float *e2, const float *den, int n, float *out)
{
  if (n < 0 || (n > 0 && (!e2 || !den || !out))) {
    misift_set_error("misift_test_fundamental_error: invalid argument");
    return MISIFT_EINVAL;
  }
  for (int i = 0; i < n; i++) out[i] = fundamental_error(e2[i], den[i]);
  return MISIFT_OK;
}

extern "C" int misift_test_fundamental_refine(const float *xy, const unsigned char *gate, int n, const float *F9_in,
                                              float thresh, int num_loops, float *F9_out, int *num_fit, int *num_rounds)
{
  if (n < 0 || (n > 0 && (!xy || !gate)) || !F9_in || num_loops < 0 || !F9_out || !num_fit || !num_rounds) {
    misift_set_error("misift_test_fundamental_refine: invalid argument");
    return MISIFT_EINVAL;
  }
  float F[9];
  for (int k = 0; k < 9; k++) F[k] = F9_in[k];
  FundamentalHostExec *ex = new FundamentalHostExec;
  const FundamentalHostRecs recs{xy, gate};
  fundamental_refine(*ex, recs, n, thresh * thresh, num_loops, F, *num_fit, *num_rounds);
  delete ex;
  for (int k = 0; k < 9; k++) F9_out[k] = F[k];
  return MISIFT_OK;
}

extern "C" int misift_test_fundamental_solve9(const float *M81, int lanes, float *n9, int *valid)
{
  if (!M81 || !n9 || !valid || lanes < 0 || lanes > 1) {
    misift_set_error("misift_test_fundamental_solve9: invalid argument");
    return MISIFT_EINVAL;
  }
  float a[81], n[9];
  for (int k = 0; k < 81; k++) a[k] = M81[k];
  FundamentalSquareMat m{a};
  *valid = (lanes ? fundamental_eliminate_lanes(a, n) : fundamental_eliminate<9>(m, n)) ? 1 : 0;
  for (int k = 0; k < 9; k++) n9[k] = n[k];
  return MISIFT_OK;
}

extern "C" int misift_test_fundamental_refine_capacity(void) { return FB_STAGE; }

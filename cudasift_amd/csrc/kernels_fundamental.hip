// kernels_fundamental.hip — misift_find_fundamental_batch / misift_score_fundamental_batch /
// misift_improve_fundamental_batch: the epipolar counterpart of the homography batch calls (homography.hip).  Entry e
// works on frame frames[e] of a device-resident record batch (counts and offsets read on the device) and writes result
// slot e; no host round trip.  No reference counterpart: the reference's only geometric model is the homography.  The
// arithmetic is fundamental_core.hpp, shared with the host-only test hooks at the end of this file.
//
// Find is the shared batch search of ransac_batch.hpp (gather + draw, solve, count, pick) with the model below: it works
// over exactly num_loops hypotheses of 8 positions each, counts with the Sampson test over the VALID records only, and
// gives nine zeros to the entries the gather marked done.  The solve is this file's: one lane per (entry, hypothesis)
// runs the normalised 8-point solve with complete pivoting; each lane's 8x9 system lives in LDS (72 floats x 64 lanes =
// 18 KiB, word (r, c) of lane l at (9 r + c) * 64 + l: every access of a wavefront hits 64 consecutive words whatever
// rows and columns the lanes have pivoted to).
// Score, one launch: one 256-thread workgroup per entry writes match_error of every record of the frame and counts the
// records that pass the gate and the inlier test.
// Improve, one launch: one 256-thread workgroup per entry refits F over its inliers (fundamental_refine), then writes what
// score writes under the result; see FB_STAGE below.
#include <math.h>
#include "common.hpp"
#include "fundamental_core.hpp"
#include "libc_rand.hpp"
#include "ransac_batch.hpp"

namespace {

struct FundamentalModel : RansacPlainLane {
  typedef RansacArgs Args;
  static constexpr int SAMPLE = 8, PARAMS = 9, COORDS = 4;
  static constexpr bool INDEX = true;          // the valid records
  static constexpr bool COUNT_ALL = false;     // only the records that pass the gate vote
  template <class Ring>
  static __device__ __forceinline__ void draw(LibcRand<Ring> &g, const FastMod31 &fm, int (&p)[8])
  {
    fundamental_draw8(g, fm, p);
  }
  static __device__ __forceinline__ bool inlier(const float (&F)[9], Lane, const float (&q)[4], float thresh2)
  {
    float den;
    const float e2 = fundamental_sampson(F, q[0], q[1], q[2], q[3], den);
    return fundamental_inlier(e2, den, thresh2);
  }
  static __device__ __forceinline__ float invalid() { return 0.0f; }
  static __device__ __forceinline__ float done(int) { return 0.0f; }
  static __device__ __forceinline__ void picked(float *) {}
};

// a lane's 8x9 system in LDS: word (r, c) at (9 r + c) * 64 from the lane's base
struct FundamentalLdsMat {
  float *base;
  __device__ float get(int r, int c) const { return base[(9 * r + c) * 64]; }
  __device__ void set(int r, int c, float v) { base[(9 * r + c) * 64] = v; }
};

__global__ __launch_bounds__(64) void fund_batch_solve_kernel(RansacArgs G, int hblocks)
{
  __shared__ float s_m[72 * 64];
  const RansacSearch &S = G.rs;
  int e, idx, num_valid;
  if (!ransac_solve_begin(S, hblocks, e, idx, num_valid)) return;
  const int npts = S.meta[(size_t)RANSAC_META * e + 2], mp = S.cap16;
  const float *coord = S.coord + (size_t)e * 4 * mp;
  const int *valid = S.index + (size_t)e * mp;
  float x1[8], y1[8], x2[8], y2[8];
  bool in_range = true;                        // the record indices come from device memory too: checked before use
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int pt = valid[ransac_sample_position<FundamentalModel>(S, e, idx, k, num_valid, in_range)];
    const bool pt_ok = (unsigned)pt < (unsigned)npts;
    const int i = pt_ok ? pt : 0;
    in_range = in_range && pt_ok;
    x1[k] = coord[i]; y1[k] = coord[mp + i]; x2[k] = coord[2 * mp + i]; y2[k] = coord[3 * mp + i];
  }
  FundamentalLdsMat m{s_m + threadIdx.x};
  float F[9];
  fundamental_solve8(m, x1, y1, x2, y2, F);
  ransac_store_hyp<FundamentalModel>(S, e, idx, in_range, F);
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

}  // namespace

int launch_find_fundamental_batch(misift_ctx *ctx, int nsel, const int *h_frames, const unsigned *h_seeds,
                                  const BatchLayout &set, int max_pts, int num_loops, float min_score,
                                  float max_ambiguity, float thresh, float *F, int *num)
{
  const RansacNames names{"misift_find_fundamental_batch", "points", "fund_batch_gather", "fund_batch_solve",
                          "fund_batch_count", "fund_batch_pick"};
  return ransac_batch_run<FundamentalModel>(ctx, names, nsel, h_frames, h_seeds, set, max_pts, num_loops, min_score,
                                            max_ambiguity, thresh, F, num, fund_batch_solve_kernel);
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
  ransac_host_samples(seed, num_valid, num_loops, out, fundamental_draw8<LibcRandArrayRing>);
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

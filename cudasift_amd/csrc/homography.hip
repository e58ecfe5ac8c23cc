// homography.hip — RANSAC homography over stored matches, on the GPU (SURVEY §8f "next" row 1).
//
// Replaces FindHomography (reference matching.cu:1000-1087) and its kernels
// ComputeHomographies (:907-948, 8x8 solve through InvertMatrix<8> :821-905) and
// TestHomographies (:953-996).  Arithmetic follows oracle/sift_oracle.c orc_find_homography
// operation by operation (explicit fmaf where the reference's expressions contract, exact
// round-toward-zero products where it uses __fmul_rz), so H and the inlier count are
// bit-identical to the oracle for the same libc rand() state.
//
// MI355X shape (latency-bound, a few k points x ~10 k hypotheses):
//   gather   one workgroup: AoS SiftPoint -> SoA coords + ORDERED list of valid points
//            (ballot/popcount compaction keeps index order, which the rand()%numValid
//            sampling depends on); numValid goes back to the host (4 bytes).
//   host     draws the 4 sample indices per hypothesis with libc rand() in the reference's
//            call order (matching.cu:1041-1053) and uploads them.
//   solve    one lane per hypothesis: 8x8 Crout LU with implicit row scaling, inverse by
//            8 unit-vector solves, h = inv(A) b.
//   count    one wavefront per hypothesis sweeps all points (coalesced SoA reads, L2
//            resident), ballot+popcount accumulate -> count[hyp].
//   pick     one workgroup: first hypothesis with the largest count; 8 floats + count D2H.
//
// Deviation: the reference counts inliers over numPts rounded up to 16
// and so reads up to 15 uninitialised coordinates; here exactly numPts points are tested.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "common.hpp"
#include "libc_rand.hpp"

namespace {

constexpr int OFF_XPOS = 0, OFF_YPOS = 1, OFF_SCORE = 6, OFF_AMBIG = 7, OFF_MXPOS = 9, OFF_MYPOS = 10;
constexpr int PT_WORDS = (int)(sizeof(SiftPointD) / sizeof(float));

__device__ __forceinline__ float mul_rz(float a, float b)
{
  // exact round-toward-zero product: RN product, then step one ulp toward zero when the exact
  // residual says RN rounded away from zero
  float p = a * b;
  const float e = fmaf(a, b, -p);
  const bool away = (p > 0.0f && e < 0.0f) || (p < 0.0f && e > 0.0f);
  return away ? __uint_as_float(__float_as_uint(p) - 1u) : p;
}

// ---- gather: SoA coordinates + ordered compaction of the valid points -------------------------
__global__ __launch_bounds__(1024) void homo_gather_kernel(const float *__restrict__ pts, int npts, int stride,
                                                             float min_score, float max_ambiguity,
                                                             float *__restrict__ coord, int *__restrict__ valid,
                                                             int *__restrict__ num_valid)
{
#define HOMO_CORE_GATHER
#include "homography_core.inc"
#undef HOMO_CORE_GATHER
  if (tid == 0) *num_valid = base_s;
}

// ---- solve: one lane per hypothesis -------------------------------------------------------------
// Crout LU with implicit scaling of an 8x8 system, in place; perm[] records the row swaps.
__device__ void lu8(float (&m)[8][8], int (&perm)[8])
{
  float rowscale[8];
  for (int r = 0; r < 8; r++) {
    float big = 0.0f;
    for (int c = 0; c < 8; c++) big = fmaxf(big, fabsf(m[r][c]));
    rowscale[r] = big > 0.0f ? 1.0f / big : 1e16f;
  }
  int piv = 0;
  for (int c = 0; c < 8; c++) {
    for (int r = 0; r < c; r++) {
      float s = m[r][c];
      for (int k = 0; k < r; k++) s = fmaf(-m[r][k], m[k][c], s);
      m[r][c] = s;
    }
    float best = 0.0f;
    for (int r = c; r < 8; r++) {
      float s = m[r][c];
      for (int k = 0; k < c; k++) s = fmaf(-m[r][k], m[k][c], s);
      m[r][c] = s;
      const float merit = rowscale[r] * fabsf(s);
      if (merit >= best) { best = merit; piv = r; }
    }
    if (piv != c) {
      for (int k = 0; k < 8; k++) { const float t = m[piv][k]; m[piv][k] = m[c][k]; m[c][k] = t; }
      rowscale[piv] = rowscale[c];
    }
    perm[c] = piv;
    if (m[c][c] == 0.0f) m[c][c] = 1e-16f;
    if (c != 7) {
      const float inv = 1.0f / m[c][c];
      for (int r = c + 1; r < 8; r++) m[r][c] *= inv;
    }
  }
}

// column `col` of the inverse from the LU factors (forward + back substitution of e_col)
__device__ void lu8_unit_solve(const float (&m)[8][8], const int (&perm)[8], int col, float (&x)[8])
{
  for (int k = 0; k < 8; k++) x[k] = 0.0f;
  x[col] = 1.0f;
  int first = -1;
  for (int r = 0; r < 8; r++) {
    const int p = perm[r];
    float s = x[p];
    x[p] = x[r];
    if (first != -1) {
      for (int k = first; k < r; k++) s = fmaf(-m[r][k], x[k], s);
    } else if (s != 0.0f) {
      first = r;
    }
    x[r] = s;
  }
  for (int r = 7; r >= 0; r--) {
    float s = x[r];
    for (int k = r + 1; k < 8; k++) s = fmaf(-m[r][k], x[k], s);
    x[r] = s / m[r][r];
  }
}

__global__ __launch_bounds__(64) void homo_solve_kernel(const float *__restrict__ coord, int stride,
                                                          const int *__restrict__ valid, const int *__restrict__ sample,
                                                          int num_loops, float *__restrict__ homo)
{
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= num_loops) return;
#define HOMO_CORE_SOLVE
#include "homography_core.inc"
#undef HOMO_CORE_SOLVE
}

// ---- count: one wavefront per hypothesis ---------------------------------------------------------
__global__ __launch_bounds__(256) void homo_count_kernel(const float *__restrict__ coord, int stride, int npts,
                                                           const float *__restrict__ homo, int num_loops,
                                                           float thresh2, int *__restrict__ counts)
{
  const int lane = threadIdx.x & 63;
  const int hyp = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (hyp >= num_loops) return;
  float a[8];
  for (int k = 0; k < 8; k++) a[k] = homo[k * num_loops + hyp];
  int cnt = 0;
  for (int i = lane; i < npts; i += 64) {
    const float x1 = coord[0 * stride + i], y1 = coord[1 * stride + i];
    const float x2 = coord[2 * stride + i], y2 = coord[3 * stride + i];
#define HOMO_CORE_INLIER
#include "homography_core.inc"
#undef HOMO_CORE_INLIER
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if (lane == 0) counts[hyp] = cnt;
}

// ---- pick: first hypothesis with the largest count (strict '>' scan of matching.cu:1063-1068) ----
__global__ __launch_bounds__(1024) void homo_pick_kernel(const int *__restrict__ counts, const float *__restrict__ homo,
                                                           int num_loops, float *__restrict__ result)
{
#define HOMO_CORE_PICK
#include "homography_core.inc"
#undef HOMO_CORE_PICK
  if (tid == 0) {
    const int idx = 0x7fffffff - (int)(unsigned)(best & 0xffffffffull);
    for (int k = 0; k < 8; k++) result[k] = homo[k * num_loops + idx];
    reinterpret_cast<int *>(result)[8] = (int)(best >> 32);
    reinterpret_cast<int *>(result)[9] = idx;
  }
}

}  // namespace

extern "C" int misift_find_homography(misift_ctx *ctx, const void *d_pts, int npts, float *homography, int *num_matches,
                                      int num_loops, float min_score, float max_ambiguity, float thresh)
{
  if (!ctx || !homography || !num_matches || num_loops < 1) {
    misift_set_error("misift_find_homography: invalid argument");
    return MISIFT_EINVAL;
  }
  *num_matches = 0;
  homography[0] = homography[4] = homography[8] = 1.0f;
  homography[1] = homography[2] = homography[3] = 0.0f;
  homography[5] = homography[6] = homography[7] = 0.0f;
  if (!d_pts || npts < 8) return MISIFT_OK;                        // matching.cu:1008, :1016-1017
  num_loops = (num_loops + 15) / 16 * 16;
  const int stride = (npts + 15) / 16 * 16;
  // temp layout: coord[4*stride] | valid[stride] | sample[4*loops] | homo[8*loops] | counts[loops] | result[16]
  const size_t words = (size_t)5 * stride + (size_t)13 * num_loops + 16 + 16;
  int rc = misift_ensure_tmp(ctx, words * sizeof(float));
  if (rc) return rc;
  float *coord = reinterpret_cast<float *>(ctx->d_match_tmp);
  int *valid = reinterpret_cast<int *>(coord + (size_t)4 * stride);
  int *sample = valid + stride;
  float *homo = reinterpret_cast<float *>(sample + (size_t)4 * num_loops);
  int *counts = reinterpret_cast<int *>(homo + (size_t)8 * num_loops);
  float *result = reinterpret_cast<float *>(counts + num_loops);
  int *d_num_valid = reinterpret_cast<int *>(result + 16);

  {
    LaunchScope ls(ctx, "homo_gather");
    hipLaunchKernelGGL(homo_gather_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const float *)d_pts, npts, stride,
                       min_score, max_ambiguity, coord, valid, d_num_valid);
    rc = ls.finish();
    if (rc) return rc;
  }
  int numValid = 0;
  HIP_TRY(hipMemcpyAsync(&numValid, d_num_valid, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (numValid < 8) return MISIFT_OK;

  std::vector<int> h_sample((size_t)4 * num_loops);
  for (int i = 0; i < num_loops; i++) {                            // draw order of matching.cu:1041-1053
    int p1 = rand() % numValid;
    int p2 = rand() % numValid;
    int p3 = rand() % numValid;
    int p4 = rand() % numValid;
    while (p2 == p1) p2 = rand() % numValid;
    while (p3 == p1 || p3 == p2) p3 = rand() % numValid;
    while (p4 == p1 || p4 == p2 || p4 == p3) p4 = rand() % numValid;
    h_sample[i + 0 * (size_t)num_loops] = p1;
    h_sample[i + 1 * (size_t)num_loops] = p2;
    h_sample[i + 2 * (size_t)num_loops] = p3;
    h_sample[i + 3 * (size_t)num_loops] = p4;
  }
  HIP_TRY(hipMemcpyAsync(sample, h_sample.data(), h_sample.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  {
    LaunchScope ls(ctx, "homo_solve");
    hipLaunchKernelGGL(homo_solve_kernel, dim3((num_loops + 63) / 64), dim3(64), 0, ctx->stream, coord, stride, valid,
                       sample, num_loops, homo);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, "homo_count");
    hipLaunchKernelGGL(homo_count_kernel, dim3((num_loops + 3) / 4), dim3(256), 0, ctx->stream, coord, stride, npts,
                       homo, num_loops, thresh * thresh, counts);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, "homo_pick");
    hipLaunchKernelGGL(homo_pick_kernel, dim3(1), dim3(1024), 0, ctx->stream, counts, homo, num_loops, result);
    rc = ls.finish();
    if (rc) return rc;
  }
  float h_result[10];
  HIP_TRY(hipMemcpyAsync(h_result, result, sizeof(h_result), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));                      // also keeps h_sample alive until the upload is done
  memcpy(homography, h_result, 8 * sizeof(float));
  homography[8] = 1.0f;
  memcpy(num_matches, &h_result[8], sizeof(int));
  return MISIFT_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// ImproveHomography on the device (reference geomFuncs.cpp:6-72, a HOST function there: it walks
// SiftData.h_data).  Same arithmetic as oracle orc_improve_homography — which is pinned bit for bit against the
// reference's own geomFuncs.cpp — and the same summation ORDER: the 36 distinct entries of the symmetric 8x8 normal
// matrix and the 8 entries of the right-hand side each belong to one lane, and every lane walks the points in index
// order, so each double-precision sum is accumulated exactly as the reference's sequential loop accumulates it.  The
// problem is tiny (a few thousand points, 5 loops); what the device version buys is that the records never leave HBM.
namespace {

struct ImproveArgs {
  const SiftPointD *pts;
  int npts, num_loops;
  float min_score, max_ambiguity, limit;
  double a0[8];
};

__device__ __forceinline__ double pick8(int k, double v0, double v1, double v2, double v3, double v4, double v5, double v6,
                                        double v7)
{
  double r = v0;
  r = k == 1 ? v1 : r; r = k == 2 ? v2 : r; r = k == 3 ? v3 : r; r = k == 4 ? v4 : r;
  r = k == 5 ? v5 : r; r = k == 6 ? v6 : r; r = k == 7 ? v7 : r;
  return r;
}

__global__ __launch_bounds__(64) void improve_homography_kernel(ImproveArgs P, SiftPointD *__restrict__ pts_rw,
                                                                float *__restrict__ result)
{
#define HOMO_CORE_IMPROVE
#include "homography_core.inc"
#undef HOMO_CORE_IMPROVE
  if (lane < 8) result[lane] = (float)s_A[lane];
  if (lane == 0) {
    result[8] = 1.0f;
    reinterpret_cast<int *>(result)[9] = numfit;
  }
}

}  // namespace

extern "C" int misift_improve_homography(misift_ctx *ctx, void *d_pts, int npts, float *homography, int num_loops,
                                         float min_score, float max_ambiguity, float thresh, int *num_fit)
{
  if (!ctx || !homography || !num_fit || num_loops < 0 || npts < 0) {
    misift_set_error("misift_improve_homography: invalid argument");
    return MISIFT_EINVAL;
  }
  *num_fit = 0;
  if (!d_pts) return MISIFT_OK;                                    // geomFuncs.cpp:11-12
  int rc = misift_ensure_tmp(ctx, 64 * sizeof(float));
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  ImproveArgs P;
  P.pts = (const SiftPointD *)d_pts;
  P.npts = npts; P.num_loops = num_loops;
  P.min_score = min_score; P.max_ambiguity = max_ambiguity; P.limit = thresh * thresh;
  for (int i = 0; i < 8; i++) P.a0[i] = homography[i] / homography[8];      // float division (geomFuncs.cpp:20-21)
  float *result = reinterpret_cast<float *>(ctx->d_match_tmp);
  {
    LaunchScope ls(ctx, "improve_homography");
    hipLaunchKernelGGL(improve_homography_kernel, dim3(1), dim3(64), 0, ctx->stream, P, (SiftPointD *)d_pts, result);
    rc = ls.finish();
    if (rc) return rc;
  }
  float h[10];
  HIP_TRY(hipMemcpyAsync(h, result, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  memcpy(homography, h, 9 * sizeof(float));
  memcpy(num_fit, &h[9], sizeof(int));
  return MISIFT_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Batches: misift_find_homography_batch / misift_improve_homography_batch.  Entry e works on frame frames[e] of a
// device-resident record batch (counts and offsets read on the device) and writes result slot e; no host round trip.
// Find, four launches whatever the number of entries (L = num_loops rounded up to 16):
//   gather  one 1024-thread workgroup per entry: the gather of homo_gather_kernel into the entry's temp, then wave 0 draws
//           the entry's L x 4 sample positions from libc rand() restated on the device (libc_rand.hpp), seeded with
//           seeds[e]: the same draws as srand(seeds[e]) followed by the single call.  Entries with fewer than 8 records,
//           fewer than 8 valid points, or more than max_pts records are marked done here.
//   solve   one lane per (entry, hypothesis): the single call's solve; also zeroes the entry's counts.
//   count   the hot path: one 64-lane workgroup per (entry, 64 hypotheses, 512-point chunk).  The chunk's coordinates
//           are staged once in LDS and read by broadcast; each lane holds one hypothesis in registers and tests every
//           point of the chunk with the single call's inlier test, then adds its count atomically (an integer sum, so
//           the order of the chunks does not matter).
//   pick    one 1024-thread workgroup per entry: the single call's pick -> H (H[8] = 1) and the count; identity H and
//           0 (or -1 over max_pts) for the entries the gather marked done.
// Improve, one launch: one 64-lane workgroup per entry runs the single call's rounds on the frame's records in place.
namespace {

constexpr int HB_CHUNK = 512;                  // points per count workgroup (8 KiB of LDS)

struct HbArgs {
  BatchLayout set;
  const int *frames;                           // pinned host copies of the caller's lists
  const unsigned *seeds;
  int max_pts, mp16, num_loops;                // mp16 = max_pts rounded up to 16; num_loops rounded up to 16
  float min_score, max_ambiguity, thresh2;
  // temp, per entry e: coord[4 x mp16] | valid[mp16] | sample[4 x L] | homo[8 x L] | hcount[L] | meta[2]
  float *coord;
  int *valid, *sample;
  float *homo;
  int *hcount, *meta;                          // meta[2e] = points to count (0: entry done), meta[2e+1] = its result
  float *H;                                    // out: nsel x 9
  int *num;                                    // out: nsel
};

__global__ __launch_bounds__(1024) void homo_batch_gather_kernel(HbArgs G)
{
  const int e = blockIdx.x;
  const int f = G.frames[e];
  const int n = G.set.counts[f];
  if (n < 8 || n > G.max_pts) {                // matching.cu:1016-1017 (count -1 included); over max_pts: -1, nothing read
    if (threadIdx.x == 0) { G.meta[2 * e] = 0; G.meta[2 * e + 1] = n > G.max_pts ? -1 : 0; }
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
    if (tid == 0) { G.meta[2 * e] = 0; G.meta[2 * e + 1] = 0; }
    return;
  }
  if (tid < 64) {                              // wave 0: the entry's rand() stream, in the reference's draw order
    const int L = G.num_loops;
    int *sample = G.sample + (size_t)e * 4 * L;
    LibcRand<LibcRandWaveRing> g;
    g.seed(G.seeds[e]);
    const FastMod31 fm((uint32_t)num_valid);
    for (int loop = 0; loop < L; loop++) {
      int p[4];
      homography_draw4(g, fm, p);
      if (tid == 0)
        for (int k = 0; k < 4; k++) sample[k * L + loop] = p[k];
    }
    if (tid == 0) { G.meta[2 * e] = npts; G.meta[2 * e + 1] = 0; }
  }
}

__global__ __launch_bounds__(64) void homo_batch_solve_kernel(HbArgs G, int hblocks)
{
  const int e = blockIdx.x / hblocks;
  const int idx = (blockIdx.x % hblocks) * 64 + threadIdx.x;
  const int num_loops = G.num_loops;
  if (G.meta[2 * e] == 0 || idx >= num_loops) return;
  const float *coord = G.coord + (size_t)e * 4 * G.mp16;
  const int stride = G.mp16;
  const int *valid = G.valid + (size_t)e * G.mp16;
  const int *sample = G.sample + (size_t)e * 4 * num_loops;
  float *homo = G.homo + (size_t)e * 8 * num_loops;
  G.hcount[(size_t)e * num_loops + idx] = 0;
#define HOMO_CORE_SOLVE
#include "homography_core.inc"
#undef HOMO_CORE_SOLVE
}

__global__ __launch_bounds__(64) void homo_batch_count_kernel(HbArgs G, int hblocks, int chunks)
{
  __shared__ float4 s_pt[HB_CHUNK];
  const int c = blockIdx.x % chunks, eh = blockIdx.x / chunks;
  const int e = eh / hblocks, hb = eh % hblocks;
  const int npts = G.meta[2 * e];
  const int i0 = c * HB_CHUNK;
  if (i0 >= npts) return;                      // beyond the frame, or an entry already done (npts 0)
  const int n = min(HB_CHUNK, npts - i0);
  const int L = G.num_loops, mp = G.mp16;
  const float *coord = G.coord + (size_t)e * 4 * mp + i0;
  for (int i = threadIdx.x; i < n; i += 64)
    s_pt[i] = make_float4(coord[i], coord[mp + i], coord[2 * mp + i], coord[3 * mp + i]);
  __syncthreads();
  const int hyp = hb * 64 + threadIdx.x;
  if (hyp >= L) return;
  const float *homo = G.homo + (size_t)e * 8 * L;
  float a[8];
  for (int k = 0; k < 8; k++) a[k] = homo[k * L + hyp];
  const float thresh2 = G.thresh2;
  int cnt = 0;
  for (int i = 0; i < n; i++) {
    const float4 q = s_pt[i];
    const float x1 = q.x, y1 = q.y, x2 = q.z, y2 = q.w;
#define HOMO_CORE_INLIER
#include "homography_core.inc"
#undef HOMO_CORE_INLIER
  }
  atomicAdd(&G.hcount[(size_t)e * L + hyp], cnt);
}

__global__ __launch_bounds__(1024) void homo_batch_pick_kernel(HbArgs G)
{
  const int e = blockIdx.x;
  float *H = G.H + (size_t)9 * e;
  if (G.meta[2 * e] == 0) {                    // identity and 0, or -1 for a frame over max_pts
    if (threadIdx.x < 9) H[threadIdx.x] = threadIdx.x % 4 == 0 ? 1.0f : 0.0f;
    if (threadIdx.x == 0) G.num[e] = G.meta[2 * e + 1];
    return;
  }
  const int num_loops = G.num_loops;
  const int *counts = G.hcount + (size_t)e * num_loops;
#define HOMO_CORE_PICK
#include "homography_core.inc"
#undef HOMO_CORE_PICK
  if (tid == 0) {
    const int idx = 0x7fffffff - (int)(unsigned)(best & 0xffffffffull);
    const float *homo = G.homo + (size_t)e * 8 * num_loops;
    for (int k = 0; k < 8; k++) H[k] = homo[k * num_loops + idx];
    H[8] = 1.0f;
    G.num[e] = (int)(best >> 32);
  }
}

struct HbImproveArgs {
  BatchLayout set;
  const int *frames;                           // pinned host copy
  int num_loops;
  float min_score, max_ambiguity, limit;
  float *H;                                    // in / out: nsel x 9
  int *num_fit;
};

__global__ __launch_bounds__(64) void improve_homography_batch_kernel(HbImproveArgs B)
{
  const int e = blockIdx.x, f = B.frames[e];
  const long long base = B.set.base(f);
  float *h = B.H + (size_t)9 * e;
  ImproveArgs P;
  P.pts = B.set.recs + base;
  P.npts = max(B.set.counts[f], 0);
  P.num_loops = B.num_loops;
  P.min_score = B.min_score; P.max_ambiguity = B.max_ambiguity; P.limit = B.limit;
  for (int i = 0; i < 8; i++) P.a0[i] = h[i] / h[8];           // float division, as the single call does on the host
  SiftPointD *pts_rw = B.set.recs + base;
#define HOMO_CORE_IMPROVE
#include "homography_core.inc"
#undef HOMO_CORE_IMPROVE
  // every lane read h[] before the fragment's first barrier
  if (lane < 8) h[lane] = (float)s_A[lane];
  if (lane == 0) {
    h[8] = 1.0f;
    B.num_fit[e] = numfit;
  }
}

size_t round16(size_t v) { return (v + 15) / 16 * 16; }

}  // namespace

size_t find_homography_batch_tmp_bytes(int nsel, int max_pts, int num_loops)
{
  const size_t mp = round16((size_t)max_pts), L = round16((size_t)num_loops);
  return (size_t)nsel * (sizeof(float) * 4 * mp + sizeof(int) * mp + sizeof(int) * 4 * L + sizeof(float) * 8 * L +
                         sizeof(int) * L + sizeof(int) * 2);
}

int launch_find_homography_batch(misift_ctx *ctx, int nsel, const int *h_frames, const unsigned *h_seeds,
                                 const BatchLayout &set, int max_pts, int num_loops, float min_score,
                                 float max_ambiguity, float thresh, float *H, int *num)
{
  HbArgs G;
  G.set = set;
  G.frames = h_frames; G.seeds = h_seeds;
  G.max_pts = max_pts;
  G.mp16 = (int)round16((size_t)max_pts);
  G.num_loops = (int)round16((size_t)num_loops);
  G.min_score = min_score; G.max_ambiguity = max_ambiguity; G.thresh2 = thresh * thresh;
  const size_t mp = (size_t)G.mp16, L = (size_t)G.num_loops, ns = (size_t)nsel;
  const int hblocks = (G.num_loops + 63) / 64, chunks = (int)((mp + HB_CHUNK - 1) / HB_CHUNK);
  if ((long long)nsel * hblocks * chunks > 0x7fffffffLL) {
    misift_set_error("misift_find_homography_batch: %d entries x %d loops x %d points is beyond one launch", nsel,
                     num_loops, max_pts);
    return MISIFT_EINVAL;
  }
  int rc = misift_ensure_tmp(ctx, find_homography_batch_tmp_bytes(nsel, max_pts, num_loops));
  if (rc) return rc;
  G.coord = reinterpret_cast<float *>(ctx->d_match_tmp);
  G.valid = reinterpret_cast<int *>(G.coord + ns * 4 * mp);
  G.sample = G.valid + ns * mp;
  G.homo = reinterpret_cast<float *>(G.sample + ns * 4 * L);
  G.hcount = reinterpret_cast<int *>(G.homo + ns * 8 * L);
  G.meta = G.hcount + ns * L;
  G.H = H; G.num = num;
  {
    LaunchScope ls(ctx, "homo_batch_gather");
    hipLaunchKernelGGL(homo_batch_gather_kernel, dim3(nsel), dim3(1024), 0, ctx->stream, G);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, "homo_batch_solve");
    hipLaunchKernelGGL(homo_batch_solve_kernel, dim3(nsel * hblocks), dim3(64), 0, ctx->stream, G, hblocks);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, "homo_batch_count");
    hipLaunchKernelGGL(homo_batch_count_kernel, dim3(nsel * hblocks * chunks), dim3(64), 0, ctx->stream, G, hblocks,
                       chunks);
    rc = ls.finish();
    if (rc) return rc;
  }
  LaunchScope ls(ctx, "homo_batch_pick");
  hipLaunchKernelGGL(homo_batch_pick_kernel, dim3(nsel), dim3(1024), 0, ctx->stream, G);
  return ls.finish();
}

int launch_improve_homography_batch(misift_ctx *ctx, int nsel, const int *h_frames, const BatchLayout &set,
                                    int num_loops, float min_score, float max_ambiguity, float thresh, float *H,
                                    int *num_fit)
{
  HbImproveArgs B;
  B.set = set;
  B.frames = h_frames;
  B.num_loops = num_loops;
  B.min_score = min_score; B.max_ambiguity = max_ambiguity; B.limit = thresh * thresh;
  B.H = H; B.num_fit = num_fit;
  LaunchScope ls(ctx, "improve_homography_batch");
  hipLaunchKernelGGL(improve_homography_batch_kernel, dim3(nsel), dim3(64), 0, ctx->stream, B);
  return ls.finish();
}

// Test-only, host-only: the restated libc rand() and the sample draw the batch kernels run (libc_rand.hpp).
extern "C" int misift_test_libc_rand(unsigned seed, int n, int *out)
{
  if (n < 0 || (n > 0 && !out)) {
    misift_set_error("misift_test_libc_rand: invalid argument");
    return MISIFT_EINVAL;
  }
  LibcRand<LibcRandArrayRing> g;
  g.seed(seed);
  for (int i = 0; i < n; i++) out[i] = g.next();
  return MISIFT_OK;
}

extern "C" int misift_test_homography_samples(unsigned seed, int num_valid, int num_loops, int *out)
{
  if (num_valid < 8 || num_loops < 0 || (num_loops > 0 && !out)) {
    misift_set_error("misift_test_homography_samples: invalid argument");
    return MISIFT_EINVAL;
  }
  LibcRand<LibcRandArrayRing> g;
  g.seed(seed);
  const FastMod31 fm((uint32_t)num_valid);
  for (int loop = 0; loop < num_loops; loop++) {
    int p[4];
    homography_draw4(g, fm, p);
    for (int k = 0; k < 4; k++) out[4 * loop + k] = p[k];
  }
  return MISIFT_OK;
}

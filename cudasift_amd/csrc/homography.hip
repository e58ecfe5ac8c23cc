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
// What the single call shares with the batch search (ransac_batch.hpp, second half of this file) is written once: the
// gather (ransac_gather) and the pick (ransac_pick) are that header's functions, the inlier test is homography_inlier
// below, and the solve is the HOMO_CORE_SOLVE fragment of homography_core.inc.
//
// Deviation: the reference counts inliers over numPts rounded up to 16
// and so reads up to 15 uninitialised coordinates; here exactly numPts points are tested.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "common.hpp"
#include "libc_rand.hpp"
#include "ransac_batch.hpp"

namespace {

__device__ __forceinline__ float mul_rz(float a, float b)
{
  // exact round-toward-zero product: RN product, then step one ulp toward zero when the exact
  // residual says RN rounded away from zero
  float p = a * b;
  const float e = fmaf(a, b, -p);
  const bool away = (p > 0.0f && e < 0.0f) || (p < 0.0f && e > 0.0f);
  return away ? __uint_as_float(__float_as_uint(p) - 1u) : p;
}

// The inlier test of TestHomographies (matching.cu:975-990) with its round-toward-zero products: hypothesis a on the
// stored match (x1, y1) -> (x2, y2).
__device__ __forceinline__ bool homography_inlier(const float (&a)[8], float x1, float y1, float x2, float y2,
                                                  float thresh2)
{
  const float nomx = mul_rz(a[0], x1) + mul_rz(a[1], y1) + a[2];
  const float nomy = mul_rz(a[3], x1) + mul_rz(a[4], y1) + a[5];
  const float deno = mul_rz(a[6], x1) + mul_rz(a[7], y1) + 1.0f;
  const float errx = mul_rz(x2, deno) - nomx;
  const float erry = mul_rz(y2, deno) - nomy;
  const float err2 = mul_rz(errx, errx) + mul_rz(erry, erry);
  return err2 < mul_rz(thresh2, mul_rz(deno, deno));
}

// ---- gather: SoA coordinates + ordered compaction of the valid points -------------------------
__global__ __launch_bounds__(1024) void homo_gather_kernel(const float *__restrict__ pts, int npts, int stride,
                                                             float min_score, float max_ambiguity,
                                                             float *__restrict__ coord, int *__restrict__ valid,
                                                             int *__restrict__ num_valid)
{
  const int nv = ransac_gather(pts, npts, stride, min_score, max_ambiguity, coord, valid);
  if (threadIdx.x == 0) *num_valid = nv;
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
    cnt += homography_inlier(a, x1, y1, x2, y2, thresh2) ? 1 : 0;
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if (lane == 0) counts[hyp] = cnt;
}

// ---- pick: first hypothesis with the largest count (strict '>' scan of matching.cu:1063-1068) ----
__global__ __launch_bounds__(1024) void homo_pick_kernel(const int *__restrict__ counts, const float *__restrict__ homo,
                                                           int num_loops, float *__restrict__ result)
{
  const unsigned long long best = ransac_pick(counts, num_loops);
  if (threadIdx.x == 0) {
    const int idx = ransac_pick_index(best);
    for (int k = 0; k < 8; k++) result[k] = homo[k * num_loops + idx];
    reinterpret_cast<int *>(result)[8] = ransac_pick_count(best);
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
// Find is the shared batch search of ransac_batch.hpp (gather + draw, solve, count, pick) with the model below: it works
// over num_loops rounded up to 16, as the single call does, draws in the reference's order (the same draws as
// srand(seeds[e]) followed by the single call), counts with the single call's inlier test over all records of the frame,
// and gives the identity to the entries the gather marked done.  The solve is this file's: one lane per (entry,
// hypothesis) runs the single call's solve.
// Improve, one launch: one 64-lane workgroup per entry runs the single call's rounds on the frame's records in place.
namespace {

struct HomographyModel : RansacPlainLane {
  typedef RansacArgs Args;
  static constexpr int SAMPLE = 4, PARAMS = 8, COORDS = 4;
  static constexpr bool INDEX = true;          // the valid records, which the sample positions go through
  static constexpr bool COUNT_ALL = true;      // TestHomographies tests every record, valid or not
  template <class Ring>
  static __device__ __forceinline__ void draw(LibcRand<Ring> &g, const FastMod31 &fm, int (&p)[4])
  {
    homography_draw4(g, fm, p);
  }
  static __device__ __forceinline__ bool inlier(const float (&a)[8], Lane, const float (&q)[4], float thresh2)
  {
    return homography_inlier(a, q[0], q[1], q[2], q[3], thresh2);
  }
  static __device__ __forceinline__ float done(int k) { return k % 4 == 0 ? 1.0f : 0.0f; }      // the identity
  static __device__ __forceinline__ void picked(float *H) { H[8] = 1.0f; }
};

// Written out, not between ransac_solve_begin and ransac_store_hyp: the fragment brings its own position loads and
// stores, and this is the kernel whose scratch-resident LU is sensitive to what surrounds it.
__global__ __launch_bounds__(64) void homo_batch_solve_kernel(RansacArgs G, int hblocks)
{
  const RansacSearch &S = G.rs;
  const int e = blockIdx.x / hblocks;
  const int idx = (blockIdx.x % hblocks) * 64 + threadIdx.x;
  if (S.meta[RANSAC_META * e] == 0 || idx >= S.num_loops) return;
  const int num_loops = S.lp;                  // the fragment's stride of sample and homo
  const float *coord = S.coord + (size_t)e * 4 * S.cap16;
  const int stride = S.cap16;
  const int *valid = S.index + (size_t)e * S.cap16;
  const int *sample = S.sample + (size_t)e * 4 * num_loops;
  float *homo = S.hyp + (size_t)e * 8 * num_loops;
  S.hcount[(size_t)e * num_loops + idx] = 0;
#define HOMO_CORE_SOLVE
#include "homography_core.inc"
#undef HOMO_CORE_SOLVE
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

}  // namespace

int launch_find_homography_batch(misift_ctx *ctx, int nsel, const int *h_frames, const unsigned *h_seeds,
                                 const BatchLayout &set, int max_pts, int num_loops, float min_score,
                                 float max_ambiguity, float thresh, float *H, int *num)
{
  const RansacNames names{"misift_find_homography_batch", "points", "homo_batch_gather", "homo_batch_solve",
                          "homo_batch_count", "homo_batch_pick"};
  return ransac_batch_run<HomographyModel>(ctx, names, nsel, h_frames, h_seeds, set, max_pts, ransac_round16(num_loops),
                                           min_score, max_ambiguity, thresh, H, num, homo_batch_solve_kernel);
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
  ransac_host_samples(seed, num_valid, num_loops, out, homography_draw4<LibcRandArrayRing>);
  return MISIFT_OK;
}

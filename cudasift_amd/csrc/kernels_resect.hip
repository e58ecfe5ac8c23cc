// kernels_resect.hip — misift_resect_cameras_batch: the camera of each selected image estimated directly from the
// observations its image makes of the triangulated track points, by batch RANSAC over calibrated six-point solves.  It
// places the images that the walk of misift_link_poses_batch never reached, and gives a placed image a second opinion that
// does not rest on the chain of pair poses.  No reference counterpart.  The arithmetic is resect_core.hpp (the draw, the
// solve) and refine_core.hpp (the inlier test), shared with the host-only test hooks at the end of this file.
//
// Two memsets (the owners, the summary) and six launches, whatever the data (nsel == 0: the summary's memset and the
// pick launch alone, which writes T):
//   cand_owner_kernel     the owner of every slot and
//   cand_key_kernel       the image every slot is a candidate of: launch_track_candidates (track_candidates.hpp).
//   resect_gather_kernel  one 1024-thread workgroup per entry walks the keys in ascending slot order; a ballot / popcount
//                         compaction keeps that order (a sample position p means "the p-th candidate"), and the lane of
//                         a candidate writes its x, y, X, Y, Z as SoA into the entry's temp.  Then wave 0 draws the
//                         entry's sample positions from libc rand() restated on the device (libc_rand.hpp), seeded with
//                         seeds[e], one hypothesis after another.  Entries that are skipped, hold more than max_cand
//                         candidates or fewer than max(6, min_inliers) are marked done here.
//   resect_solve_kernel   one lane per (entry, hypothesis), 64-lane workgroups: sample positions -> (R, t).  Each lane's
//                         11 x 12 system lives in LDS, word (r, c) of lane l at (12 r + c) * 64 + l, so every access of
//                         the wavefront hits 64 consecutive words whatever rows and columns the lanes have pivoted to:
//                         33 KiB per workgroup.  It also zeroes the entry's counts.
//   resect_count_kernel   the hot path: one 64-lane workgroup per (entry, 64 hypotheses, 512-candidate chunk).  The
//                         chunk's x, y, X, Y, Z are staged once in LDS (10 KiB) and read by broadcast; each lane holds
//                         one hypothesis and the image's intrinsics in registers, tests every candidate of the chunk
//                         with refine_member, then adds its count atomically (an integer sum: the order of the chunks
//                         does not matter).
//   resect_pick_kernel    one 1024-thread workgroup per entry: the largest count at the smallest hypothesis index
//                         (ransac_pick) -> the entry's results, the install, the summary.
// Not built: a minimal P3P solver, a local optimisation inside the search, a 32-hypothesis solve workgroup.
#include <stdint.h>
#include <string.h>
#include "common.hpp"
#include "ransac_batch.hpp"
#include "resect_core.hpp"
#include "track_candidates.hpp"

namespace {

constexpr int RESECT_META = 4;                 // ints of meta per entry

struct ResectArgs {
  TrackScene s;                                // intrinsics: the pinned host copy; cam and cam_pair may be NULL
  const int *owner, *key;                      // temp: max_obs each
  int nsel, max_cand, mc16;                    // mc16 = min(max_cand, max_obs) rounded up to 16
  int num_loops, lp;                           // hypotheses; their stride, num_loops rounded up to 16
  int min_inliers, only_unset, install;
  float thresh2;
  const int *images;                           // the pinned host copies: nsel,
  const unsigned *seeds;                       // nsel
  // temp behind owner and key, per entry e:  coord[5 x mc16] | sample[6 x lp] | hyp[12 x lp] | hcount[lp] | meta[4]
  float *coord;                                // x, y, X, Y, Z of the candidates in slot order, SoA
  int *sample;
  float *hyp;
  int *hcount;
  int *meta;                                   // [0] candidates to count (0: entry done), [1] a done entry's status,
                                               // [2] what d_res_cand gets
  float *cam;                                  // in/out: nimages x 12, written under install
  int *cam_pair;                               // in/out: nimages
  float *res_cam;
  int *res_cand, *res_inliers, *res_status, *summary;
};

__global__ __launch_bounds__(1024) void resect_gather_kernel(ResectArgs A)
{
  __shared__ int wave_cnt[16];
  __shared__ int base_s;
  const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = A.images[e];                 // checked on the host: in [0, nimages)
  int *meta = A.meta + (size_t)RESECT_META * e;
  if (A.only_unset && A.cam_pair[img] != POSEGRAPH_UNSET) {
    if (tid == 0) { meta[0] = 0; meta[1] = RESECT_SKIPPED; meta[2] = 0; }
    return;
  }
  const int O = scene_O(A.s), T = scene_T(A.s);
  float *coord = A.coord + (size_t)e * 5 * A.mc16;
  const int mc = A.mc16;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (long long o0 = 0; o0 < O; o0 += 1024) {
    const long long o = o0 + tid;
    const bool ok = o < O && A.key[o] == img;
    const unsigned long long m = __ballot(ok);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = base_s;
    for (int w = 0; w < wave; w++) off += wave_cnt[w];
    const int pos = off + __popcll(m & ((1ull << lane) - 1ull));
    if (ok && pos < A.max_cand) {              // beyond max_cand only the count goes on
      const int t = A.owner[o];
      const bool t_ok = (unsigned)t < (unsigned)T;           // an index from device memory: checked before use
      const float *P = A.s.points + 4 * (size_t)(t_ok ? t : 0);
      const TrackObs ob = track_obs_load(A.s.obs + o);
      coord[pos] = ob.xpos;
      coord[mc + pos] = ob.ypos;
      coord[2 * mc + pos] = t_ok ? P[0] : 0.0f;
      coord[3 * mc + pos] = t_ok ? P[1] : 0.0f;
      coord[4 * mc + pos] = t_ok ? P[2] : 0.0f;
    }
    __syncthreads();
    if (tid == 0) {
      int s = 0;
      for (int w = 0; w < 16; w++) s += wave_cnt[w];
      base_s += s;
    }
    __syncthreads();
  }
  const int n = base_s;
  const int need = A.min_inliers > RESECT_SAMPLE ? A.min_inliers : RESECT_SAMPLE;
  if (n > A.max_cand || n < need) {
    if (tid == 0) { meta[0] = 0; meta[1] = n > A.max_cand ? RESECT_OVER : RESECT_FEW_CAND; meta[2] = n; }
    return;
  }
  if (tid < 64) {                              // wave 0: the entry's rand() stream, hypotheses one after another
    const int L = A.num_loops, lp = A.lp;
    int *sample = A.sample + (size_t)e * RESECT_SAMPLE * lp;
    LibcRand<LibcRandWaveRing> g;
    g.seed(A.seeds[e]);
    const FastMod31 fm((uint32_t)n);
    for (int loop = 0; loop < L; loop++) {
      int p[RESECT_SAMPLE];
      resect_draw6(g, fm, p);
      if (tid == 0)
        for (int k = 0; k < RESECT_SAMPLE; k++) sample[k * lp + loop] = p[k];
    }
    if (tid == 0) { meta[0] = n; meta[1] = 0; meta[2] = n; }
  }
}

// a lane's 11 x 12 system in LDS: word (r, c) at (12 r + c) * 64 from the lane's base
struct ResectLdsMat {
  float *base;
  __device__ float get(int r, int c) const { return base[(RESECT_COLS * r + c) * 64]; }
  __device__ void set(int r, int c, float v) { base[(RESECT_COLS * r + c) * 64] = v; }
};

__global__ __launch_bounds__(64) void resect_solve_kernel(ResectArgs A, int hblocks)
{
  __shared__ float s_m[RESECT_ROWS * RESECT_COLS * 64];
  const int e = blockIdx.x / hblocks;
  const int idx = (blockIdx.x % hblocks) * 64 + threadIdx.x;
  const int *meta = A.meta + (size_t)RESECT_META * e;
  const int n = min(meta[0], A.max_cand);
  if (n <= 0 || idx >= A.num_loops) return;
  const int lp = A.lp, mc = A.mc16;
  const float *coord = A.coord + (size_t)e * 5 * mc;
  const int *sample = A.sample + (size_t)e * RESECT_SAMPLE * lp;
  A.hcount[(size_t)e * lp + idx] = 0;
  float x[6], y[6], X[6], Y[6], Z[6];
  bool in_range = true;                        // positions come from device memory: checked before use
#pragma unroll
  for (int k = 0; k < RESECT_SAMPLE; k++) {
    const int pos = sample[k * lp + idx];
    const bool pos_ok = (unsigned)pos < (unsigned)n;
    const int i = pos_ok ? pos : 0;
    in_range = in_range && pos_ok;
    x[k] = coord[i]; y[k] = coord[mc + i]; X[k] = coord[2 * mc + i]; Y[k] = coord[3 * mc + i]; Z[k] = coord[4 * mc + i];
  }
  const float *kp = A.s.intrinsics + 4 * (size_t)A.images[e];
  const float k[4] = {kp[0], kp[1], kp[2], kp[3]};
  ResectLdsMat m{s_m + threadIdx.x};
  float cam[12];
  resect_solve6(m, x, y, X, Y, Z, k, cam);
  float *hyp = A.hyp + (size_t)e * 12 * lp;
#pragma unroll
  for (int j = 0; j < 12; j++) hyp[j * lp + idx] = in_range ? cam[j] : 0.0f;
}

__global__ __launch_bounds__(64) void resect_count_kernel(ResectArgs A, int hblocks, int chunks)
{
  __shared__ float4 s_a[RANSAC_CHUNK];         // x, y, X, Y
  __shared__ float s_z[RANSAC_CHUNK];
  const int c = blockIdx.x % chunks, eh = blockIdx.x / chunks;
  const int e = eh / hblocks, hb = eh % hblocks;
  const int *meta = A.meta + (size_t)RESECT_META * e;
  const int total = min(meta[0], A.max_cand);
  const int i0 = c * RANSAC_CHUNK;
  if (i0 >= total) return;                     // beyond the candidates, or an entry already done (0)
  const int n = min(RANSAC_CHUNK, total - i0);
  const int lp = A.lp, mc = A.mc16;
  const float *coord = A.coord + (size_t)e * 5 * mc + i0;
  for (int i = threadIdx.x; i < n; i += 64) {
    s_a[i] = make_float4(coord[i], coord[mc + i], coord[2 * mc + i], coord[3 * mc + i]);
    s_z[i] = coord[4 * mc + i];
  }
  __syncthreads();
  const int h = hb * 64 + threadIdx.x;
  if (h >= A.num_loops) return;
  const float *hyp = A.hyp + (size_t)e * 12 * lp;
  float cam[12];
#pragma unroll
  for (int j = 0; j < 12; j++) cam[j] = hyp[j * lp + h];
  const float *kp = A.s.intrinsics + 4 * (size_t)A.images[e];
  const float k[4] = {kp[0], kp[1], kp[2], kp[3]};
  const float thresh2 = A.thresh2;
  int cnt = 0;
  for (int i = 0; i < n; i++) {
    const float4 q = s_a[i];
    const float X[3] = {q.z, q.w, s_z[i]};
    cnt += refine_member(cam, k, X, q.x, q.y, thresh2) ? 1 : 0;
  }
  atomicAdd(&A.hcount[(size_t)e * lp + h], cnt);
}

__global__ __launch_bounds__(1024) void resect_pick_kernel(ResectArgs A)
{
  const int e = blockIdx.x, tid = threadIdx.x;
  if (e == 0 && tid == 0) A.summary[0] = scene_T(A.s);
  if (e >= A.nsel) return;                     // nsel == 0: the one workgroup that writes T
  const int *meta = A.meta + (size_t)RESECT_META * e;
  const bool searched = meta[0] != 0;
  unsigned long long best = 0;
  if (searched) best = ransac_pick(A.hcount + (size_t)e * A.lp, A.num_loops);
  if (tid != 0) return;
  int status = meta[1], inliers = 0;
  float cam[12];
#pragma unroll
  for (int j = 0; j < 12; j++) cam[j] = 0.0f;
  if (searched) {
    inliers = ransac_pick_count(best);
    status = inliers < A.min_inliers ? RESECT_NO_MODEL : RESECT_OK;
    if (status == RESECT_OK) {
      const int idx = min(max(ransac_pick_index(best), 0), A.num_loops - 1);
      const float *hyp = A.hyp + (size_t)e * 12 * A.lp;
#pragma unroll
      for (int j = 0; j < 12; j++) cam[j] = pose_one_nan(hyp[j * A.lp + idx]);
    }
  }
  float *out = A.res_cam + 12 * (size_t)e;
#pragma unroll
  for (int j = 0; j < 12; j++) out[j] = cam[j];
  A.res_cand[e] = meta[2];
  A.res_inliers[e] = inliers;
  A.res_status[e] = status;
  if (A.install && status == RESECT_OK) {
    const int img = A.images[e];
    float *dst = A.cam + 12 * (size_t)img;
#pragma unroll
    for (int j = 0; j < 12; j++) dst[j] = cam[j];
    A.cam_pair[img] = POSEGRAPH_RESECTED;
  }
  atomicAdd(&A.summary[status == RESECT_OK ? 1 : status + 2], 1);
  if (status == RESECT_OK) atomicAdd(&A.summary[2], inliers);
}

// the candidates an entry's temp has room for: an image has no more than O <= max_obs, so n > max_cand decides as stated
int resect_capacity(int max_obs, int max_cand) { return min(max_cand, min(max_obs, 0x7fffffff - 15)); }

// the words of temp behind owner and key that one entry takes
size_t resect_entry_words(int max_obs, int max_cand, int num_loops)
{
  return 5 * (size_t)ransac_round16(resect_capacity(max_obs, max_cand)) +
         (RESECT_SAMPLE + 12 + 1) * (size_t)ransac_round16(num_loops) + RESECT_META;
}

}  // namespace

// whether the count's grid, nsel x hypothesis blocks x chunks, fits one launch (and num_loops its stride)
bool resect_cameras_batch_one_launch(int max_obs, int nsel, int max_cand, int num_loops)
{
  const long long hb = ((long long)num_loops + 63) / 64;
  const long long ch = ((long long)resect_capacity(max_obs, max_cand) + RANSAC_CHUNK - 1) / RANSAC_CHUNK;
  return num_loops <= 0x7fffffff - 15 && nsel * hb <= 0x7fffffffLL && nsel * hb * ch <= 0x7fffffffLL;
}

size_t resect_cameras_batch_tmp_bytes(int max_obs, int nsel, int max_cand, int num_loops)
{
  return sizeof(int) * (2 * (size_t)max_obs + (size_t)nsel * resect_entry_words(max_obs, max_cand, num_loops));
}

// Enqueue misift_resect_cameras_batch on the context stream (common.hpp): two memsets and six launches.
int launch_resect_cameras_batch(misift_ctx *ctx, const TrackScene &scene, int nsel, const int *h_images,
                                const unsigned *h_seeds, int max_cand, int num_loops, float thresh2, int min_inliers,
                                int only_unset, int install, float *d_cam, int *d_cam_pair, float *d_res_cam,
                                int *d_res_cand, int *d_res_inliers, int *d_res_status, int *d_summary)
{
  const int max_obs = scene.max_obs;
  const int cap = resect_capacity(max_obs, max_cand);
  if (!resect_cameras_batch_one_launch(max_obs, nsel, max_cand, num_loops)) {                // the wrapper's check
    misift_set_error("misift_resect_cameras_batch: %d entries x %d loops x %d candidates is beyond one launch", nsel,
                     num_loops, cap);
    return MISIFT_EINVAL;
  }
  ResectArgs A{};
  A.s = scene;
  A.nsel = nsel; A.max_cand = max_cand; A.mc16 = ransac_round16(cap);
  A.num_loops = num_loops; A.lp = ransac_round16(num_loops);
  A.min_inliers = min_inliers; A.only_unset = only_unset; A.install = install; A.thresh2 = thresh2;
  const int hblocks = (num_loops + 63) / 64, chunks = (A.mc16 + RANSAC_CHUNK - 1) / RANSAC_CHUNK;
  const int rc = misift_ensure_tmp(ctx, resect_cameras_batch_tmp_bytes(max_obs, nsel, max_cand, num_loops));
  if (rc) return rc;
  A.images = h_images; A.seeds = h_seeds;
  const size_t ns = (size_t)nsel, mc = (size_t)A.mc16, lp = (size_t)A.lp;
  int *owner = reinterpret_cast<int *>(ctx->d_match_tmp), *key = owner + max_obs;
  A.owner = owner; A.key = key;
  A.coord = reinterpret_cast<float *>(key + max_obs);
  A.sample = reinterpret_cast<int *>(A.coord + ns * 5 * mc);
  A.hyp = reinterpret_cast<float *>(A.sample + ns * RESECT_SAMPLE * lp);
  A.hcount = reinterpret_cast<int *>(A.hyp + ns * 12 * lp);
  A.meta = A.hcount + ns * lp;
  A.cam = d_cam; A.cam_pair = d_cam_pair;
  A.res_cam = d_res_cam; A.res_cand = d_res_cand; A.res_inliers = d_res_inliers; A.res_status = d_res_status;
  A.summary = d_summary;
  HIP_TRY(hipMemsetAsync(d_summary, 0, 8 * sizeof(int), ctx->stream));
  if (nsel == 0) {
    LaunchScope ls(ctx, "resect_pick");
    hipLaunchKernelGGL(resect_pick_kernel, dim3(1), dim3(1024), 0, ctx->stream, A);
    return ls.finish();
  }
  HIP_TRY(hipMemsetAsync(owner, 0xff, sizeof(int) * (size_t)max_obs, ctx->stream));
  int r;
  {
    LaunchScope ls(ctx, "resect_gather");
    launch_track_candidates(ctx, scene, owner, key);
    hipLaunchKernelGGL(resect_gather_kernel, dim3(nsel), dim3(1024), 0, ctx->stream, A);
    r = ls.finish();
    if (r) return r;
  }
  {
    LaunchScope ls(ctx, "resect_solve");
    hipLaunchKernelGGL(resect_solve_kernel, dim3(nsel * hblocks), dim3(64), 0, ctx->stream, A, hblocks);
    r = ls.finish();
    if (r) return r;
  }
  {
    LaunchScope ls(ctx, "resect_count");
    hipLaunchKernelGGL(resect_count_kernel, dim3(nsel * hblocks * chunks), dim3(64), 0, ctx->stream, A, hblocks, chunks);
    r = ls.finish();
    if (r) return r;
  }
  LaunchScope ls(ctx, "resect_pick");
  hipLaunchKernelGGL(resect_pick_kernel, dim3(nsel), dim3(1024), 0, ctx->stream, A);
  return ls.finish();
}

// Test-only, host-only: the sample draw and the six-point solve as the kernels compute them (resect_core.hpp).
extern "C" int misift_test_resect_samples(unsigned seed, int n, int num_loops, int *out)
{
  if (n < RESECT_SAMPLE || num_loops < 0 || (num_loops > 0 && !out)) {
    misift_set_error("misift_test_resect_samples: invalid argument");
    return MISIFT_EINVAL;
  }
  LibcRand<LibcRandArrayRing> g;
  g.seed(seed);
  const FastMod31 fm((uint32_t)n);
  for (int loop = 0; loop < num_loops; loop++) {
    int p[RESECT_SAMPLE];
    resect_draw6(g, fm, p);
    for (int k = 0; k < RESECT_SAMPLE; k++) out[RESECT_SAMPLE * loop + k] = p[k];
  }
  return MISIFT_OK;
}

extern "C" int misift_test_resect_solve(const float *xyXYZ, const float *intrinsics4, float *cam12, int *valid)
{
  if (!xyXYZ || !intrinsics4 || !cam12 || !valid) {
    misift_set_error("misift_test_resect_solve: invalid argument");
    return MISIFT_EINVAL;
  }
  float x[6], y[6], X[6], Y[6], Z[6], cam[12];
  for (int k = 0; k < 6; k++) {
    x[k] = xyXYZ[5 * k]; y[k] = xyXYZ[5 * k + 1];
    X[k] = xyXYZ[5 * k + 2]; Y[k] = xyXYZ[5 * k + 3]; Z[k] = xyXYZ[5 * k + 4];
  }
  ResectArrayMat m;
  *valid = resect_solve6(m, x, y, X, Y, Z, intrinsics4, cam) ? 1 : 0;
  for (int k = 0; k < 12; k++) cam12[k] = cam[k];
  return MISIFT_OK;
}

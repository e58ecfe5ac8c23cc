// kernels_align.hip — two reconstructions related by a similarity transform, on the device:
//   misift_correspond_tracks_batch  which track of scene B holds the records of each track of scene A,
//   misift_align_points_batch       per entry a RANSAC search over three-point closed-form solves (Horn), refitted over
//                                   its inliers,
//   misift_transform_scene_batch    the transform applied to the points and the cameras of a scene.
// No reference counterpart.  The arithmetic is align_core.hpp, shared with the host-only test hooks at the end of this
// file.
//
// misift_align_points_batch: the search is ransac_batch.hpp's with AlignModel below.  What is this file's: one memset
// (the summary) and, whatever the data, five launches (nsel == 0: the memset alone):
//   align_gather_kernel  walks the entry's source points in ascending index; the lane of a candidate writes its six
//                        coordinates and its index.  d_inlier gets 0 / -1 here.
//   align_solve_kernel   all in registers: positions -> 13 floats.
//   (count)              ransac_count_kernel<AlignModel>: align_error2 under the threshold, 12 KiB of LDS.
//   align_pick_kernel    the picked hypothesis into cur, the tail of the entry's temp, and its count into meta[3].
//   align_refit_kernel   behind the search, one 256-thread workgroup per entry: the refits (align_refit; the 256-slot
//                        sums in 11 KiB of LDS), the rms, and every output of the entry.
// Not built: a reprojection-error inlier test, a local optimisation inside the search.
#include <stdint.h>
#include <string.h>
#include "common.hpp"
#include "ransac_batch.hpp"
#include "align_core.hpp"

namespace {

constexpr int ALIGN_COORDS = 6;
constexpr int ALIGN_TAIL = 16;                 // words of temp per entry behind the search's: cur

struct AlignArgs {
  RansacSearch rs;                             // coord: ax ay az bx by bz of the candidates in index order; index: the
                                               // source index i of each; meta[1] a done entry's status, [2] candidates,
                                               // [3] the picked count
  const float *src, *dst;                      // pooled, four floats per point
  const int *src_status, *dst_status;          // pooled, or NULL
  const int *map;                              // pooled with src
  const int *ranges;                           // the pinned host copy: nsel x 4
  const int *count;                            // device, or NULL
  long long count_stride;
  int min_inliers, refit_loops;
  float *cur;                                  // temp: the picked hypothesis
  float *sim;
  int *cand, *inliers, *status, *inlier, *summary;
};

struct AlignModel : RansacPlainLane {
  typedef AlignArgs Args;
  static constexpr int SAMPLE = ALIGN_SAMPLE, PARAMS = ALIGN_PARAMS, COORDS = ALIGN_COORDS;
  static constexpr bool INDEX = true, COUNT_ALL = true;
  template <class Ring>
  static __device__ __forceinline__ void draw(LibcRand<Ring> &g, const FastMod31 &fm, int (&p)[ALIGN_SAMPLE])
  {
    align_draw3(g, fm, p);
  }
  static __device__ __forceinline__ bool inlier(const float (&g)[ALIGN_PARAMS], Lane, const float (&q)[6], float thresh2)
  {
    return align_error2(g, q[0], q[1], q[2], q[3], q[4], q[5]) < thresh2;
  }
  static __device__ __forceinline__ float invalid() { return pose_one_nan(NAN); }      // align_invalid
};

__global__ __launch_bounds__(1024) void align_gather_kernel(AlignArgs A)
{
  const RansacSearch &S = A.rs;
  const int e = blockIdx.x, tid = threadIdx.x;
  const int src_first = A.ranges[4 * e], src_cap = A.ranges[4 * e + 1];
  const int dst_first = A.ranges[4 * e + 2], dst_cap = A.ranges[4 * e + 3];
  int ne = src_cap;
  if (A.count) ne = scene_clamp(A.count[(long long)e * A.count_stride], src_cap);
  int *meta = S.meta + (size_t)RANSAC_META * e;
  const int mc = S.cap16;
  float *coord = S.coord + (size_t)e * ALIGN_COORDS * mc;
  int *index = S.index + (size_t)e * mc;
  const RansacCompaction c = ransac_compaction();
  for (int i0 = 0; i0 < src_cap; i0 += 1024) {
    const int i = i0 + tid;
    bool ok = false;
    float a[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f};
    if (i < ne) {
      const size_t si = (size_t)src_first + (size_t)i;
      const int m = A.map[si];
      if ((unsigned)m < (unsigned)dst_cap) {   // an index from device memory: checked before use
        const size_t di = (size_t)dst_first + (size_t)m;
        ok = (!A.src_status || A.src_status[si] == 0) && (!A.dst_status || A.dst_status[di] == 0);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          a[k] = A.src[4 * si + k];
          b[k] = A.dst[4 * di + k];
          ok = ok && fundamental_finite(a[k]) && fundamental_finite(b[k]);
        }
      }
    }
    const int pos = c.place(ok);
    if (ok) {                                  // pos <= i < src_cap <= mc
#pragma unroll
      for (int k = 0; k < 3; k++) {
        coord[k * mc + pos] = a[k];
        coord[(3 + k) * mc + pos] = b[k];
      }
      index[pos] = i;
    }
    if (A.inlier && i < src_cap) A.inlier[(size_t)src_first + (size_t)i] = ok ? 0 : -1;
    c.next();
  }
  const int n = c.total();
  const int need = A.min_inliers > ALIGN_SAMPLE ? A.min_inliers : ALIGN_SAMPLE;
  if (n < need) {
    if (tid == 0) { meta[0] = 0; meta[1] = ALIGN_FEW_CAND; meta[2] = n; meta[3] = 0; }
    return;
  }
  if (tid < 64) {                              // wave 0
    ransac_draw<AlignModel>(S.seeds[e], n, S.sample + (size_t)e * ALIGN_SAMPLE * S.lp, S.num_loops, S.lp);
    if (tid == 0) { meta[0] = n; meta[1] = 0; meta[2] = n; meta[3] = 0; }
  }
}

__global__ __launch_bounds__(64) void align_solve_kernel(AlignArgs A, int hblocks)
{
  const RansacSearch &S = A.rs;
  int e, idx, n;
  if (!ransac_solve_begin(S, hblocks, e, idx, n)) return;
  const int mc = S.cap16;
  const float *coord = S.coord + (size_t)e * ALIGN_COORDS * mc;
  float a[3][3], b[3][3];
  bool in_range = true;
#pragma unroll
  for (int k = 0; k < ALIGN_SAMPLE; k++) {
    const int i = ransac_sample_position<AlignModel>(S, e, idx, k, n, in_range);
#pragma unroll
    for (int j = 0; j < 3; j++) {
      a[k][j] = coord[j * mc + i];
      b[k][j] = coord[(3 + j) * mc + i];
    }
  }
  float h[ALIGN_PARAMS];
  align_solve3(a, b, h);
  ransac_store_hyp<AlignModel>(S, e, idx, in_range, h);
}

__global__ __launch_bounds__(1024) void align_pick_kernel(AlignArgs A)
{
  const RansacSearch &S = A.rs;
  const int e = blockIdx.x, tid = threadIdx.x;
  int *meta = S.meta + (size_t)RANSAC_META * e;
  if (meta[0] == 0) return;
  const unsigned long long best = ransac_pick(S.hcount + (size_t)e * S.lp, S.num_loops);
  if (tid != 0) return;
  const int idx = min(max(ransac_pick_index(best), 0), S.num_loops - 1);
  const float *hyp = S.hyp + (size_t)e * ALIGN_PARAMS * S.lp;
  float *cur = A.cur + ALIGN_TAIL * (size_t)e;
#pragma unroll
  for (int j = 0; j < ALIGN_PARAMS; j++) cur[j] = hyp[j * S.lp + idx];
  meta[3] = ransac_pick_count(best);
}

// the entry's candidates in its temp
struct AlignTempCand {
  const float *coord;
  int mc;
  __device__ void load(int p, float (&a)[3], float (&b)[3]) const
  {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      a[k] = coord[k * mc + p];
      b[k] = coord[(3 + k) * mc + p];
    }
  }
};

// the 256-thread workgroup's Exec: the slot is the thread
struct AlignBlockExec {
  float *p;                                    // LDS: ALIGN_MOMENT_SUMS x FUND_SLOTS
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
    c = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
    __syncthreads();                           // cnt is free again
    return c;
  }
};

__global__ __launch_bounds__(FUND_SLOTS) void align_refit_kernel(AlignArgs A)
{
  __shared__ float s_p[ALIGN_MOMENT_SUMS * FUND_SLOTS];
  __shared__ int s_cnt[4];
  const RansacSearch &S = A.rs;
  const int e = blockIdx.x, tid = threadIdx.x;
  const int *meta = S.meta + (size_t)RANSAC_META * e;
  const int n = min(meta[0], S.cap16);         // 0: the gather marked the entry done
  int status = meta[1], inliers = 0, kept = 0;
  float h[ALIGN_PARAMS], rms = 0.0f;
#pragma unroll
  for (int j = 0; j < ALIGN_PARAMS; j++) h[j] = 0.0f;
  if (n > 0) {                                 // uniform over the workgroup
    inliers = meta[3];
    status = inliers < A.min_inliers ? ALIGN_NO_MODEL : ALIGN_OK;
  }
  const AlignTempCand cand{S.coord + (size_t)e * ALIGN_COORDS * S.cap16, S.cap16};
  if (n > 0 && status == ALIGN_OK) {
    const float *cur = A.cur + ALIGN_TAIL * (size_t)e;
#pragma unroll
    for (int j = 0; j < ALIGN_PARAMS; j++) h[j] = cur[j];
    AlignBlockExec ex{s_p, s_cnt};
    align_refit(ex, cand, n, S.thresh2, A.refit_loops, h, inliers, kept, rms);
    if (A.inlier) {
      const int src_first = A.ranges[4 * e], src_cap = A.ranges[4 * e + 1];
      const int *index = S.index + (size_t)e * S.cap16;
      for (int p = tid; p < n; p += FUND_SLOTS) {
        float a[3], b[3];
        cand.load(p, a, b);
        const int i = index[p];
        if (align_error2(h, a[0], a[1], a[2], b[0], b[1], b[2]) < S.thresh2 && (unsigned)i < (unsigned)src_cap)
          A.inlier[(size_t)src_first + (size_t)i] = 1;
      }
    }
  }
  if (tid != 0) return;
  float *out = A.sim + 16 * (size_t)e;
  const bool ok = status == ALIGN_OK;
#pragma unroll
  for (int j = 0; j < ALIGN_PARAMS; j++) out[j] = ok ? pose_one_nan(h[j]) : 0.0f;
  out[13] = ok ? rms : 0.0f;
  out[14] = 0.0f;
  out[15] = 0.0f;
  A.cand[e] = meta[2];
  A.inliers[e] = inliers;
  A.status[e] = status;
  atomicAdd(&A.summary[ok ? 0 : status + 1], 1);
  if (ok) {
    atomicAdd(&A.summary[1], inliers);
    atomicAdd(&A.summary[5], kept);
  }
  atomicAdd(&A.summary[4], meta[2]);
}

// ---- misift_correspond_tracks_batch

struct CorrespondArgs {
  const int *record_obs_a, *offsets_a, *summary_a;
  const int *record_obs_b, *offsets_b, *summary_b;
  int max_records_a, max_tracks_a, max_obs_a, max_records_b, max_tracks_b, max_obs_b;
  long long shift;
  int *tmin, *tmax;                            // temp: max_tracks_a each
  int *map, *summary;
};

__global__ __launch_bounds__(256) void correspond_tie_kernel(CorrespondArgs A)
{
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= A.max_records_a) return;
  const long long gb = g - A.shift;
  if (gb < 0 || gb >= A.max_records_b) return;
  const int TA = scene_clamp(A.summary_a[2], A.max_tracks_a), OA = scene_clamp(A.summary_a[3], A.max_obs_a);
  const int TB = scene_clamp(A.summary_b[2], A.max_tracks_b), OB = scene_clamp(A.summary_b[3], A.max_obs_b);
  const int oa = A.record_obs_a[g], ob = A.record_obs_b[gb];
  if ((unsigned)oa >= (unsigned)OA || (unsigned)ob >= (unsigned)OB) return;   // indices from device memory
  const int ta = align_track_of(A.offsets_a, TA, oa), tb = align_track_of(A.offsets_b, TB, ob);
  if (ta < 0 || tb < 0) return;
  atomicMin(&A.tmin[ta], tb);
  atomicMax(&A.tmax[ta], tb);
  atomicAdd(&A.summary[2], 1);
}

__global__ __launch_bounds__(256) void correspond_map_kernel(CorrespondArgs A)
{
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int TA = scene_clamp(A.summary_a[2], A.max_tracks_a);
  if (t == 0) {
    A.summary[0] = TA;
    A.summary[1] = scene_clamp(A.summary_b[2], A.max_tracks_b);
  }
  if (t >= TA) return;
  const int lo = A.tmin[t], hi = A.tmax[t];
  const int m = hi < 0 ? -1 : (lo == hi ? lo : -2);
  A.map[t] = m;
  if (m >= 0) atomicAdd(&A.summary[3], 1);
  if (m == -2) atomicAdd(&A.summary[4], 1);
}

// ---- misift_transform_scene_batch

struct TransformArgs {
  const float *sim;
  const int *sim_status;                       // or NULL
  const int *export_summary;
  int max_tracks, nimages;
  const float *points;
  const int *point_status;
  const float *cam;
  const int *cam_pair;
  float *points_out, *cam_out;
};

__global__ __launch_bounds__(256) void transform_scene_kernel(TransformArgs A)
{
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool apply = !A.sim_status || A.sim_status[0] == 0;
  float sim[ALIGN_PARAMS];
#pragma unroll
  for (int j = 0; j < ALIGN_PARAMS; j++) sim[j] = A.sim[j];
  if (k < A.max_tracks) {
    const int T = scene_clamp(A.export_summary[2], A.max_tracks);
    const unsigned *in = reinterpret_cast<const unsigned *>(A.points) + 4 * k;
    unsigned w[4] = {in[0], in[1], in[2], in[3]};                // copied bit for bit unless transformed
    if (apply && k < T && A.point_status[k] == 0) {
      const float X[3] = {__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2])};
      float Y[3];
      align_transform_point(sim, X, Y);
#pragma unroll
      for (int j = 0; j < 3; j++) w[j] = __float_as_uint(Y[j]);
    }
    unsigned *out = reinterpret_cast<unsigned *>(A.points_out) + 4 * k;
#pragma unroll
    for (int j = 0; j < 4; j++) out[j] = w[j];
  }
  if (k < A.nimages) {
    const unsigned *in = reinterpret_cast<const unsigned *>(A.cam) + 12 * k;
    unsigned wds[12];
#pragma unroll
    for (int j = 0; j < 12; j++) wds[j] = in[j];
    if (apply && A.cam_pair[k] != POSEGRAPH_UNSET) {
      float c[12], o[12];
#pragma unroll
      for (int j = 0; j < 12; j++) c[j] = __uint_as_float(wds[j]);
      align_transform_camera(sim, c, o);
#pragma unroll
      for (int j = 0; j < 12; j++) wds[j] = __float_as_uint(o[j]);
    }
    unsigned *out = reinterpret_cast<unsigned *>(A.cam_out) + 12 * k;
#pragma unroll
    for (int j = 0; j < 12; j++) out[j] = wds[j];
  }
}

}  // namespace

bool align_points_batch_one_launch(int nsel, int max_cap, int num_loops)
{
  return ransac_one_launch(nsel, max_cap, num_loops);
}

// Enqueue misift_align_points_batch on the context stream (common.hpp): one memset and five launches.  h_ranges and
// h_seeds are the pinned host copies; max_cap is the largest src_cap among them.
int launch_align_points_batch(misift_ctx *ctx, const float *d_src, const int *d_src_status, const float *d_dst,
                              const int *d_dst_status, const int *d_map, int nsel, const int *h_ranges,
                              const unsigned *h_seeds, int max_cap, const int *d_count, int count_stride, int num_loops,
                              float thresh2, int min_inliers, int refit_loops, float *d_sim, int *d_align_cand,
                              int *d_align_inliers, int *d_align_status, int *d_inlier, int *d_summary)
{
  const RansacNames names{"misift_align_points_batch", "candidates", "align_gather", "align_solve", "align_count",
                          "align_pick"};
  AlignArgs A{};
  int rc = ransac_search(names, nsel, max_cap, num_loops, thresh2, h_seeds, A.rs);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(d_summary, 0, 8 * sizeof(int), ctx->stream));
  if (nsel == 0) return MISIFT_OK;
  void *tail;
  rc = ransac_temp<AlignModel>(ctx, A.rs, 0, ALIGN_TAIL, &tail);
  if (rc) return rc;
  A.cur = static_cast<float *>(tail);
  A.src = d_src; A.dst = d_dst; A.src_status = d_src_status; A.dst_status = d_dst_status; A.map = d_map;
  A.ranges = h_ranges; A.count = d_count; A.count_stride = count_stride;
  A.min_inliers = min_inliers; A.refit_loops = refit_loops;
  A.sim = d_sim; A.cand = d_align_cand; A.inliers = d_align_inliers; A.status = d_align_status; A.inlier = d_inlier;
  A.summary = d_summary;
  rc = ransac_launches<AlignModel>(
      ctx, names, A, [&] { hipLaunchKernelGGL(align_gather_kernel, dim3(nsel), dim3(1024), 0, ctx->stream, A); },
      align_solve_kernel, [&] { hipLaunchKernelGGL(align_pick_kernel, dim3(nsel), dim3(1024), 0, ctx->stream, A); });
  if (rc) return rc;
  return ransac_scope(ctx, "align_refit", [&] {
    hipLaunchKernelGGL(align_refit_kernel, dim3(nsel), dim3(FUND_SLOTS), 0, ctx->stream, A);
  });
}

// Enqueue misift_correspond_tracks_batch: three memsets and two launches; temp: two ints per track of A's capacity.
int launch_correspond_tracks_batch(misift_ctx *ctx, int shift, int max_records_a, const int *d_record_obs_a,
                                   int max_tracks_a, int max_obs_a, const int *d_track_offsets_a,
                                   const int *d_export_summary_a, int max_records_b, const int *d_record_obs_b,
                                   int max_tracks_b, int max_obs_b, const int *d_track_offsets_b,
                                   const int *d_export_summary_b, int *d_map, int *d_summary)
{
  const int rc = misift_ensure_tmp(ctx, 2 * sizeof(int) * (size_t)max_tracks_a);
  if (rc) return rc;
  CorrespondArgs A{};
  A.record_obs_a = d_record_obs_a; A.offsets_a = d_track_offsets_a; A.summary_a = d_export_summary_a;
  A.record_obs_b = d_record_obs_b; A.offsets_b = d_track_offsets_b; A.summary_b = d_export_summary_b;
  A.max_records_a = max_records_a; A.max_tracks_a = max_tracks_a; A.max_obs_a = max_obs_a;
  A.max_records_b = max_records_b; A.max_tracks_b = max_tracks_b; A.max_obs_b = max_obs_b;
  A.shift = shift;
  A.tmin = reinterpret_cast<int *>(ctx->d_match_tmp);
  A.tmax = A.tmin + max_tracks_a;
  A.map = d_map; A.summary = d_summary;
  HIP_TRY(hipMemsetAsync(d_summary, 0, 8 * sizeof(int), ctx->stream));
  HIP_TRY(hipMemsetAsync(A.tmin, 0x7f, sizeof(int) * (size_t)max_tracks_a, ctx->stream));
  HIP_TRY(hipMemsetAsync(A.tmax, 0xff, sizeof(int) * (size_t)max_tracks_a, ctx->stream));
  int r;
  {
    LaunchScope ls(ctx, "correspond_tie");
    hipLaunchKernelGGL(correspond_tie_kernel, dim3((unsigned)(((long long)max_records_a + 255) / 256)), dim3(256), 0,
                       ctx->stream, A);
    r = ls.finish();
    if (r) return r;
  }
  LaunchScope ls(ctx, "correspond_map");
  hipLaunchKernelGGL(correspond_map_kernel, dim3((unsigned)(((long long)max_tracks_a + 255) / 256)), dim3(256), 0,
                     ctx->stream, A);
  return ls.finish();
}

// Enqueue misift_transform_scene_batch: one launch, no temp.
int launch_transform_scene_batch(misift_ctx *ctx, const float *d_sim, const int *d_sim_status, int max_tracks,
                                 const int *d_export_summary, const float *d_points, const int *d_point_status,
                                 int nimages, const float *d_cam, const int *d_cam_pair, float *d_points_out,
                                 float *d_cam_out)
{
  TransformArgs A{d_sim, d_sim_status, d_export_summary, max_tracks, nimages, d_points, d_point_status,
                  d_cam, d_cam_pair, d_points_out, d_cam_out};
  const long long n = max_tracks > nimages ? max_tracks : nimages;
  LaunchScope ls(ctx, "transform_scene");
  hipLaunchKernelGGL(transform_scene_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, A);
  return ls.finish();
}

// Test-only, host-only: the draw, the solve, the refit and the camera transform as the kernels compute them
// (align_core.hpp).
extern "C" int misift_test_align_samples(unsigned seed, int n, int num_loops, int *out)
{
  if (n < ALIGN_SAMPLE || num_loops < 0 || (num_loops > 0 && !out)) {
    misift_set_error("misift_test_align_samples: invalid argument");
    return MISIFT_EINVAL;
  }
  ransac_host_samples(seed, n, num_loops, out, align_draw3<LibcRandArrayRing>);
  return MISIFT_OK;
}

extern "C" int misift_test_align_solve(const float *a9, const float *b9, float *out13, int *valid)
{
  if (!a9 || !b9 || !out13 || !valid) {
    misift_set_error("misift_test_align_solve: invalid argument");
    return MISIFT_EINVAL;
  }
  float a[3][3], b[3][3], h[ALIGN_PARAMS];
  for (int k = 0; k < 3; k++)
    for (int j = 0; j < 3; j++) { a[k][j] = a9[3 * k + j]; b[k][j] = b9[3 * k + j]; }
  *valid = align_solve3(a, b, h) ? 1 : 0;
  for (int j = 0; j < ALIGN_PARAMS; j++) out13[j] = h[j];
  return MISIFT_OK;
}

namespace {
struct AlignHostCand {
  const float *a, *b;                          // n x 3 each
  void load(int p, float (&x)[3], float (&y)[3]) const
  {
    for (int k = 0; k < 3; k++) { x[k] = a[3 * (size_t)p + k]; y[k] = b[3 * (size_t)p + k]; }
  }
};
}  // namespace

// step 6 on n candidates (a3, b3: n x 3) from the transform sim13, which is refitted in place; the 256 slots run one
// after another.  out_counts = members, refits kept; *rms the rms of the final members.
extern "C" int misift_test_align_refit(const float *a3, const float *b3, int n, float thresh, int refit_loops,
                                       float *sim13, int *out_counts, float *rms)
{
  if (!a3 || !b3 || n < 0 || refit_loops < 0 || !sim13 || !out_counts || !rms || !(thresh > 0.0f)) {
    misift_set_error("misift_test_align_refit: invalid argument");
    return MISIFT_EINVAL;
  }
  static FundamentalHostExec ex;               // 46 KiB: not on the stack
  const AlignHostCand cand{a3, b3};
  float h[ALIGN_PARAMS];
  for (int j = 0; j < ALIGN_PARAMS; j++) h[j] = sim13[j];
  const float thresh2 = thresh * thresh;
  align_refit(ex, cand, n, thresh2, refit_loops, h, out_counts[0], out_counts[1], *rms);
  for (int j = 0; j < ALIGN_PARAMS; j++) sim13[j] = h[j];
  return MISIFT_OK;
}

extern "C" int misift_test_transform_camera(const float *sim13, const float *cam12, float *out12)
{
  if (!sim13 || !cam12 || !out12) {
    misift_set_error("misift_test_transform_camera: invalid argument");
    return MISIFT_EINVAL;
  }
  float c[12], o[12];
  for (int j = 0; j < 12; j++) c[j] = cam12[j];
  align_transform_camera(sim13, c, o);
  for (int j = 0; j < 12; j++) out12[j] = o[j];
  return MISIFT_OK;
}

extern "C" int misift_test_transform_point(const float *sim13, const float *x3, float *out3)
{
  if (!sim13 || !x3 || !out3) {
    misift_set_error("misift_test_transform_point: invalid argument");
    return MISIFT_EINVAL;
  }
  const float X[3] = {x3[0], x3[1], x3[2]};
  float Y[3];
  align_transform_point(sim13, X, Y);
  for (int j = 0; j < 3; j++) out3[j] = Y[j];
  return MISIFT_OK;
}

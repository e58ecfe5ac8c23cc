// kernels_localize.hip — new frames placed against a reconstruction: misift_describe_points_batch gives every track
// point an 8-bit descriptor (the rounded mean of the rows its observations name) in the layout of a one-frame record
// set, so that misift_match_pairs_batch_i8 matches query frames against the points; misift_localize_frames_batch turns
// the match rows into cameras by batch RANSAC over 2-D/3-D correspondences and emits the inliers as a scene that
// misift_merge_scenes_batch takes as its scene A.  No reference counterpart.  The rules are localize_core.hpp, shared
// with the host-only test hooks (misift_host.hip); the search is ransac_batch.hpp's with resect's model
// (resect_model.hpp): the same draw, solve, count and entry results as misift_resect_cameras_batch.
//
// describe: one memset (the summary) and one launch.
//   describe_points_kernel  one wavefront per track, eight to a workgroup, on a grid of at most 1024 workgroups whose
//                           wavefronts walk the tracks in steps of the grid.  The work is a gather of 128-byte rows whose
//                           addresses come from a dependent load (slot -> frame, record -> count, offset -> row).
//                           Sixteen lanes share an observation and load 8 bytes of its row each, so one load instruction
//                           of the wavefront brings four rows; the loop takes two observations per lane group and turn,
//                           so eight rows are in flight.  The bytes are sign-extended into 64-bit sums (a track has up
//                           to 2^31 - 1 slots and 127 x that does not fit 32 bits; the adds are not what the kernel
//                           waits for).  Two __shfl_xor steps (16, 32) join the four lane groups; the lanes of group 0
//                           store 8 bytes of the mean each, and lanes 0 .. 35 the record's 576 bytes in 16-byte stores.
//                           The three sums of the summary are kept per wavefront, joined in LDS and added once per
//                           workgroup: one atomic per track made the launch twenty times longer.
// localise: one memset (the summary) and five launches whatever the data (nsel == 0: the memset, the pick and the emit):
//   localize_gather_kernel  one 1024-thread workgroup per entry: the ordered compaction of the frame's rows that are
//                           candidates (RansacCompaction), x, y, X, Y, Z and the row index of each, then the draw.
//   localize_solve_kernel   resect's solve (resect_solve_lane).
//   (count)                 ransac_count_kernel<LocalizeModel>.
//   localize_pick_kernel    the entry's results, the install, the summary (resect_entry_results); the finds an entry
//                           will emit and its picked hypothesis go to the tail of the temp.
//   localize_emit_kernel    one workgroup per entry: the integer prefix of the finds of the entries before it, then the
//                           count's own test of the picked hypothesis on every candidate, compacted in order.
// Not built: a renormalised mean, fp32 scene descriptors, a guided second pass, one find per point, a P3P
// solver, a local optimisation, device-side pairs.
#include <stdint.h>
#include <string.h>
#include "common.hpp"
#include "localize_core.hpp"
#include "ransac_batch.hpp"
#include "resect_model.hpp"

namespace {

struct DescribeArgs {
  DescribeIn in;
  DescribeOut out;
};

// the 8 bytes a lane holds of one contributing row, or zeros
__device__ __forceinline__ uint2 describe_load(const DescribeIn &D, bool has, const TrackObs *slot, int sub, bool &contributes)
{
  contributes = false;
  if (!has) return make_uint2(0u, 0u);
  const TrackObs ob = track_obs_load(slot);
  long long row;
  contributes = loc_contributes(D, ob, row);
  if (!contributes) return make_uint2(0u, 0u);
  const uint2 *p = reinterpret_cast<const uint2 *>(D.q + LOC_DESC_BYTES * row) + sub;       // d_q is 16-byte aligned
  return *p;
}

__device__ __forceinline__ void describe_add(long long (&acc)[8], const uint2 v)
{
#pragma unroll
  for (int k = 0; k < 4; k++) {
    acc[k] += (int)(v.x << (24 - 8 * k)) >> 24;              // byte k, sign-extended
    acc[4 + k] += (int)(v.y << (24 - 8 * k)) >> 24;
  }
}

constexpr int DESCRIBE_WAVES = 8;              // wavefronts, so tracks in flight, per workgroup: three workgroups fit a CU
constexpr int DESCRIBE_MAX_BLOCKS = 1024;      // the grid: every wavefront walks the tracks from its own in steps of the grid

__global__ __launch_bounds__(64 * DESCRIBE_WAVES) void describe_points_kernel(DescribeArgs A)
{
  __shared__ unsigned s_sum[3];                // described points, their observations, the other observations
  const DescribeIn &D = A.in;
  const TrackScene &S = D.s;
  const int lane = threadIdx.x & 63;
  const int T = scene_T(S);
  if (threadIdx.x < 3) s_sum[threadIdx.x] = 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    A.out.scene_count[0] = T;
    A.out.summary[0] = T;                      // the other sums are added behind the memset
  }
  __syncthreads();
  const int g = lane >> 4, sub = lane & 15;
  unsigned described = 0u, contributing = 0u, others = 0u;   // sums modulo 2^32, as the host's
  const long long step = (long long)gridDim.x * DESCRIBE_WAVES;
  for (long long tl = (long long)blockIdx.x * DESCRIBE_WAVES + (threadIdx.x >> 6); tl < T; tl += step) {
    const int t = (int)tl;                     // the whole wavefront
    int off, end;
    const bool valid = loc_track_range(S, t, off, end);
    long long acc[8];
#pragma unroll
    for (int k = 0; k < 8; k++) acc[k] = 0;
    int m = 0, idle = 0;
    for (long long o0 = off; o0 < end; o0 += 8) {
      const long long oa = o0 + g, ob = o0 + 4 + g;
      bool ca, cb;
      const uint2 va = describe_load(D, oa < end, S.obs + oa, sub, ca);
      const uint2 vb = describe_load(D, ob < end, S.obs + ob, sub, cb);
      describe_add(acc, va);
      describe_add(acc, vb);
      m += (ca ? 1 : 0) + (cb ? 1 : 0);
      idle += (oa < end && !ca ? 1 : 0) + (ob < end && !cb ? 1 : 0);
    }
    // the four lane groups joined: every lane ends with the sums of its 8 bytes over all rows
#pragma unroll
    for (int st = 16; st <= 32; st <<= 1) {
#pragma unroll
      for (int k = 0; k < 8; k++) acc[k] += __shfl_xor(acc[k], st, 64);
      m += __shfl_xor(m, st, 64);
      idle += __shfl_xor(idle, st, 64);
    }
    const bool desc = loc_described(S, t, valid, m);
    if (g == 0) {
      uint32_t w[2] = {0u, 0u};
      if (desc) {
#pragma unroll
        for (int k = 0; k < 8; k++) w[k >> 2] |= (uint32_t)(loc_mean(acc[k], m) & 0xff) << (8 * (k & 3));
      }
      uint2 *dst = reinterpret_cast<uint2 *>(A.out.scene_q + LOC_DESC_BYTES * (size_t)t) + sub;
      *dst = make_uint2(w[0], w[1]);
    }
    if (lane < LOC_REC_WORDS / 4) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (lane == 0 && desc) {
        const float *X = S.points + 4 * (size_t)t;
        v = make_uint4(loc_bits(X[0]), loc_bits(X[1]), loc_bits(X[2]), 0u);   // xpos, ypos, scale, sharpness
      }
      reinterpret_cast<uint4 *>(A.out.scene_recs + LOC_REC_WORDS * (size_t)t)[lane] = v;
    }
    if (lane == 0) A.out.members[t] = m;
    described += desc ? 1u : 0u;
    contributing += desc ? (unsigned)m : 0u;
    others += (unsigned)idle;
  }
  // one add per workgroup and sum: a hundred thousand adds to one address would be what the launch waits for
  if (lane == 0) {
    if (described) atomicAdd(&s_sum[0], described);
    if (contributing) atomicAdd(&s_sum[1], contributing);
    if (others) atomicAdd(&s_sum[2], others);
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_sum[threadIdx.x])
    atomicAdd(reinterpret_cast<unsigned *>(A.out.summary) + 1 + threadIdx.x, s_sum[threadIdx.x]);
}

// ---- localise

constexpr int LOC_TAIL = 2;                    // ints per entry behind the search's temp: the finds, the picked index

struct LocalizeArgs {
  RansacSearch rs;                             // coord: x, y, X, Y, Z of the candidates in row order; index: their rows;
                                               // meta[1] a done entry's status, [2] what d_res_cand gets
  TrackScene s;                                // max_tracks, export_summary, points, point_status; intrinsics: pinned
  BatchLayout rows;
  const int *frames, *images;                  // the pinned host copies: nsel each
  int max_pts;
  float min_score, max_ambiguity;
  int min_inliers, only_unset, install;
  float *cam;                                  // in/out: nimages x 12, written under install
  int *cam_pair;                               // in/out: nimages
  float *res_cam;
  int *res_cand, *res_inliers, *res_status, *summary;
  int *tail;                                   // temp: nsel x LOC_TAIL
  int max_found;
  int *found_offsets;
  TrackObs *found_obs;
  int *found_summary;
  float *found_points;
  int *found_views, *found_status, *found_map;
};

typedef ResectModelOf<LocalizeArgs, true> LocalizeModel;

__global__ __launch_bounds__(1024) void localize_gather_kernel(LocalizeArgs A)
{
  const RansacSearch &S = A.rs;
  const int e = blockIdx.x, tid = threadIdx.x;
  const int img = A.images[e];                 // checked on the host: in [0, nimages)
  int *meta = S.meta + (size_t)RANSAC_META * e;
  if (A.only_unset && A.cam_pair[img] != POSEGRAPH_UNSET) {
    if (tid == 0) { meta[0] = 0; meta[1] = RESECT_SKIPPED; meta[2] = 0; }
    return;
  }
  const int f = A.frames[e];                   // checked on the host: in [0, nframes_rows)
  const int count = A.rows.counts[f];
  if (count > A.max_pts) {                     // nothing of the frame is read
    if (tid == 0) { meta[0] = 0; meta[1] = RESECT_OVER; meta[2] = 0; }
    return;
  }
  const int nrows = count > 0 ? count : 0;
  const int T = scene_T(A.s);
  const int mc = S.cap16;                      // >= max_pts >= nrows
  float *coord = S.coord + (size_t)e * 5 * mc;
  int *index = S.index + (size_t)e * mc;
  const float *pts = reinterpret_cast<const float *>(A.rows.recs + A.rows.base(f));
  const RansacCompaction c = ransac_compaction();
  for (int i0 = 0; i0 < nrows; i0 += 1024) {
    const int i = i0 + tid;
    LocCandidate cand;
    const bool ok = i < nrows && loc_candidate(pts + (size_t)i * PT_WORDS, T, A.s.points, A.s.point_status, A.min_score,
                                               A.max_ambiguity, cand);
    const int pos = c.place(ok);
    if (ok && pos < mc) {
      coord[pos] = cand.x;
      coord[mc + pos] = cand.y;
      coord[2 * mc + pos] = cand.X;
      coord[3 * mc + pos] = cand.Y;
      coord[4 * mc + pos] = cand.Z;
      index[pos] = i;
    }
    c.next();
  }
  const int n = c.total();
  const int need = A.min_inliers > RESECT_SAMPLE ? A.min_inliers : RESECT_SAMPLE;
  if (n < need) {
    if (tid == 0) { meta[0] = 0; meta[1] = RESECT_FEW_CAND; meta[2] = n; }
    return;
  }
  if (tid < 64) {                              // wave 0
    ransac_draw<LocalizeModel>(S.seeds[e], n, S.sample + (size_t)e * RESECT_SAMPLE * S.lp, S.num_loops, S.lp);
    if (tid == 0) { meta[0] = n; meta[1] = 0; meta[2] = n; }
  }
}

__global__ __launch_bounds__(64) void localize_solve_kernel(LocalizeArgs A, int hblocks)
{
  __shared__ float s_m[RESECT_SOLVE_LDS];
  resect_solve_lane<LocalizeModel>(A, hblocks, s_m);
}

__global__ __launch_bounds__(1024) void localize_pick_kernel(LocalizeArgs A)
{
  const RansacSearch &S = A.rs;
  const int e = blockIdx.x, tid = threadIdx.x;
  if (e == 0 && tid == 0) A.summary[0] = scene_T(A.s);
  if (e >= S.nsel) return;                     // nsel == 0: the one workgroup that writes T
  const int *meta = S.meta + (size_t)RANSAC_META * e;
  const bool searched = meta[0] != 0;
  unsigned long long best = 0;
  if (searched) best = ransac_pick(S.hcount + (size_t)e * S.lp, S.num_loops);
  if (tid != 0) return;
  int picked = 0;
  const int status = resect_entry_results(A, e, searched, best, &picked);
  A.tail[LOC_TAIL * (size_t)e] = status == RESECT_OK ? ransac_pick_count(best) : 0;
  A.tail[LOC_TAIL * (size_t)e + 1] = picked;
}

// the sum of v over the 1024 threads of the workgroup, to every thread
__device__ __forceinline__ long long localize_block_sum(long long v, long long *s_part)
{
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  long long s = 0;
  for (int w = 0; w < 16; w++) s += s_part[w];
  return s;
}

__global__ __launch_bounds__(1024) void localize_emit_kernel(LocalizeArgs A)
{
  __shared__ long long s_part[16];
  const RansacSearch &S = A.rs;
  const int e = blockIdx.x, tid = threadIdx.x;
  long long before = 0, all = 0;
  for (int j = tid; j < S.nsel; j += 1024) {
    const int v = max(A.tail[LOC_TAIL * (size_t)j], 0);
    all += v;
    if (j < e) before += v;
  }
  before = localize_block_sum(before, s_part);
  all = localize_block_sum(all, s_part);
  if (e == 0 && tid == 0) {
    const int N = (int)min(all, (long long)0x7fffffff);
    const int written = min(N, A.max_found);
    A.found_summary[0] = N; A.found_summary[1] = N;
    A.found_summary[2] = written; A.found_summary[3] = written;
    A.found_summary[4] = written > 0 ? 1 : 0;
    A.found_summary[5] = 0; A.found_summary[6] = 0; A.found_summary[7] = 0;
    A.found_offsets[written] = written;        // closes the last track; [0] = 0 when there is none
    A.summary[7] = written;
  }
  if (e >= S.nsel) return;
  const int finds = A.tail[LOC_TAIL * (size_t)e];
  if (finds <= 0) return;                      // the whole workgroup
  const int *meta = S.meta + (size_t)RANSAC_META * e;
  const int n = min(meta[0], S.cap16), mc = S.cap16, lp = S.lp;
  const int idx = min(max(A.tail[LOC_TAIL * (size_t)e + 1], 0), S.num_loops - 1);
  const float *hyp = S.hyp + (size_t)e * 12 * lp;
  float a[12];
#pragma unroll
  for (int k = 0; k < 12; k++) a[k] = hyp[k * lp + idx];     // the floats the count tested, not the stored result
  const LocalizeModel::Lane ln = LocalizeModel::lane(A, e);
  const float *coord = S.coord + (size_t)e * 5 * mc;
  const int *index = S.index + (size_t)e * mc;
  const int f = A.frames[e], img = A.images[e];
  const SiftPointD *rows = A.rows.recs + A.rows.base(f);
  const int T = scene_T(A.s);
  const RansacCompaction c = ransac_compaction();
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + tid;
    bool in = false;
    float q[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (i < n) {
#pragma unroll
      for (int k = 0; k < 5; k++) q[k] = coord[k * mc + i];
      in = LocalizeModel::inlier(a, ln, q, S.thresh2);
    }
    const int pos = c.place(in);
    const long long find = before + pos;
    if (in && find < A.max_found) {
      int r = index[i];                        // from the temp: checked before it addresses anything
      r = (unsigned)r < (unsigned)A.max_pts ? r : 0;
      int t = rows[r].match;
      t = (unsigned)t < (unsigned)T ? t : 0;
      TrackObs ob;
      ob.frame = img; ob.record = r; ob.xpos = q[0]; ob.ypos = q[1];
      A.found_obs[find] = ob;
      A.found_offsets[find] = (int)find;
      A.found_map[find] = t;
      const float *P = A.s.points + 4 * (size_t)t;
      float *Q = A.found_points + 4 * (size_t)find;
#pragma unroll
      for (int k = 0; k < 4; k++) Q[k] = __uint_as_float(loc_bits(P[k]));   // bit copies
      A.found_views[find] = 1;
      A.found_status[find] = 0;
    }
    c.next();
  }
}

}  // namespace

// Enqueue misift_describe_points_batch on the context stream (common.hpp): one memset and one launch.
int launch_describe_points_batch(misift_ctx *ctx, const DescribeIn &in, const DescribeOut &out)
{
  HIP_TRY(hipMemsetAsync(out.summary, 0, 8 * sizeof(int), ctx->stream));
  const DescribeArgs A{in, out};
  LaunchScope ls(ctx, "describe_points");
  const long long need = ((long long)in.s.max_tracks + DESCRIBE_WAVES - 1) / DESCRIBE_WAVES;
  const unsigned blocks = (unsigned)(need < DESCRIBE_MAX_BLOCKS ? need : DESCRIBE_MAX_BLOCKS);
  hipLaunchKernelGGL(describe_points_kernel, dim3(blocks), dim3(64 * DESCRIBE_WAVES), 0, ctx->stream, A);
  return ls.finish();
}

bool localize_frames_batch_one_launch(int nsel, int max_pts, int num_loops)
{
  return ransac_one_launch(nsel, max_pts, num_loops);
}

size_t localize_frames_batch_tmp_bytes(int nsel, int max_pts, int num_loops)
{
  RansacSearch S{};
  S.nsel = nsel; S.cap16 = ransac_round16(max_pts); S.lp = ransac_round16(num_loops);
  return ransac_tmp_bytes<LocalizeModel>(S, 0, LOC_TAIL);
}

// Enqueue misift_localize_frames_batch on the context stream (common.hpp): one memset and five launches.
int launch_localize_frames_batch(misift_ctx *ctx, const TrackScene &scene, const LocalizeCall &call)
{
  const RansacNames names{"misift_localize_frames_batch", "rows", "localize_gather", "localize_solve", "localize_count",
                          "localize_pick"};
  const int nsel = call.nsel;
  LocalizeArgs A{};
  void *tail = nullptr;
  int rc = ransac_search(names, nsel, call.max_pts, call.num_loops, call.thresh2, call.h_seeds, A.rs);
  if (!rc) rc = ransac_temp<LocalizeModel>(ctx, A.rs, 0, LOC_TAIL, &tail);
  if (rc) return rc;
  A.s = scene;
  A.rows = call.rows;
  A.frames = call.h_frames; A.images = call.h_images;
  A.max_pts = call.max_pts;
  A.min_score = call.min_score; A.max_ambiguity = call.max_ambiguity;
  A.min_inliers = call.min_inliers; A.only_unset = call.only_unset; A.install = call.install;
  A.cam = call.d_cam; A.cam_pair = call.d_cam_pair;
  A.res_cam = call.d_res_cam; A.res_cand = call.d_res_cand; A.res_inliers = call.d_res_inliers;
  A.res_status = call.d_res_status; A.summary = call.d_summary;
  A.tail = reinterpret_cast<int *>(tail);
  A.max_found = call.max_found;
  A.found_offsets = call.d_found_offsets; A.found_obs = call.d_found_obs; A.found_summary = call.d_found_summary;
  A.found_points = call.d_found_points; A.found_views = call.d_found_views; A.found_status = call.d_found_status;
  A.found_map = call.d_found_map;
  HIP_TRY(hipMemsetAsync(call.d_summary, 0, 8 * sizeof(int), ctx->stream));
  const auto pick = [&] {
    hipLaunchKernelGGL(localize_pick_kernel, dim3(max(nsel, 1)), dim3(1024), 0, ctx->stream, A);
  };
  const auto emit = [&] {
    hipLaunchKernelGGL(localize_emit_kernel, dim3(max(nsel, 1)), dim3(1024), 0, ctx->stream, A);
  };
  if (nsel == 0) {
    rc = ransac_scope(ctx, names.pick, pick);
    return rc ? rc : ransac_scope(ctx, "localize_emit", emit);
  }
  rc = ransac_launches<LocalizeModel>(
      ctx, names, A,
      [&] { hipLaunchKernelGGL(localize_gather_kernel, dim3(nsel), dim3(1024), 0, ctx->stream, A); },
      localize_solve_kernel, pick);
  return rc ? rc : ransac_scope(ctx, "localize_emit", emit);
}

// kernels_filter.hip — misift_filter_tracks_batch: the observation lists of misift_export_tracks_batch gated against the
// current points and cameras and written out again, compact and in export's own format, so that triangulate, refine,
// resect and adjust take them unchanged.  No reference counterpart.  The rules are filter_core.hpp, shared with the
// host-only test hook at the end of this file.
//
// One copy (the intrinsics into temp), three memsets (the owners, the tile sums, the summary) and six launches, whatever
// the data:
//   cand_owner_kernel        the owner of every slot: launch_track_candidates (track_candidates.hpp) without the keys.
//   filter_classify_kernel   one lane per slot: rule 1.  The reason goes to code[] and, where d_obs_map is given, there; a
//                            survivor's unit ray and e2 go to ray[] as one 16-byte store.
//   filter_track_kernel      one wavefront per track, four to a workgroup: the two pairwise rules.  The lanes stride over
//                            the track's views; the first FILTER_STAGE of them (ray, e2, frame) are staged in LDS, 20 bytes
//                            a view, the rest are read from temp, which is L2-resident.  Every lane walks all the views
//                            in the same order, so an LDS read is a broadcast.  Pass A marks the duplicates, the kept
//                            views are counted, pass B looks for one pair of rays wide enough apart and ends at the first
//                            found.  The track's m, or 0 when it is dropped, goes to keep[], and its share to the sums of
//                            its tile of 2048 tracks by one 64-bit integer atomic.
//   filter_scan_kernel       ONE workgroup: the exclusive prefix sum of the tile sums, T' and O' to both summaries.
//   filter_apply_kernel      per tile: the exclusive scan inside the tile on top of its prefix: t' and off' of every
//                            surviving track; its point, its offsets and its d_track_map entry.
//   filter_write_kernel      one wavefront per surviving track: the kept views of 64 slots at a time ranked by ballot and
//                            popcount, copied as 16 bytes each; the rms from the kept e2 in ascending slot.
// No workgroup waits for another.  Every sum but that rms is an integer sum, so the outputs are byte-identical from run
// to run.
#include <stdint.h>
#include <string.h>
#include "common.hpp"
#include "filter_core.hpp"
#include "scan_core.hpp"
#include "track_candidates.hpp"

namespace {

constexpr int FILTER_THREADS = 256;
constexpr int FILTER_WAVES = FILTER_THREADS / 64;
// views of a track staged in LDS: 20 bytes each, 20 KiB a workgroup, so the eight workgroups that fill a CU's 32 wave
// slots take exactly its 160 KiB and the staging costs no occupancy; a longer track reads the rest from temp
constexpr int FILTER_STAGE = 256;
constexpr int FILTER_TILE = 2048;              // tracks per scan tile: 256 lanes x 8
constexpr int FILTER_SCAN_WG = 1024;

struct FilterArgs {
  TrackScene s;                                // intrinsics: the device copy in temp
  const int *owner;                            // temp, max_obs
  float E2, max_cos;
  int min_views, unique_frames, ntiles;
  float4 *ray;                                 // temp, max_obs: a survivor's unit ray and e2
  int *code;                                   // temp, max_obs: 0 for a kept view, otherwise the reason
  int *keep;                                   // temp, max_tracks: m of a surviving track, else 0
  int *newoff;                                 // temp, max_tracks: off' of a surviving track
  unsigned long long *tile;                    // temp, ntiles: (m summed << 32) | surviving tracks, then the prefix sums
  int *track_offsets_out;
  int4 *obs_out;
  int *export_summary_out;
  float *points_out;
  int *point_views_out, *point_status_out, *track_map, *obs_map, *summary;
};

__device__ __forceinline__ int wave_sum(int v)
{
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(FILTER_THREADS) void filter_classify_kernel(FilterArgs A)
{
  const int o = blockIdx.x * FILTER_THREADS + threadIdx.x;   // below max_obs + 256: no overflow
  int code = 0;
  const bool live = o < scene_O(A.s);
  if (live) {
    float e2, u[3];
    const TrackObs ob = track_obs_load(A.s.obs + o);
    code = filter_classify(TriCamsPlain{A.s.cam, A.s.cam_pair, A.s.intrinsics}, A.s.nimages, A.owner[o], A.s.point_status,
                           A.s.points, ob, A.E2, e2, u);
    A.code[o] = code;
    A.ray[o] = make_float4(u[0], u[1], u[2], e2);
    if (A.obs_map && code < 0) A.obs_map[o] = code;
  }
  const int behind = wave_sum(live && code == FILTER_BEHIND), error = wave_sum(live && code == FILTER_ERROR);
  const int other = wave_sum(live && code < 0 && code >= FILTER_NOT_USABLE);
  if ((threadIdx.x & 63) == 0) {
    if (behind) atomicAdd(&A.summary[2], behind);
    if (error) atomicAdd(&A.summary[3], error);
    if (other) atomicAdd(&A.summary[7], other);
  }
}

// view j of the track at off, as its wavefront sees it: the frame of a view that counts (-1 otherwise) and its ray.
// with_lost: a duplicate that pass A has marked still counts, as the survivor it was.
struct FilterTrackView {
  const FilterArgs &A;
  const float4 *s_ray;
  const int *s_fr;
  int t, off;
  __device__ __forceinline__ int at(int j, bool with_lost, float4 &r) const
  {
    if (j < FILTER_STAGE) {
      r = s_ray[j];
      return s_fr[j];
    }
    const int o = off + j;
    r = A.ray[o];
    if (A.owner[o] != t) return -1;
    const int c = A.code[o];
    return c == 0 || (with_lost && c == FILTER_DUPLICATE) ? A.s.obs[o].frame : -1;
  }
};

__global__ __launch_bounds__(FILTER_THREADS) void filter_track_kernel(FilterArgs A)
{
  __shared__ float4 s_ray[FILTER_WAVES][FILTER_STAGE];
  __shared__ int s_fr[FILTER_WAVES][FILTER_STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long tl = (long long)blockIdx.x * FILTER_WAVES + wave;
  if (tl >= scene_T(A.s)) return;               // the same in every lane of the wavefront; no workgroup barrier below
  const int t = (int)tl, O = scene_O(A.s);
  const int off = A.s.track_offsets[t], end = A.s.track_offsets[t + 1];
  int result = 0;
  if (!tri_range_ok(off, end, O)) result = FILTER_NO_OWNER;    // before it addresses anything
  else if (filter_bad_point(A.s.point_status[t], A.s.points + 4 * (size_t)t)) result = FILTER_BAD_POINT;
  int m = 0;
  if (result == 0) {
    const int n = end - off;
    float4 *ray = s_ray[wave];
    int *fr = s_fr[wave];
    const FilterTrackView V{A, ray, fr, t, off};
    // a view counts when this track owns its slot and rule 1 left it a survivor
    for (int k = lane; k < min(n, FILTER_STAGE); k += 64) {
      const int o = off + k;
      ray[k] = A.ray[o];
      fr[k] = A.owner[o] == t && A.code[o] == 0 ? A.s.obs[o].frame : -1;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int lost = 0;
    if (A.unique_frames) {
      // pass A: LDS and code[] keep counting a marked duplicate as the survivor it was, so the marks disturb nothing
      for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        float4 mine = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const int f = k < n ? V.at(k, false, mine) : -1;
        if (!__any(f >= 0)) continue;
        bool loses = false;
        for (int j = 0; j < n; j++) {
          float4 r;
          const int fj = V.at(j, true, r);
          loses = loses || (f >= 0 && fj == f && j != k && filter_loses(mine.w, k, r.w, j));
        }
        if (loses) A.code[off + k] = FILTER_DUPLICATE;
        if (loses && A.obs_map) A.obs_map[off + k] = FILTER_DUPLICATE;
        lost += loses;
      }
      __threadfence();                         // the marks beyond the staged views are read by other lanes below
      for (int k = lane; k < min(n, FILTER_STAGE); k += 64)
        if (fr[k] >= 0 && A.code[off + k] != 0) fr[k] = -1;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      lost = wave_sum(lost);
      if (lane == 0 && lost) atomicAdd(&A.summary[4], lost);
    }
    for (int k = lane; k < n; k += 64) {
      float4 r;
      m += V.at(k, false, r) >= 0;
    }
    m = wave_sum(m);
    if (m < A.min_views) {
      result = FILTER_FEW_VIEWS;
    } else if (A.max_cos < INFINITY) {
      // pass B: one pair wide enough apart is all it takes
      bool wide = false;
      for (int k0 = 0; k0 < n && !wide; k0 += 64) {
        const int k = k0 + lane;
        float4 mine = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const bool have = k < n && V.at(k, false, mine) >= 0;
        if (!__any(have)) continue;
        const float a[3] = {mine.x, mine.y, mine.z};
        for (int j0 = 0; j0 < n && !wide; j0 += 16) {
          bool found = false;
          for (int j = j0; j < min(n, j0 + 16); j++) {
            float4 r;
            const bool other = V.at(j, false, r) >= 0 && j != k;
            const float b[3] = {r.x, r.y, r.z};
            found = found || (have && other && filter_pair_wide(a, b, A.max_cos));
          }
          wide = __any(found);
        }
      }
      if (!wide) result = FILTER_NARROW;
    }
    if (result < 0) {
      // the kept views of a dropped track take its reason
      for (int k = lane; k < n; k += 64) {
        float4 r;
        if (V.at(k, false, r) < 0) continue;
        A.code[off + k] = result;
        if (A.obs_map) A.obs_map[off + k] = result;
      }
    }
  }
  if (lane != 0) return;
  A.keep[t] = result == 0 ? m : 0;
  if (result < 0) {
    A.track_map[t] = result;
    if (result == FILTER_FEW_VIEWS) atomicAdd(&A.summary[5], 1);
    if (result == FILTER_NARROW) atomicAdd(&A.summary[6], 1);
  } else {
    atomicAdd(&A.tile[t / FILTER_TILE], ((unsigned long long)(unsigned)m << 32) | 1ull);   // at most 2048 per tile: no carry
  }
}

__global__ __launch_bounds__(FILTER_SCAN_WG) void filter_scan_kernel(FilterArgs A)
{
  __shared__ uint2 red[FILTER_SCAN_WG / 64];
  uint2 carry = make_uint2(0, 0);
  for (int t0 = 0; t0 < A.ntiles; t0 += FILTER_SCAN_WG) {
    const int t = t0 + threadIdx.x;
    const unsigned long long w = t < A.ntiles ? A.tile[t] : 0ull;
    const uint2 v = make_uint2((unsigned)w, (unsigned)(w >> 32));
    uint2 total;
    const uint2 ex = exp_block_scan<FILTER_SCAN_WG / 64>(v, red, total);
    if (t < A.ntiles) A.tile[t] = ((unsigned long long)(carry.y + ex.y) << 32) | (carry.x + ex.x);
    carry.x += total.x; carry.y += total.y;
  }
  if (threadIdx.x == 0) {
    A.summary[0] = A.export_summary_out[0] = A.export_summary_out[2] = (int)carry.x;
    A.summary[1] = A.export_summary_out[1] = A.export_summary_out[3] = (int)carry.y;
    A.export_summary_out[4] = A.export_summary_out[5] = A.export_summary_out[6] = A.export_summary_out[7] = 0;
    A.track_offsets_out[0] = 0;
  }
}

__global__ __launch_bounds__(256) void filter_apply_kernel(FilterArgs A)
{
  __shared__ uint2 red[4];
  __shared__ int s_longest[4];
  const int T = scene_T(A.s), O = scene_O(A.s);
  int longest = 0;
  for (int tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
    const long long i0 = (long long)tile * FILTER_TILE + threadIdx.x * 8;
    int v[8];
    uint2 mine = make_uint2(0, 0);
    for (int k = 0; k < 8; k++) {
      v[k] = i0 + k < T ? A.keep[i0 + k] : 0;  // keep[] is written below T only
      mine.x += v[k] > 0; mine.y += (unsigned)v[k];
    }
    uint2 total;
    uint2 ex = exp_block_scan<4>(mine, red, total);
    const unsigned long long before = A.tile[tile];
    ex.x += (unsigned)before; ex.y += (unsigned)(before >> 32);
    for (int k = 0; k < 8; k++) {
      const int m = v[k];
      if (m <= 0) continue;
      const int t = (int)(i0 + k), tn = (int)ex.x, off = (int)ex.y;
      ex.x += 1; ex.y += (unsigned)m;
      // tn <= t and off + m <= O by construction (the kept views are distinct slots); checked all the same
      if (tn < 0 || tn > t || off < 0 || (long long)off + m > O) {
        A.keep[t] = 0;
        continue;
      }
      A.newoff[t] = off;
      A.track_map[t] = tn;
      A.track_offsets_out[tn + 1] = off + m;
      A.point_views_out[tn] = m;
      A.point_status_out[tn] = 0;
      const unsigned *src = reinterpret_cast<const unsigned *>(A.s.points) + 4 * (size_t)t;
      unsigned *dst = reinterpret_cast<unsigned *>(A.points_out) + 4 * (size_t)tn;
      dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
      longest = max(longest, m);
    }
  }
  for (int o = 32; o > 0; o >>= 1) longest = max(longest, __shfl_xor(longest, o, 64));
  if ((threadIdx.x & 63) == 0) s_longest[threadIdx.x >> 6] = longest;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) longest = max(longest, s_longest[w]);
    if (longest) atomicMax(&A.export_summary_out[4], longest);
  }
}

__global__ __launch_bounds__(FILTER_THREADS) void filter_write_kernel(FilterArgs A)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long tl = (long long)blockIdx.x * FILTER_WAVES + wave;
  if (tl >= scene_T(A.s)) return;
  const int t = (int)tl;
  const int m = A.keep[t];
  if (m <= 0) return;                          // a surviving track has a valid range: the track launch checked it
  const int off = A.s.track_offsets[t], end = A.s.track_offsets[t + 1];
  const int tn = A.track_map[t], at = A.newoff[t];
  int base = 0;
  float s = 0.0f;
  for (int o0 = off; o0 < end; o0 += 64) {
    const int o = o0 + lane;
    const bool kept = o < end && A.owner[o] == t && A.code[o] == 0;
    const float e2 = kept ? A.ray[o].w : 0.0f;
    unsigned long long mask = __ballot(kept);
    const int rank = base + __popcll(mask & ((1ull << lane) - 1ull));
    if (kept && rank < m) {                    // rank < m always: m is this count
      const TrackObs ob = track_obs_load(A.s.obs + o);
      A.obs_out[at + rank] = make_int4(ob.frame, ob.record, __float_as_int(ob.xpos), __float_as_int(ob.ypos));
      if (A.obs_map) A.obs_map[o] = at + rank;
    }
    base += __popcll(mask);
    while (mask) {                             // the kept e2 in ascending slot, one term at a time
      const int j = __ffsll((long long)mask) - 1;
      s = s + __shfl(e2, j, 64);
      mask &= mask - 1;
    }
  }
  if (lane == 0) A.points_out[4 * (size_t)tn + 3] = filter_rms(s, m);
}

size_t filter_align16(size_t v) { return (v + 15) / 16 * 16; }

}  // namespace

size_t filter_tracks_batch_tmp_bytes(int max_tracks, int max_obs, int nimages)
{
  const size_t ntiles = ((size_t)max_tracks + FILTER_TILE - 1) / FILTER_TILE;
  return 16 * (size_t)max_obs + 2 * filter_align16(sizeof(int) * (size_t)max_obs) +
         2 * filter_align16(sizeof(int) * (size_t)max_tracks) + filter_align16(8 * ntiles) + 16 * (size_t)nimages;
}

// Enqueue misift_filter_tracks_batch on the context stream (common.hpp): a copy, three memsets and six launches.
int launch_filter_tracks_batch(misift_ctx *ctx, const TrackScene &scene, float thresh2, float max_cos, int min_views,
                               int unique_frames, int *d_track_offsets_out, void *d_obs_out, int *d_export_summary_out,
                               float *d_points_out, int *d_point_views_out, int *d_point_status_out, int *d_track_map,
                               int *d_obs_map, int *d_summary)
{
  const int max_tracks = scene.max_tracks, max_obs = scene.max_obs, nimages = scene.nimages;
  const int rc = misift_ensure_tmp(ctx, filter_tracks_batch_tmp_bytes(max_tracks, max_obs, nimages));
  if (rc) return rc;
  const size_t obs_ints = filter_align16(sizeof(int) * (size_t)max_obs);
  const size_t track_ints = filter_align16(sizeof(int) * (size_t)max_tracks);
  const int ntiles = (int)(((long long)max_tracks + FILTER_TILE - 1) / FILTER_TILE);
  const size_t tile_bytes = filter_align16(8 * (size_t)ntiles);
  char *t = reinterpret_cast<char *>(ctx->d_match_tmp);
  FilterArgs A;
  A.s = scene;
  A.ray = reinterpret_cast<float4 *>(t); t += 16 * (size_t)max_obs;
  int *owner = reinterpret_cast<int *>(t); t += obs_ints;
  A.owner = owner;
  A.code = reinterpret_cast<int *>(t); t += obs_ints;
  A.keep = reinterpret_cast<int *>(t); t += track_ints;
  A.newoff = reinterpret_cast<int *>(t); t += track_ints;
  A.tile = reinterpret_cast<unsigned long long *>(t); t += tile_bytes;
  float *d_intrinsics = reinterpret_cast<float *>(t);
  A.s.intrinsics = d_intrinsics;
  A.E2 = thresh2; A.max_cos = max_cos; A.min_views = min_views; A.unique_frames = unique_frames; A.ntiles = ntiles;
  A.track_offsets_out = d_track_offsets_out; A.obs_out = reinterpret_cast<int4 *>(d_obs_out);
  A.export_summary_out = d_export_summary_out; A.points_out = d_points_out; A.point_views_out = d_point_views_out;
  A.point_status_out = d_point_status_out; A.track_map = d_track_map; A.obs_map = d_obs_map; A.summary = d_summary;
  HIP_TRY(hipMemcpyAsync(d_intrinsics, scene.intrinsics, 16 * (size_t)nimages, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemsetAsync(owner, 0xff, sizeof(int) * (size_t)max_obs, ctx->stream));
  HIP_TRY(hipMemsetAsync(A.tile, 0, tile_bytes, ctx->stream));
  HIP_TRY(hipMemsetAsync(d_summary, 0, 8 * sizeof(int), ctx->stream));
  const int ncu = ctx->num_cus > 0 ? ctx->num_cus : 256;
  const dim3 wgrid((unsigned)(((long long)max_tracks + FILTER_WAVES - 1) / FILTER_WAVES));   // a wavefront per track
  int lrc;
  {
    LaunchScope ls(ctx, "filter_owner");
    launch_track_candidates(ctx, scene, owner, nullptr);
    if ((lrc = ls.finish())) return lrc;
  }
  {
    LaunchScope ls(ctx, "filter_classify");
    const dim3 per_slot((unsigned)(((long long)max_obs + FILTER_THREADS - 1) / FILTER_THREADS));
    hipLaunchKernelGGL(filter_classify_kernel, per_slot, dim3(FILTER_THREADS), 0, ctx->stream, A);
    if ((lrc = ls.finish())) return lrc;
  }
  {
    LaunchScope ls(ctx, "filter_track");
    hipLaunchKernelGGL(filter_track_kernel, wgrid, dim3(FILTER_THREADS), 0, ctx->stream, A);
    if ((lrc = ls.finish())) return lrc;
  }
  {
    LaunchScope ls(ctx, "filter_scan");
    hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(FILTER_SCAN_WG), 0, ctx->stream, A);
    if ((lrc = ls.finish())) return lrc;
  }
  {
    LaunchScope ls(ctx, "filter_apply");
    hipLaunchKernelGGL(filter_apply_kernel, dim3(ntiles < 8 * ncu ? ntiles : 8 * ncu), dim3(256), 0, ctx->stream, A);
    if ((lrc = ls.finish())) return lrc;
  }
  LaunchScope ls(ctx, "filter_write");
  hipLaunchKernelGGL(filter_write_kernel, wgrid, dim3(FILTER_THREADS), 0, ctx->stream, A);
  return ls.finish();
}

extern "C" int misift_test_filter_stage(void) { return FILTER_STAGE; }

// Test-only, host-only: the whole call on host arrays by the rules the kernels compile (filter_core.hpp).
extern "C" int misift_test_filter_tracks(int max_tracks, int max_obs, const int *track_offsets, const misift_track_obs *obs,
                                         const int *export_summary, const float *points, const int *point_status,
                                         int nimages, const float *cam, const int *cam_pair, const float *intrinsics,
                                         float max_error, float max_cos, int min_views, int unique_frames,
                                         int *track_offsets_out, misift_track_obs *obs_out, int *export_summary_out,
                                         float *points_out, int *point_views_out, int *point_status_out, int *track_map,
                                         int *obs_map, int *summary)
{
  const bool ok = max_tracks >= 1 && max_obs >= 1 && nimages >= 1 && track_offsets && obs && export_summary && points &&
                  point_status && cam && cam_pair && intrinsics && max_error > 0.0f && max_cos == max_cos &&
                  min_views >= 2 && (unique_frames == 0 || unique_frames == 1) && track_offsets_out && obs_out &&
                  export_summary_out && points_out && point_views_out && point_status_out && track_map && summary;
  if (!ok) {
    misift_set_error("misift_test_filter_tracks: invalid argument");
    return MISIFT_EINVAL;
  }
  const TrackScene S{max_tracks, max_obs, nimages, track_offsets, reinterpret_cast<const TrackObs *>(obs), export_summary,
                     points, point_status, cam, cam_pair, intrinsics};
  filter_tracks_host(S, max_error * max_error, max_cos, min_views, unique_frames, track_offsets_out,
                     reinterpret_cast<TrackObs *>(obs_out), export_summary_out, points_out, point_views_out,
                     point_status_out, track_map, obs_map, summary);
  return MISIFT_OK;
}

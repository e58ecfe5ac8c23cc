// kernels_posegraph.hip — misift_link_poses_batch: the pair poses of misift_recover_pose_batch joined into one frame.  A
// relative scale per link from the depths two pairs give the same point in the image they share, one propagation of the
// scales from a seed pair, and a camera per image by composing the scaled poses along a walk.  No reference counterpart.
// The arithmetic is posegraph_core.hpp, shared with the host-only test hooks at the end of this file.
//
// Two launches, whatever the data:
//   posegraph_ratio_kernel   one 256-thread workgroup per link.  Each thread walks its rows r = t, t + 256, ... of pair p:
//                            the partner row (range-checked), the edge rule on both rows, the four depths, rho = zq / zp.
//                            The bits of rho (0 for a row that is no sample) are staged in LDS for the first PG_STAGE rows
//                            and recomputed per pass behind them.  The lower median is a radix select over those bits,
//                            most significant byte first: a 256-bin LDS histogram of integer counts (LDS atomics), a
//                            wavefront shuffle scan of the bins, and the bin that holds the rank becomes the next byte of
//                            the prefix.  Four passes; the first also counts the samples.  The result is one of the
//                            samples and every count is an integer, so it depends on the sample set alone.
//                            One more workgroup, the last, prepares step 2 while the others run: it copies the three host
//                            lists out of the pinned slot into temp memory, decides which pair is usable, and sets the
//                            scales to 0, the cameras to twelve zeros and d_cam_pair to -2.
//   posegraph_solve_kernel   one wavefront.  The lists, the usable flags, the ratios, the scales, the cameras and
//                            d_cam_pair are a few KiB at the sizes the call is made for: the 64 lanes stage them in LDS
//                            when they fit PG_SERIAL_WORDS (4 words per link, 4 per pair, 1 per walk entry, 13 per image),
//                            and lane 0 then runs posegraph_solve on them: a dependent chain of LDS round trips instead of
//                            L2 round trips.  Otherwise the same function runs on the temp memory and the outputs.  Only the poses are read from global memory, twelve floats per placed
//                            image.  All lanes then write the staged scales, cameras and d_cam_pair back and reduce the
//                            summary over the links.
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "common.hpp"
#include "posegraph_core.hpp"

namespace {

constexpr int PG_THREADS = 256;
constexpr int PG_STAGE = 4096;                 // rows of a link whose rho bits are kept in LDS
constexpr int PG_SERIAL_WORDS = 12288;         // words of step 2's lists and state that are staged in LDS

struct PgArgs {
  const int *h_links, *h_pairs, *h_walk;       // pinned host copies of the caller's lists
  int npairs, nlinks, nwalk, nimages, max_pts, min_common, seed_pair, root_image;
  const SiftPointD *rows;
  const int *row_counts;
  const float *pose;
  const int *num_front;
  const float *xyz;
  float min_score, max_ambiguity, max_error;
  int use_error;
  int *tmp;                                    // links (3 nlinks) | pairs (2 npairs) | walk (nwalk) | usable (npairs)
  float *link_ratio;
  int *link_common;
  float *pair_scale, *cam;
  int *cam_pair, *summary;
};

// the last workgroup of the ratio launch: everything of step 2 that is not serial
__device__ void posegraph_prepare(const PgArgs &A)
{
  int *links = A.tmp, *pairs = links + 3 * (size_t)A.nlinks, *walk = pairs + 2 * (size_t)A.npairs;
  int *usable = walk + A.nwalk;
  for (int i = threadIdx.x; i < 3 * A.nlinks; i += PG_THREADS) links[i] = A.h_links[i];
  for (int i = threadIdx.x; i < 2 * A.npairs; i += PG_THREADS) pairs[i] = A.h_pairs[i];
  for (int i = threadIdx.x; i < A.nwalk; i += PG_THREADS) walk[i] = A.h_walk[i];
  for (int p = threadIdx.x; p < A.npairs; p += PG_THREADS) {
    usable[p] = posegraph_usable(A.pose + 12 * (size_t)p, A.num_front[p]) ? 1 : 0;
    A.pair_scale[p] = 0.0f;
  }
  for (int i = threadIdx.x; i < 12 * A.nimages; i += PG_THREADS) A.cam[i] = 0.0f;
  for (int i = threadIdx.x; i < A.nimages; i += PG_THREADS) A.cam_pair[i] = POSEGRAPH_UNSET;
}

__global__ __launch_bounds__(PG_THREADS) void posegraph_ratio_kernel(PgArgs A)
{
  __shared__ unsigned s_bits[PG_STAGE];
  __shared__ int s_hist[256], s_wsum[PG_THREADS / 64], s_bin, s_below;
  const int l = blockIdx.x, tid = threadIdx.x;
  if (l == A.nlinks) {
    posegraph_prepare(A);
    return;
  }
  const int p = A.h_links[3 * l], q = A.h_links[3 * l + 1], kind = A.h_links[3 * l + 2];   // checked by the host
  const int np = posegraph_rows(A.row_counts[p], A.max_pts), nq = posegraph_rows(A.row_counts[q], A.max_pts);
  const SiftPointD *rows_p = A.rows + (size_t)p * A.max_pts, *rows_q = A.rows + (size_t)q * A.max_pts;
  const float *xyz_p = A.xyz + 4 * (size_t)p * A.max_pts, *xyz_q = A.xyz + 4 * (size_t)q * A.max_pts;
  const auto sample = [&](int r) {
    return posegraph_sample(rows_p, xyz_p, rows_q, xyz_q, nq, kind, r, A.min_score, A.max_ambiguity, A.use_error != 0,
                            A.max_error);
  };
  unsigned prefix = 0;                         // the bytes of the median found so far
  int rank = 0, c = 0;
  for (int pass = 0; pass < 4; pass++) {
    const int shift = 24 - 8 * pass;
    s_hist[tid] = 0;
    __syncthreads();
    for (int r = tid; r < np; r += PG_THREADS) {
      unsigned u;
      if (pass == 0) {
        u = sample(r);
        if (r < PG_STAGE) s_bits[r] = u;
      } else {
        u = r < PG_STAGE ? s_bits[r] : sample(r);
      }
      if (u != 0u && (pass == 0 || (u >> (shift + 8)) == prefix)) atomicAdd(&s_hist[(u >> shift) & 255u], 1);
    }
    __syncthreads();
    const int mine = s_hist[tid];
    int incl = mine;                           // inclusive scan of the 256 bins: within the wavefront, then across
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(incl, off, 64);
      if ((tid & 63) >= off) incl += up;
    }
    if ((tid & 63) == 63) s_wsum[tid >> 6] = incl;
    __syncthreads();
    int total = 0;
    for (int w = 0; w < PG_THREADS / 64; w++) {
      if (w < (tid >> 6)) incl += s_wsum[w];
      total += s_wsum[w];
    }
    if (pass == 0) {
      c = total;
      rank = (c - 1) >> 1;
    }
    if (c < A.min_common) break;               // the same c in every thread; min_common >= 1 covers c == 0
    if (incl - mine <= rank && rank < incl) {  // one bin holds the rank
      s_bin = tid;
      s_below = incl - mine;
    }
    __syncthreads();
    prefix = (prefix << 8) | (unsigned)s_bin;
    rank -= s_below;
  }
  if (tid == 0) {
    float rho = 0.0f;
    if (c >= A.min_common) __builtin_memcpy(&rho, &prefix, sizeof rho);
    A.link_ratio[l] = rho;
    A.link_common[l] = c;
  }
}

// lane 0's part of the second kernel on lists laid out as the temp memory is; inlined once per address space
__device__ __forceinline__ void posegraph_solve_lists(const PgArgs &A, const int *lists, const float *ratio, float *scale,
                                                      float *cam, int *cam_pair, int *counts)
{
  const int *links = lists, *pairs = links + 3 * (size_t)A.nlinks, *walk = pairs + 2 * (size_t)A.npairs;
  const int *usable = walk + A.nwalk;
  posegraph_solve(A.npairs, pairs, usable, A.pose, A.nlinks, links, ratio, A.seed_pair, A.root_image, A.nwalk, walk,
                  scale, cam, cam_pair, counts);
}

__global__ __launch_bounds__(64) void posegraph_solve_kernel(PgArgs A)
{
  __shared__ int s_words[PG_SERIAL_WORDS];
  __shared__ int s_counts[2];
  const int lane = threadIdx.x;
  const long long nlist = 3LL * A.nlinks + 3LL * A.npairs + A.nwalk;
  if (nlist + A.nlinks + A.npairs + 13LL * A.nimages <= PG_SERIAL_WORDS) {
    // lists | ratios | scales | cameras | cam_pair, all in LDS; the two calls below differ in nothing but where the
    // pointers lead, and are kept apart so that this one compiles to LDS instructions and not to flat ones
    float *s_ratio = reinterpret_cast<float *>(s_words + nlist), *s_scale = s_ratio + A.nlinks;
    float *s_cam = s_scale + A.npairs;
    int *s_cam_pair = reinterpret_cast<int *>(s_cam + 12 * A.nimages);
    for (int i = lane; i < (int)nlist; i += 64) s_words[i] = A.tmp[i];
    for (int i = lane; i < A.nlinks; i += 64) s_ratio[i] = A.link_ratio[i];
    for (int i = lane; i < A.npairs; i += 64) s_scale[i] = A.pair_scale[i];
    for (int i = lane; i < 12 * A.nimages; i += 64) s_cam[i] = A.cam[i];
    for (int i = lane; i < A.nimages; i += 64) s_cam_pair[i] = A.cam_pair[i];
    __syncthreads();
    if (lane == 0) posegraph_solve_lists(A, s_words, s_ratio, s_scale, s_cam, s_cam_pair, s_counts);
    __syncthreads();
    for (int i = lane; i < A.npairs; i += 64) A.pair_scale[i] = s_scale[i];
    for (int i = lane; i < 12 * A.nimages; i += 64) A.cam[i] = s_cam[i];
    for (int i = lane; i < A.nimages; i += 64) A.cam_pair[i] = s_cam_pair[i];
  } else {
    if (lane == 0) posegraph_solve_lists(A, A.tmp, A.link_ratio, A.pair_scale, A.cam, A.cam_pair, s_counts);
    __syncthreads();
  }
  int enough = 0, least = 0x7fffffff;
  for (int l = lane; l < A.nlinks; l += 64) {
    const int c = A.link_common[l];
    if (c >= A.min_common) {
      enough++;
      least = min(least, c);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    enough += __shfl_xor(enough, off, 64);
    least = min(least, __shfl_xor(least, off, 64));
  }
  if (lane < 8) {
    const int v[8] = {enough, s_counts[0], s_counts[1], enough ? least : 0, 0, 0, 0, 0};
    int out = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) out = lane == j ? v[j] : out;
    A.summary[lane] = out;
  }
}

}  // namespace

size_t link_poses_batch_tmp_bytes(int npairs, int nlinks, int nwalk)
{
  return sizeof(int) * (3 * (size_t)nlinks + 3 * (size_t)npairs + (size_t)nwalk + 4);
}

// Enqueue misift_link_poses_batch on the context stream (common.hpp): two launches.  h_lists: links, pairs, walk.
int launch_link_poses_batch(misift_ctx *ctx, int npairs, int nimages, int nlinks, int nwalk, const int *h_lists,
                            const void *d_rows, const int *d_row_counts, int max_pts, float min_score,
                            float max_ambiguity, float max_error, const float *d_pose, const int *d_num_front,
                            const float *d_xyz, int seed_pair, int root_image, int min_common, float *d_link_ratio,
                            int *d_link_common, float *d_pair_scale, float *d_cam, int *d_cam_pair, int *d_summary)
{
  int rc = misift_ensure_tmp(ctx, link_poses_batch_tmp_bytes(npairs, nlinks, nwalk));
  if (rc) return rc;
  PgArgs A;
  A.h_links = h_lists; A.h_pairs = h_lists + 3 * (size_t)nlinks; A.h_walk = A.h_pairs + 2 * (size_t)npairs;
  A.npairs = npairs; A.nlinks = nlinks; A.nwalk = nwalk; A.nimages = nimages; A.max_pts = max_pts;
  A.min_common = min_common; A.seed_pair = seed_pair; A.root_image = root_image;
  A.rows = (const SiftPointD *)d_rows; A.row_counts = d_row_counts;
  A.pose = d_pose; A.num_front = d_num_front; A.xyz = d_xyz;
  A.min_score = min_score; A.max_ambiguity = max_ambiguity; A.max_error = max_error;
  A.use_error = max_error < __builtin_huge_valf();                // +inf: match_error is not read
  A.tmp = reinterpret_cast<int *>(ctx->d_match_tmp);
  A.link_ratio = d_link_ratio; A.link_common = d_link_common; A.pair_scale = d_pair_scale; A.cam = d_cam;
  A.cam_pair = d_cam_pair; A.summary = d_summary;
  {
    LaunchScope ls(ctx, "posegraph_ratio");
    hipLaunchKernelGGL(posegraph_ratio_kernel, dim3(nlinks + 1), dim3(PG_THREADS), 0, ctx->stream, A);
    rc = ls.finish();
    if (rc) return rc;
  }
  LaunchScope ls(ctx, "posegraph_solve");
  hipLaunchKernelGGL(posegraph_solve_kernel, dim3(1), dim3(64), 0, ctx->stream, A);
  return ls.finish();
}

// Test-only, host-only: step 1 for one link and step 2 for a whole graph, as the kernels compute them
// (posegraph_core.hpp).  The median is taken from a sorted copy: any exact selection gives the same sample.
extern "C" int misift_test_posegraph_capacity(int which) { return which == 0 ? PG_STAGE : PG_SERIAL_WORDS; }

extern "C" int misift_test_posegraph_ratio(const void *rows_p, const float *xyz_p, int count_p, const void *rows_q,
                                           const float *xyz_q, int count_q, int max_pts, int kind, float min_score,
                                           float max_ambiguity, float max_error, int min_common, float *ratio,
                                           int *common)
{
  if (!rows_p || !xyz_p || !rows_q || !xyz_q || max_pts < 1 || (kind != POSEGRAPH_CHAIN && kind != POSEGRAPH_FAN) ||
      min_common < 1 || !ratio || !common) {
    misift_set_error("misift_test_posegraph_ratio: invalid argument");
    return MISIFT_EINVAL;
  }
  const int np = posegraph_rows(count_p, max_pts), nq = posegraph_rows(count_q, max_pts);
  const bool use_error = max_error < __builtin_huge_valf();
  std::vector<unsigned> bits;
  for (int r = 0; r < np; r++) {
    const unsigned u = posegraph_sample((const SiftPointD *)rows_p, xyz_p, (const SiftPointD *)rows_q, xyz_q, nq, kind,
                                        r, min_score, max_ambiguity, use_error, max_error);
    if (u) bits.push_back(u);
  }
  std::sort(bits.begin(), bits.end());
  const int c = (int)bits.size();
  *common = c;
  *ratio = 0.0f;
  if (c >= min_common) __builtin_memcpy(ratio, &bits[(size_t)((c - 1) >> 1)], sizeof(float));
  return MISIFT_OK;
}

extern "C" int misift_test_posegraph_compose(int npairs, const int *pairs, int nimages, const float *pose,
                                             const int *num_front, int nlinks, const int *links, const float *ratio,
                                             int seed_pair, int root_image, int nwalk, const int *walk, float *pair_scale,
                                             float *cam, int *cam_pair, int *counts2)
{
  bool ok = npairs >= 0 && nimages >= 1 && nlinks >= 0 && nwalk >= 0 && root_image >= 0 && root_image < nimages &&
            pair_scale && cam && cam_pair && counts2 && (npairs == 0 || (pairs && pose && num_front)) &&
            (nlinks == 0 || (links && ratio)) && (nwalk == 0 || walk) &&
            (npairs == 0 || (seed_pair >= 0 && seed_pair < npairs));
  for (int p = 0; ok && p < 2 * npairs; p++) ok = pairs[p] >= 0 && pairs[p] < nimages;
  for (int l = 0; ok && l < nlinks; l++)
    ok = links[3 * l] >= 0 && links[3 * l] < npairs && links[3 * l + 1] >= 0 && links[3 * l + 1] < npairs;
  for (int w = 0; ok && w < nwalk; w++) ok = walk[w] >= 0 && walk[w] < npairs;
  if (!ok) {
    misift_set_error("misift_test_posegraph_compose: invalid argument");
    return MISIFT_EINVAL;
  }
  std::vector<int> usable((size_t)npairs + 1, 0);
  for (int p = 0; p < npairs; p++) {
    usable[p] = posegraph_usable(pose + 12 * (size_t)p, num_front[p]) ? 1 : 0;
    pair_scale[p] = 0.0f;
  }
  for (int i = 0; i < 12 * nimages; i++) cam[i] = 0.0f;
  for (int i = 0; i < nimages; i++) cam_pair[i] = POSEGRAPH_UNSET;
  posegraph_solve(npairs, pairs, usable.data(), pose, nlinks, links, ratio, seed_pair, root_image, nwalk, walk,
                  pair_scale, cam, cam_pair, counts2);
  return MISIFT_OK;
}

// ransac_batch.hpp — the batch RANSAC search that misift_find_homography_batch (homography.hip) and
// misift_find_fundamental_batch (kernels_fundamental.hip) share.  Entry e works on frame frames[e] of a device-resident
// record batch (counts and offsets read on the device) and writes result slot e; no host round trip.  Four launches
// whatever the number of entries:
//   gather  one 1024-thread workgroup per entry: SoA coordinates and the ORDERED list of the valid records into the
//           entry's temp (ransac_gather), then wave 0 draws the entry's sample positions from libc rand() restated on the
//           device (libc_rand.hpp), seeded with seeds[e], one hypothesis after another.  Entries with fewer than 8 records,
//           fewer than 8 valid records, or more than max_pts records are marked done here.
//   solve   the model's own kernel, one lane per (entry, hypothesis): sample positions -> parameters; it also zeroes the
//           entry's counts.
//   count   the hot path: one 64-lane workgroup per (entry, 64 hypotheses, 512-point chunk).  The chunk's coordinates are
//           staged once in LDS and read by broadcast; each lane holds one hypothesis in registers and tests every point of
//           the chunk, then adds its count atomically (an integer sum: the order of the chunks does not matter).
//   pick    one 1024-thread workgroup per entry: the largest count at the smallest hypothesis index (ransac_pick) -> the
//           entry's nine floats and its count; the model's done result for the entries the gather marked done.
//
// A model is a struct of constants and __forceinline__ statics, all resolved at compile time:
//   SAMPLE, PARAMS        positions drawn and floats solved per hypothesis
//   COUNT_ALL             the count runs over all records of the frame (true) or over the valid list (false)
//   draw(g, fm, p)        one hypothesis' SAMPLE distinct positions from the entry's rand() stream
//   inlier(h, x1, y1, x2, y2, thresh2)  the inlier test of hypothesis h on one stored match
//   done(k)               float k of the nine a done entry gets
//   picked(out)           completes the nine floats of a picked entry behind its PARAMS parameters
//
// What differs between the two searches, and is meant to (each difference is pinned by tests):
//   what is counted   the homography counts inliers over ALL n records of the frame, invalid ones included (the reference's
//                     TestHomographies); the fundamental counts over the valid list only, each index range-checked.
//   how many run      the homography draws, solves, counts and picks over num_loops rounded up to 16, as the single call
//                     does; the fundamental over exactly num_loops, lp being only a stride.  This is what each wrapper
//                     puts into RansacArgs::num_loops and ::lp, not a switch.
//   done entries      the homography writes the identity and 0 (-1 over max_pts); the fundamental nine zeros and 0 / -1.
//   picked result     a picked homography gets H[8] = 1; a picked F is its nine parameters.
//   solve             a scratch-resident 8x8 LU per lane for the homography; a lane's 8x9 system in LDS, behind a range
//                     check of the positions and record indices it read, for the fundamental.
#pragma once
#include "common.hpp"
#include "libc_rand.hpp"

// what the searches read of a record, in floats
constexpr int OFF_XPOS = 0, OFF_YPOS = 1, OFF_SCORE = 6, OFF_AMBIG = 7, OFF_MXPOS = 9, OFF_MYPOS = 10;
constexpr int PT_WORDS = (int)(sizeof(SiftPointD) / sizeof(float));

constexpr int RANSAC_CHUNK = 512;              // points per count workgroup (8 KiB of LDS)
constexpr int RANSAC_META = 4;                 // ints of meta per entry

struct RansacArgs {
  BatchLayout set;
  const int *frames;                           // pinned host copies of the caller's lists
  const unsigned *seeds;
  int max_pts, mp16;                           // mp16 = max_pts rounded up to 16
  int num_loops, lp;                           // hypotheses drawn, solved, counted and picked over; their stride
  float min_score, max_ambiguity, thresh2;
  // temp, per entry e:
  //   coord[4 x mp16] | valid[mp16] | sample[SAMPLE x lp] | hyp[PARAMS x lp] | hcount[lp] | meta[RANSAC_META]
  float *coord;
  int *valid, *sample;
  float *hyp;
  int *hcount;
  int *meta;                                   // [0] points to count (0: entry done), [1] a done entry's result,
                                               // [2] records of the frame
  float *out;                                  // out: nsel x 9
  int *num;                                    // out: nsel
};

// One 1024-thread workgroup: SoA coordinates coord[k * stride + i] of the npts records at pts, and the ORDERED list of the
// valid ones (ballot/popcount compaction keeps index order, which the rand() % numValid sampling depends on).  Returns the
// number of valid records to every thread.
__device__ __forceinline__ int ransac_gather(const float *pts, int npts, int stride, float min_score, float max_ambiguity,
                                             float *coord, int *valid)
{
  __shared__ int wave_cnt[16];
  __shared__ int base_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int i0 = 0; i0 < npts; i0 += 1024) {
    const int i = i0 + tid;
    bool ok = false;
    if (i < npts) {
      const float *p = pts + (size_t)i * PT_WORDS;
      coord[0 * stride + i] = p[OFF_XPOS];
      coord[1 * stride + i] = p[OFF_YPOS];
      coord[2 * stride + i] = p[OFF_MXPOS];
      coord[3 * stride + i] = p[OFF_MYPOS];
      ok = p[OFF_SCORE] > min_score && p[OFF_AMBIG] < max_ambiguity;      // matching.cu:1035
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = base_s;
    for (int w = 0; w < wave; w++) off += wave_cnt[w];
    if (ok) valid[off + __popcll(m & ((1ull << lane) - 1ull))] = i;
    __syncthreads();
    if (tid == 0) {
      int s = 0;
      for (int w = 0; w < 16; w++) s += wave_cnt[w];
      base_s += s;
    }
    __syncthreads();
  }
  return base_s;
}

// One 1024-thread workgroup: the first hypothesis with the largest count (strict '>' scan of matching.cu:1063-1068).
// Returns, in thread 0, the max key: the count in the high word, (INT_MAX - index) in the low word.
__device__ __forceinline__ unsigned long long ransac_pick(const int *counts, int num_loops)
{
  __shared__ unsigned long long best_s[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long best = 0;
  for (int i = tid; i < num_loops; i += 1024) {
    const unsigned long long key = ((unsigned long long)(unsigned)counts[i] << 32) | (unsigned)(0x7fffffff - i);
    best = key > best ? key : best;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(best, off, 64);
    best = o > best ? o : best;
  }
  if (lane == 0) best_s[wave] = best;
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < 16; w++) best = best_s[w] > best ? best_s[w] : best;
  return best;
}
__device__ __forceinline__ int ransac_pick_index(unsigned long long key)
{
  return 0x7fffffff - (int)(unsigned)(key & 0xffffffffull);
}
__device__ __forceinline__ int ransac_pick_count(unsigned long long key) { return (int)(key >> 32); }

template <class Model>
__global__ __launch_bounds__(1024) void ransac_gather_kernel(RansacArgs G)
{
  const int e = blockIdx.x;
  const int f = G.frames[e];
  const int n = G.set.counts[f];
  int *meta = G.meta + (size_t)RANSAC_META * e;
  if (n < 8 || n > G.max_pts) {                // matching.cu:1016-1017 (count -1 included); over max_pts: -1, nothing read
    if (threadIdx.x == 0) { meta[0] = 0; meta[1] = n > G.max_pts ? -1 : 0; meta[2] = 0; }
    return;
  }
  const float *pts = reinterpret_cast<const float *>(G.set.recs + G.set.base(f));
  const int num_valid = ransac_gather(pts, n, G.mp16, G.min_score, G.max_ambiguity, G.coord + (size_t)e * 4 * G.mp16,
                                      G.valid + (size_t)e * G.mp16);
  const int tid = threadIdx.x;
  if (num_valid < 8) {
    if (tid == 0) { meta[0] = 0; meta[1] = 0; meta[2] = 0; }
    return;
  }
  if (tid < 64) {                              // wave 0: the entry's rand() stream, hypotheses one after another
    const int L = G.num_loops, lp = G.lp;
    int *sample = G.sample + (size_t)e * Model::SAMPLE * lp;
    LibcRand<LibcRandWaveRing> g;
    g.seed(G.seeds[e]);
    const FastMod31 fm((uint32_t)num_valid);
    for (int loop = 0; loop < L; loop++) {
      int p[Model::SAMPLE];
      Model::draw(g, fm, p);
      if (tid == 0)
        for (int k = 0; k < Model::SAMPLE; k++) sample[k * lp + loop] = p[k];
    }
    if (tid == 0) { meta[0] = Model::COUNT_ALL ? n : num_valid; meta[1] = 0; meta[2] = n; }
  }
}

template <class Model>
__global__ __launch_bounds__(64) void ransac_count_kernel(RansacArgs G, int hblocks, int chunks)
{
  __shared__ float4 s_pt[RANSAC_CHUNK];
  const int c = blockIdx.x % chunks, eh = blockIdx.x / chunks;
  const int e = eh / hblocks, hb = eh % hblocks;
  const int *meta = G.meta + (size_t)RANSAC_META * e;
  const int total = min(meta[0], G.mp16), npts = meta[2];
  const int i0 = c * RANSAC_CHUNK;
  if (i0 >= total) return;                     // beyond the points to count, or an entry already done (0)
  const int n = min(RANSAC_CHUNK, total - i0);
  const int lp = G.lp, mp = G.mp16;
  const float *coord = G.coord + (size_t)e * 4 * mp + (Model::COUNT_ALL ? i0 : 0);
  const int *valid = G.valid + (size_t)e * mp + i0;
  for (int i = threadIdx.x; i < n; i += 64) {
    int j = i;                                 // the chunk's i-th record, or the one its i-th valid position names
    if (!Model::COUNT_ALL) {                   // a record index from device memory: checked before use
      const int pt = valid[i];
      j = (unsigned)pt < (unsigned)npts ? pt : 0;
    }
    s_pt[i] = make_float4(coord[j], coord[mp + j], coord[2 * mp + j], coord[3 * mp + j]);
  }
  __syncthreads();
  const int h = hb * 64 + threadIdx.x;
  if (h >= G.num_loops) return;
  const float *hyp = G.hyp + (size_t)e * Model::PARAMS * lp;
  float a[Model::PARAMS];
#pragma unroll
  for (int k = 0; k < Model::PARAMS; k++) a[k] = hyp[k * lp + h];
  const float thresh2 = G.thresh2;
  int cnt = 0;
  for (int i = 0; i < n; i++) {
    const float4 q = s_pt[i];
    cnt += Model::inlier(a, q.x, q.y, q.z, q.w, thresh2) ? 1 : 0;
  }
  atomicAdd(&G.hcount[(size_t)e * lp + h], cnt);
}

template <class Model>
__global__ __launch_bounds__(1024) void ransac_pick_kernel(RansacArgs G)
{
  const int e = blockIdx.x;
  float *out = G.out + (size_t)9 * e;
  const int *meta = G.meta + (size_t)RANSAC_META * e;
  if (meta[0] == 0) {                          // the model's done result and 0, or -1 for a frame over max_pts
    if (threadIdx.x < 9) out[threadIdx.x] = Model::done(threadIdx.x);
    if (threadIdx.x == 0) G.num[e] = meta[1];
    return;
  }
  const unsigned long long best = ransac_pick(G.hcount + (size_t)e * G.lp, G.num_loops);
  if (threadIdx.x == 0) {
    const int idx = ransac_pick_index(best);
    const float *hyp = G.hyp + (size_t)e * Model::PARAMS * G.lp;
    for (int k = 0; k < Model::PARAMS; k++) out[k] = hyp[k * G.lp + idx];
    Model::picked(out);
    G.num[e] = ransac_pick_count(best);
  }
}

// The entry point's name (for its errors) and the LaunchScope slots of its four launches.
struct RansacNames {
  const char *who, *gather, *solve, *count, *pick;
};

inline int ransac_round16(int v) { return (int)(((size_t)v + 15) / 16 * 16); }

// The host side of a search: everything of RansacArgs but the temp.  num_loops is the number of hypotheses the search
// works over: the caller's, or the caller's rounded up to 16, as the wrapper decides.
inline RansacArgs ransac_args(const int *h_frames, const unsigned *h_seeds, const BatchLayout &set, int max_pts,
                              int num_loops, float min_score, float max_ambiguity, float thresh, float *out, int *num)
{
  RansacArgs G{};
  G.set = set;
  G.frames = h_frames; G.seeds = h_seeds;
  G.max_pts = max_pts;
  G.mp16 = ransac_round16(max_pts);
  G.num_loops = num_loops;
  G.lp = ransac_round16(num_loops);
  G.min_score = min_score; G.max_ambiguity = max_ambiguity; G.thresh2 = thresh * thresh;
  G.out = out; G.num = num;
  return G;
}

// Sizes and carves the temp (misift_ensure_tmp), then the four launches on the context stream; solve(G, hblocks) enqueues
// the model's solve kernel on nsel * hblocks 64-lane workgroups.
template <class Model, class Solve>
int ransac_batch_run(misift_ctx *ctx, const RansacNames &names, int nsel, RansacArgs G, Solve solve)
{
  const size_t mp = (size_t)G.mp16, lp = (size_t)G.lp, ns = (size_t)nsel;
  const int hblocks = (G.num_loops + 63) / 64, chunks = (int)((mp + RANSAC_CHUNK - 1) / RANSAC_CHUNK);
  if ((long long)nsel * hblocks * chunks > 0x7fffffffLL) {
    misift_set_error("%s: %d entries x %d loops x %d points is beyond one launch", names.who, nsel, G.num_loops,
                     G.max_pts);
    return MISIFT_EINVAL;
  }
  const size_t words = 5 * mp + (Model::SAMPLE + Model::PARAMS + 1) * lp + RANSAC_META;
  int rc = misift_ensure_tmp(ctx, ns * words * sizeof(float));
  if (rc) return rc;
  G.coord = reinterpret_cast<float *>(ctx->d_match_tmp);
  G.valid = reinterpret_cast<int *>(G.coord + ns * 4 * mp);
  G.sample = G.valid + ns * mp;
  G.hyp = reinterpret_cast<float *>(G.sample + ns * Model::SAMPLE * lp);
  G.hcount = reinterpret_cast<int *>(G.hyp + ns * Model::PARAMS * lp);
  G.meta = G.hcount + ns * lp;
  {
    LaunchScope ls(ctx, names.gather);
    hipLaunchKernelGGL(ransac_gather_kernel<Model>, dim3(nsel), dim3(1024), 0, ctx->stream, G);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, names.solve);
    solve(G, hblocks);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, names.count);
    hipLaunchKernelGGL(ransac_count_kernel<Model>, dim3(nsel * hblocks * chunks), dim3(64), 0, ctx->stream, G, hblocks,
                       chunks);
    rc = ls.finish();
    if (rc) return rc;
  }
  LaunchScope ls(ctx, names.pick);
  hipLaunchKernelGGL(ransac_pick_kernel<Model>, dim3(nsel), dim3(1024), 0, ctx->stream, G);
  return ls.finish();
}

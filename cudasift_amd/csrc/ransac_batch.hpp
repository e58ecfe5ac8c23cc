// ransac_batch.hpp — the batch RANSAC search that misift_find_homography_batch (homography.hip),
// misift_find_fundamental_batch (kernels_fundamental.hip), misift_resect_cameras_batch (kernels_resect.hip),
// misift_align_points_batch (kernels_align.hip) and misift_localize_frames_batch (kernels_localize.hip: resect's model
// over its own candidates, resect_model.hpp) share.  Entry e gathers its candidates on the device and writes result
// slot e; no host round trip.  Four launches whatever the number of entries (ransac_launches):
//   gather  one 1024-thread workgroup per entry: SoA coordinates of the entry's candidates into its temp, in ORDER
//           (RansacCompaction: a sample position p means "the p-th candidate"), then wave 0 draws the entry's sample
//           positions from libc rand() restated on the device (ransac_draw, libc_rand.hpp), seeded with seeds[e], one
//           hypothesis after another.  Entries with nothing to search are marked done here (meta[0] = 0).
//   solve   the model's own kernel, one lane per (entry, hypothesis): sample positions -> parameters, between
//           ransac_solve_begin (which also zeroes the entry's counts), ransac_sample_position and ransac_store_hyp.
//   count   the hot path, ransac_count_kernel: one 64-lane workgroup per (entry, 64 hypotheses, 512-candidate chunk).
//           The chunk's coordinates are staged once in LDS and read by broadcast; each lane holds one hypothesis in
//           registers and tests every candidate of the chunk, then adds its count atomically (an integer sum: the order
//           of the chunks does not matter).
//   pick    one 1024-thread workgroup per entry: the largest count at the smallest hypothesis index (ransac_pick).
// The temp of every search is laid out by ransac_temp, pooled array by array over the entries:
//   prefix | coord[COORDS x cap16] | index[cap16] if INDEX | sample[SAMPLE x lp] | hyp[PARAMS x lp] | hcount[lp] |
//   meta[RANSAC_META] | tail
//
// A model is a struct of constants and __forceinline__ statics, all resolved at compile time:
//   Args                  the kernels' argument struct; its member rs is the RansacSearch
//   SAMPLE, PARAMS        positions drawn and floats solved per hypothesis
//   COORDS                floats per candidate: 4, 5 or 6 (a float4 in LDS, plus nothing, a float or a float2)
//   INDEX                 an index per candidate follows coord in the temp
//   COUNT_ALL             the count runs over everything coord holds (true) or over the index list (false)
//   draw(g, fm, p)        one hypothesis' SAMPLE distinct positions from the entry's rand() stream
//   lane(A, e)            what a lane holds beside its hypothesis while it counts (Lane; RansacPlainLane: nothing)
//   inlier(h, lane, q, thresh2)  the inlier test of hypothesis h on one candidate's COORDS values
//   invalid()             what a hypothesis from an out-of-range sample is made of
// and, for the two searches on frames of stored matches, which also share their gather and pick kernels:
//   done(k)               float k of the nine a done entry gets
//   picked(out)           completes the nine floats of a picked entry behind its PARAMS parameters
//
// What differs between the searches, and is meant to (each difference is pinned by tests):
//   the candidates    the records of a frame with (x, y, match x, match y), gated by score and ambiguity (homography,
//                     fundamental); the observations an image makes of triangulated points, (x, y, X, Y, Z) (resect:
//                     its own gather, which goes on counting past max_cand without storing); the mapped point pairs of
//                     two scenes, (a, b) (align: its own gather, which also marks d_inlier and keeps each index); the rows
//                     of a frame matched against a scene's points, (x, y, X, Y, Z) with the row index kept (localise).
//   what is counted   the homography counts inliers over ALL n records of the frame, invalid ones included (the reference's
//                     TestHomographies); the fundamental counts over the valid list only, each index range-checked;
//                     resect and align store only candidates, and count them all.
//   how many run      the homography draws, solves, counts and picks over num_loops rounded up to 16, as the single call
//                     does; the others over exactly num_loops, lp being only a stride.  This is what each launcher puts
//                     into RansacSearch::num_loops, not a switch.
//   done entries      the homography writes the identity and 0 (-1 over max_pts); the fundamental nine zeros and 0 / -1;
//                     resect and align a status of their own (meta[1]) from their own pick / refit kernels.
//   picked result     a picked homography gets H[8] = 1; a picked F is its nine parameters; resect installs the camera
//                     and sums up; align hands the picked transform to its refit launch (the tail of its temp).
//   solve             a scratch-resident 8x8 LU per lane for the homography, written out in its kernel (the
//                     HOMO_CORE_SOLVE fragment); a lane's system in LDS for the fundamental (8x9) and resect (11x12);
//                     registers for align.
//   per lane          resect's count holds the image's four intrinsics beside the camera.
#pragma once
#include "common.hpp"
#include "libc_rand.hpp"

// what the searches read of a record, in floats
constexpr int OFF_XPOS = 0, OFF_YPOS = 1, OFF_SCORE = 6, OFF_AMBIG = 7, OFF_MXPOS = 9, OFF_MYPOS = 10;
constexpr int PT_WORDS = (int)(sizeof(SiftPointD) / sizeof(float));

constexpr int RANSAC_CHUNK = 512;              // candidates per count workgroup (8 to 12 KiB of LDS)
constexpr int RANSAC_META = 4;                 // ints of meta per entry

// What every search has.
struct RansacSearch {
  int nsel, cap16;                             // entries; the candidates an entry has room for, rounded up to 16
  int num_loops, lp;                           // hypotheses drawn, solved, counted and picked over; their stride
  float thresh2;
  const unsigned *seeds;                       // pinned host copy: nsel
  float *coord;                                // temp (ransac_temp)
  int *index, *sample;
  float *hyp;
  int *hcount;
  int *meta;                                   // [0] candidates to count (0: entry done), [1..3] the model's
};

struct RansacArgs {                            // the two searches on frames of stored matches
  RansacSearch rs;                             // index: the valid records; meta[1] a done entry's result, [2] records
  BatchLayout set;
  const int *frames;                           // pinned host copy of the caller's list
  int max_pts;
  float min_score, max_ambiguity;
  float *out;                                  // out: nsel x 9
  int *num;                                    // out: nsel
};

// Ordered compaction over the rounds of a 1024-thread workgroup: in every round each thread hands in a flag and gets
// the position its candidate takes among all flagged so far, in thread order (ballot / popcount within a wavefront, a
// prefix over the earlier wavefronts).  Every thread of the workgroup calls place() and next() in every round.
struct RansacCompaction {
  int *wave_cnt, *base;                        // LDS: 16 ints, 1 int
  __device__ __forceinline__ int place(bool ok) const
  {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(ok);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = *base;
    for (int w = 0; w < wave; w++) off += wave_cnt[w];
    return off + __popcll(m & ((1ull << lane) - 1ull));
  }
  __device__ __forceinline__ void next() const
  {
    __syncthreads();
    if (threadIdx.x == 0) {
      int s = 0;
      for (int w = 0; w < 16; w++) s += wave_cnt[w];
      *base += s;
    }
    __syncthreads();
  }
  __device__ __forceinline__ int total() const { return *base; }            // behind next(): all flagged so far
};
__device__ __forceinline__ RansacCompaction ransac_compaction()
{
  __shared__ int wave_cnt[16];
  __shared__ int base_s;
  if (threadIdx.x == 0) base_s = 0;
  __syncthreads();
  return RansacCompaction{wave_cnt, &base_s};
}

// One 1024-thread workgroup: SoA coordinates coord[k * stride + i] of the npts records at pts, and the ORDERED list of the
// valid ones (the rand() % numValid sampling depends on index order).  Returns the number of valid records to every
// thread.
__device__ __forceinline__ int ransac_gather(const float *pts, int npts, int stride, float min_score, float max_ambiguity,
                                             float *coord, int *valid)
{
  const RansacCompaction c = ransac_compaction();
  for (int i0 = 0; i0 < npts; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    bool ok = false;
    if (i < npts) {
      const float *p = pts + (size_t)i * PT_WORDS;
      coord[0 * stride + i] = p[OFF_XPOS];
      coord[1 * stride + i] = p[OFF_YPOS];
      coord[2 * stride + i] = p[OFF_MXPOS];
      coord[3 * stride + i] = p[OFF_MYPOS];
      ok = p[OFF_SCORE] > min_score && p[OFF_AMBIG] < max_ambiguity;      // matching.cu:1035
    }
    const int pos = c.place(ok);
    if (ok) valid[pos] = i;
    c.next();
  }
  return c.total();
}

// Wave 0 of a gather workgroup: the entry's rand() stream over n candidates, hypotheses one after another, into
// sample[k * lp + loop].
template <class Model>
__device__ __forceinline__ void ransac_draw(unsigned seed, int n, int *sample, int L, int lp)
{
  LibcRand<LibcRandWaveRing> g;
  g.seed(seed);
  const FastMod31 fm((uint32_t)n);
  for (int loop = 0; loop < L; loop++) {
    int p[Model::SAMPLE];
    Model::draw(g, fm, p);
    if (threadIdx.x == 0)
      for (int k = 0; k < Model::SAMPLE; k++) sample[k * lp + loop] = p[k];
  }
}

// The same draws on the host, hypothesis after hypothesis into out[SAMPLE * loop + k]: behind the misift_test_*_samples
// hooks.  draw is the model's draw function over LibcRandArrayRing.
template <int SAMPLE>
void ransac_host_samples(unsigned seed, int n, int num_loops, int *out,
                         void (*draw)(LibcRand<LibcRandArrayRing> &, const FastMod31 &, int (&)[SAMPLE]))
{
  LibcRand<LibcRandArrayRing> g;
  g.seed(seed);
  const FastMod31 fm((uint32_t)n);
  for (int loop = 0; loop < num_loops; loop++) {
    int p[SAMPLE];
    draw(g, fm, p);
    for (int k = 0; k < SAMPLE; k++) out[SAMPLE * loop + k] = p[k];
  }
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

// A solve kernel's prologue, 64-lane workgroups on a grid of nsel * hblocks: the lane's entry e and hypothesis idx and
// the entry's candidates n.  False for a done entry or a lane beyond num_loops; otherwise the hypothesis' count is zeroed.
__device__ __forceinline__ bool ransac_solve_begin(const RansacSearch &S, int hblocks, int &e, int &idx, int &n)
{
  e = blockIdx.x / hblocks;
  idx = (blockIdx.x % hblocks) * 64 + threadIdx.x;
  n = min(S.meta[(size_t)RANSAC_META * e], S.cap16);
  if (n <= 0 || idx >= S.num_loops) return false;
  S.hcount[(size_t)e * S.lp + idx] = 0;
  return true;
}

// Position k of hypothesis idx of entry e.  Positions come from device memory and are checked before use: one that is
// not in [0, n) reads as 0 and clears in_range.
template <class Model>
__device__ __forceinline__ int ransac_sample_position(const RansacSearch &S, int e, int idx, int k, int n, bool &in_range)
{
  const int pos = S.sample[((size_t)e * Model::SAMPLE + k) * S.lp + idx];
  const bool pos_ok = (unsigned)pos < (unsigned)n;
  in_range = in_range && pos_ok;
  return pos_ok ? pos : 0;
}

// A solve kernel's epilogue: the hypothesis, or the model's invalid one where a position was out of range.
template <class Model>
__device__ __forceinline__ void ransac_store_hyp(const RansacSearch &S, int e, int idx, bool in_range,
                                                 const float (&h)[Model::PARAMS])
{
  float *hyp = S.hyp + (size_t)e * Model::PARAMS * S.lp;
#pragma unroll
  for (int k = 0; k < Model::PARAMS; k++) hyp[k * S.lp + idx] = in_range ? h[k] : Model::invalid();
}

// for the models whose lanes hold nothing but their hypothesis while they count
struct RansacPlainLane {
  struct Lane {};
  template <class Args>
  static __device__ __forceinline__ Lane lane(const Args &, int) { return Lane{}; }
};

// how a candidate's coordinates beyond four sit in LDS
template <int COORDS> struct RansacRest { typedef float type; };             // 5: a float; 4: nothing (never referenced)
template <> struct RansacRest<6> { typedef float2 type; };

template <class Model>
__global__ __launch_bounds__(64) void ransac_count_kernel(typename Model::Args A, int hblocks, int chunks)
{
  constexpr int C = Model::COORDS;
  static_assert(C >= 4 && C <= 6, "a float4 and nothing, a float or a float2");
  __shared__ float4 s_pt[RANSAC_CHUNK];
  __shared__ typename RansacRest<C>::type s_rest[RANSAC_CHUNK];
  const RansacSearch &S = A.rs;
  const int c = blockIdx.x % chunks, eh = blockIdx.x / chunks;
  const int e = eh / hblocks, hb = eh % hblocks;
  const int *meta = S.meta + (size_t)RANSAC_META * e;
  const int total = min(meta[0], S.cap16), npts = meta[2];
  const int i0 = c * RANSAC_CHUNK;
  if (i0 >= total) return;                     // beyond the candidates to count, or an entry already done (0)
  const int n = min(RANSAC_CHUNK, total - i0);
  const int lp = S.lp, mp = S.cap16;
  const float *coord = S.coord + (size_t)e * C * mp + (Model::COUNT_ALL ? i0 : 0);
  for (int i = threadIdx.x; i < n; i += 64) {
    int j = i;                                 // the chunk's i-th candidate, or the one its i-th index names
    if constexpr (!Model::COUNT_ALL) {         // a record index from device memory: checked before use
      const int pt = S.index[(size_t)e * mp + i0 + i];
      j = (unsigned)pt < (unsigned)npts ? pt : 0;
    }
    s_pt[i] = make_float4(coord[j], coord[mp + j], coord[2 * mp + j], coord[3 * mp + j]);
    if constexpr (C == 5) s_rest[i] = coord[4 * mp + j];
    if constexpr (C == 6) s_rest[i] = make_float2(coord[4 * mp + j], coord[5 * mp + j]);
  }
  __syncthreads();
  const int h = hb * 64 + threadIdx.x;
  if (h >= S.num_loops) return;
  const float *hyp = S.hyp + (size_t)e * Model::PARAMS * lp;
  float a[Model::PARAMS];
#pragma unroll
  for (int k = 0; k < Model::PARAMS; k++) a[k] = hyp[k * lp + h];
  const typename Model::Lane ln = Model::lane(A, e);
  const float thresh2 = S.thresh2;
  int cnt = 0;
  for (int i = 0; i < n; i++) {
    float q[C];                                // the candidate by value, not the LDS element by reference
    const float4 p = s_pt[i];
    q[0] = p.x; q[1] = p.y; q[2] = p.z; q[3] = p.w;
    if constexpr (C == 5) q[4] = s_rest[i];
    if constexpr (C == 6) {
      const float2 r = s_rest[i];
      q[4] = r.x; q[5] = r.y;
    }
    cnt += Model::inlier(a, ln, q, thresh2) ? 1 : 0;
  }
  atomicAdd(&S.hcount[(size_t)e * lp + h], cnt);
}

template <class Model>
__global__ __launch_bounds__(1024) void ransac_gather_kernel(RansacArgs G)
{
  const RansacSearch &S = G.rs;
  const int e = blockIdx.x;
  const int f = G.frames[e];
  const int n = G.set.counts[f];
  int *meta = S.meta + (size_t)RANSAC_META * e;
  if (n < 8 || n > G.max_pts) {                // matching.cu:1016-1017 (count -1 included); over max_pts: -1, nothing read
    if (threadIdx.x == 0) { meta[0] = 0; meta[1] = n > G.max_pts ? -1 : 0; meta[2] = 0; }
    return;
  }
  const float *pts = reinterpret_cast<const float *>(G.set.recs + G.set.base(f));
  const int num_valid = ransac_gather(pts, n, S.cap16, G.min_score, G.max_ambiguity, S.coord + (size_t)e * 4 * S.cap16,
                                      S.index + (size_t)e * S.cap16);
  const int tid = threadIdx.x;
  if (num_valid < 8) {
    if (tid == 0) { meta[0] = 0; meta[1] = 0; meta[2] = 0; }
    return;
  }
  if (tid < 64) {                              // wave 0
    ransac_draw<Model>(S.seeds[e], num_valid, S.sample + (size_t)e * Model::SAMPLE * S.lp, S.num_loops, S.lp);
    if (tid == 0) { meta[0] = Model::COUNT_ALL ? n : num_valid; meta[1] = 0; meta[2] = n; }
  }
}

template <class Model>
__global__ __launch_bounds__(1024) void ransac_pick_kernel(RansacArgs G)
{
  const RansacSearch &S = G.rs;
  const int e = blockIdx.x;
  float *out = G.out + (size_t)9 * e;
  const int *meta = S.meta + (size_t)RANSAC_META * e;
  if (meta[0] == 0) {                          // the model's done result and 0, or -1 for a frame over max_pts
    if (threadIdx.x < 9) out[threadIdx.x] = Model::done(threadIdx.x);
    if (threadIdx.x == 0) G.num[e] = meta[1];
    return;
  }
  const unsigned long long best = ransac_pick(S.hcount + (size_t)e * S.lp, S.num_loops);
  if (threadIdx.x == 0) {
    const int idx = ransac_pick_index(best);
    const float *hyp = S.hyp + (size_t)e * Model::PARAMS * S.lp;
    for (int k = 0; k < Model::PARAMS; k++) out[k] = hyp[k * S.lp + idx];
    Model::picked(out);
    G.num[e] = ransac_pick_count(best);
  }
}

// The entry point's name and what it calls its candidates (for its errors), and the LaunchScope slots of its four
// launches.
struct RansacNames {
  const char *who, *what, *gather, *solve, *count, *pick;
};

inline int ransac_round16(int v) { return (int)(((size_t)v + 15) / 16 * 16); }

// whether the count's grid, nsel x hypothesis blocks x chunks, fits one launch (and cap and num_loops their strides)
inline bool ransac_one_launch(int nsel, int cap, int num_loops)
{
  const long long hb = ((long long)num_loops + 63) / 64, ch = ((long long)cap + RANSAC_CHUNK - 1) / RANSAC_CHUNK;
  return num_loops <= 0x7fffffff - 15 && cap <= 0x7fffffff - 15 && nsel * hb <= 0x7fffffffLL &&
         nsel * hb * ch <= 0x7fffffffLL;
}

// The host side of RansacSearch but the temp, behind the one-launch check.  num_loops is the number of hypotheses the
// search works over: the caller's, or the caller's rounded up to 16, as the launcher decides.
inline int ransac_search(const RansacNames &names, int nsel, int cap, int num_loops, float thresh2, const unsigned *h_seeds,
                         RansacSearch &S)
{
  if (!ransac_one_launch(nsel, cap, num_loops)) {
    misift_set_error("%s: %d entries x %d loops x %d %s is beyond one launch", names.who, nsel, num_loops, cap,
                     names.what);
    return MISIFT_EINVAL;
  }
  S = RansacSearch{};
  S.nsel = nsel; S.cap16 = ransac_round16(cap);
  S.num_loops = num_loops; S.lp = ransac_round16(num_loops);
  S.thresh2 = thresh2;
  S.seeds = h_seeds;
  return MISIFT_OK;
}

// The temp of a search in bytes: prefix_bytes of the model's own ahead of the arrays, tail_words per entry behind them.
template <class Model>
size_t ransac_tmp_bytes(const RansacSearch &S, size_t prefix_bytes, int tail_words)
{
  const size_t words = (Model::COORDS + (Model::INDEX ? 1 : 0)) * (size_t)S.cap16 +
                       (Model::SAMPLE + Model::PARAMS + 1) * (size_t)S.lp + RANSAC_META + tail_words;
  return prefix_bytes + sizeof(float) * (size_t)S.nsel * words;
}

// Sizes the temp (misift_ensure_tmp) and carves S's arrays out of it, each pooled over the entries; *tail gets where the
// model's nsel x tail_words begin.
template <class Model>
int ransac_temp(misift_ctx *ctx, RansacSearch &S, size_t prefix_bytes, int tail_words, void **tail)
{
  const int rc = misift_ensure_tmp(ctx, ransac_tmp_bytes<Model>(S, prefix_bytes, tail_words));
  if (rc) return rc;
  const size_t ns = (size_t)S.nsel, cap = (size_t)S.cap16, lp = (size_t)S.lp;
  S.coord = reinterpret_cast<float *>(reinterpret_cast<char *>(ctx->d_match_tmp) + prefix_bytes);
  S.index = reinterpret_cast<int *>(S.coord + ns * Model::COORDS * cap);
  S.sample = S.index + (Model::INDEX ? ns * cap : 0);
  S.hyp = reinterpret_cast<float *>(S.sample + ns * Model::SAMPLE * lp);
  S.hcount = reinterpret_cast<int *>(S.hyp + ns * Model::PARAMS * lp);
  S.meta = S.hcount + ns * lp;
  if (tail) *tail = S.meta + ns * RANSAC_META;
  return MISIFT_OK;
}

// One launch scope of the profile around what launch() enqueues.
template <class Launch>
int ransac_scope(misift_ctx *ctx, const char *name, Launch launch)
{
  LaunchScope ls(ctx, name);
  launch();
  return ls.finish();
}

// The four launches on the context stream, each in its scope: gather() and pick() enqueue the model's kernels on nsel
// 1024-thread workgroups, solve is its solve kernel, run on nsel * hblocks 64-lane workgroups.
template <class Model, class Gather, class Pick>
int ransac_launches(misift_ctx *ctx, const RansacNames &names, const typename Model::Args &A, Gather gather,
                    void (*solve)(typename Model::Args, int), Pick pick)
{
  const RansacSearch &S = A.rs;
  const int hblocks = (S.num_loops + 63) / 64, chunks = (S.cap16 + RANSAC_CHUNK - 1) / RANSAC_CHUNK;
  int rc = ransac_scope(ctx, names.gather, gather);
  if (rc) return rc;
  rc = ransac_scope(ctx, names.solve, [&] {
    hipLaunchKernelGGL(solve, dim3(S.nsel * hblocks), dim3(64), 0, ctx->stream, A, hblocks);
  });
  if (rc) return rc;
  rc = ransac_scope(ctx, names.count, [&] {
    hipLaunchKernelGGL(ransac_count_kernel<Model>, dim3(S.nsel * hblocks * chunks), dim3(64), 0, ctx->stream, A, hblocks,
                       chunks);
  });
  if (rc) return rc;
  return ransac_scope(ctx, names.pick, pick);
}

// misift_find_homography_batch and misift_find_fundamental_batch from here on: the search over the frames `h_frames` of
// `set`, with the shared gather and pick kernels.
template <class Model>
int ransac_batch_run(misift_ctx *ctx, const RansacNames &names, int nsel, const int *h_frames, const unsigned *h_seeds,
                     const BatchLayout &set, int max_pts, int num_loops, float min_score, float max_ambiguity,
                     float thresh, float *out, int *num, void (*solve)(RansacArgs, int))
{
  RansacArgs G{};
  int rc = ransac_search(names, nsel, max_pts, num_loops, thresh * thresh, h_seeds, G.rs);
  if (!rc) rc = ransac_temp<Model>(ctx, G.rs, 0, 0, nullptr);
  if (rc) return rc;
  G.set = set;
  G.frames = h_frames;
  G.max_pts = max_pts;
  G.min_score = min_score; G.max_ambiguity = max_ambiguity;
  G.out = out; G.num = num;
  return ransac_launches<Model>(
      ctx, names, G,
      [&] { hipLaunchKernelGGL(ransac_gather_kernel<Model>, dim3(nsel), dim3(1024), 0, ctx->stream, G); }, solve,
      [&] { hipLaunchKernelGGL(ransac_pick_kernel<Model>, dim3(nsel), dim3(1024), 0, ctx->stream, G); });
}

// kernels_merge.hip — misift_merge_scenes_batch: two exported scenes in one gauge written out as one export, with the
// points, the cameras and the record index that go with it, so that triangulate, refine, resect, filter and adjust take
// the merged scene unchanged.  No reference counterpart.  The rules are merge_core.hpp, shared with the host-only test
// hook (misift_test_merge_scenes, misift_host.hip).
//
// Three memsets (the owners of both scenes, the counters, the summary) and ten launches, whatever the data:
//   cand_owner_kernel        twice: the owner of every slot of A and of B (track_candidates.hpp, without the keys).
//   merge_class_kernel       one lane per A-track: its class word, and for a PARTNER one more in the count of its B-track
//                            and in the count of that track's tile of 2048.
//   merge_tile_scan_kernel   ONE workgroup: the exclusive prefix sum of the partner tile counts.
//   merge_partner_kernel     per tile: the exclusive scan of the counts inside the tile: where each B-track's list starts.
//   merge_fill_kernel        one lane per A-track: a PARTNER takes the next place of its B-track's list by atomicAdd.  The
//                            order of a list is whatever the hardware made it; the two rules of a union are order-free,
//                            so it does not reach the output.
//   merge_union_kernel       the hot path.  One wavefront per merged index (B-track, or A-track beyond T_B), four to a
//                            workgroup.  The live observations of the track and of its partners are gathered as (key, id)
//                            by ballot and popcount: the first MERGE_STAGE of them into LDS, 16 bytes an element; a longer
//                            union is gathered again into a piece of temp memory taken by one atomicAdd.  Then all pairs:
//                            every lane holds one element and walks all of them in the same order, so an LDS read is a
//                            broadcast: pass 1 marks the elements that lose to a twin, pass 2 counts the kept elements
//                            with a smaller key.  The rank goes to temp per slot, the length to len[] and to the sums of
//                            the track's tile by one 64-bit integer atomic.
//   merge_tile_scan_kernel   again: the prefix sums of (merged tracks, kept observations) per tile; N and the total.
//   merge_number_kernel      per tile: t' and off' of every merged track, the capacity rule, its offsets, its point, the
//                            d_track_map_a entry of an ALONE track.
//   merge_write_kernel       one lane per slot of A, slot of B, A-track, record and image: the observation copied to its
//                            place, both slot maps, the d_track_map_a entry of every other track, d_record_obs_out, the
//                            cameras; T' and O' to the call's own summary.
// No workgroup waits for another.  Every sum is an integer sum and no output depends on where an atomicAdd placed
// something in temp memory, so the outputs are byte-identical from run to run.
#include <stdint.h>
#include "common.hpp"
#include "merge_core.hpp"
#include "scan_core.hpp"
#include "track_candidates.hpp"

namespace {

constexpr int MERGE_THREADS = 256;
constexpr int MERGE_WAVES = MERGE_THREADS / 64;
// elements of a union staged in LDS: a key, an id and a flag, 16 bytes each, 16 KiB a workgroup, so the eight workgroups
// that fill a CU's 32 wave slots take 128 of its 160 KiB and the staging costs no occupancy; the unions of two
// overlapping 64-image windows (at most 128 observations) fit twice over
constexpr int MERGE_STAGE = 256;
constexpr int MERGE_TILE = 2048;               // tracks per scan tile: 256 lanes x 8
constexpr int MERGE_SCAN_WG = 1024;

struct MergeArgs {
  MergeScene a, b;
  const int *map, *accept;
  MergeOut out;
  // temp
  int *owner_a, *owner_b;                      // per slot
  int *rank_a, *rank_b;                        // per slot
  int *cls;                                    // per A-track
  int *pcount, *pcur, *plist;                  // partners per B-track, the cursor of its list (its end once filled), the lists
  unsigned long long *ptile, *tile;            // tile sums, then their prefix sums
  int *len, *dup, *newoff;                     // per merged index
  long long *spill_key;                        // unions beyond the staging: a.max_obs + b.max_obs elements
  unsigned *spill_id;
  int *spill_flag;
  unsigned long long *spill_used;
  int nptiles, ntiles;
  long long spill_cap;
};

__device__ __forceinline__ int wave_sum(int v)
{
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ MergeTables merge_tables(const MergeArgs &A)
{
  return MergeTables{A.owner_a, A.owner_b, A.cls, A.rank_a, A.rank_b, A.newoff};
}

__global__ __launch_bounds__(MERGE_THREADS) void merge_class_kernel(MergeArgs A)
{
  const int t = blockIdx.x * MERGE_THREADS + threadIdx.x;    // below max_tracks_a + 256: no overflow
  int dropped = 0;
  if (t < scene_T(A.a.s)) {
    const bool valid = tri_range_ok(A.a.s.track_offsets[t], A.a.s.track_offsets[t + 1], scene_O(A.a.s));
    const int c = merge_class(valid, A.map[t], scene_T(A.b.s), A.accept, t);
    A.cls[t] = c;
    if (c >= 0) {                              // c < T_B: checked by merge_class before it addresses anything
      atomicAdd(&A.pcount[c], 1);
      atomicAdd(&A.ptile[c / MERGE_TILE], 1ull);
    }
    dropped = c < 0 && c != MERGE_ALONE;
  }
  dropped = wave_sum(dropped);
  if ((threadIdx.x & 63) == 0 && dropped) atomicAdd(&A.out.summary[4], dropped);
}

// The exclusive prefix sums of ntiles packed pairs (high word << 32 | low word), in place.  final: the pairs are (kept
// observations, merged tracks): N, the total and the zeros of the export summary, and the first offset.
__global__ __launch_bounds__(MERGE_SCAN_WG) void merge_tile_scan_kernel(MergeArgs A, unsigned long long *tile, int ntiles,
                                                                        int final)
{
  __shared__ uint2 red[MERGE_SCAN_WG / 64];
  uint2 carry = make_uint2(0, 0);
  for (int t0 = 0; t0 < ntiles; t0 += MERGE_SCAN_WG) {
    const int t = t0 + threadIdx.x;
    const unsigned long long w = t < ntiles ? tile[t] : 0ull;
    const uint2 v = make_uint2((unsigned)w, (unsigned)(w >> 32));
    uint2 total;
    const uint2 ex = exp_block_scan<MERGE_SCAN_WG / 64>(v, red, total);
    if (t < ntiles) tile[t] = ((unsigned long long)(carry.y + ex.y) << 32) | (carry.x + ex.x);
    carry.x += total.x; carry.y += total.y;
  }
  if (final && threadIdx.x == 0) {
    int *es = A.out.export_summary;
    es[0] = (int)carry.x;
    es[1] = (int)carry.y;
    es[2] = es[3] = es[4] = es[5] = es[6] = es[7] = 0;
    A.out.track_offsets[0] = 0;
  }
}

__global__ __launch_bounds__(256) void merge_partner_kernel(MergeArgs A)
{
  __shared__ uint2 red[4];
  const int TB = scene_T(A.b.s);
  for (int tile = blockIdx.x; tile < A.nptiles; tile += gridDim.x) {
    const long long i0 = (long long)tile * MERGE_TILE + threadIdx.x * 8;
    int v[8];
    uint2 mine = make_uint2(0, 0);
    for (int k = 0; k < 8; k++) {
      v[k] = i0 + k < TB ? A.pcount[i0 + k] : 0;
      mine.x += (unsigned)v[k];
    }
    uint2 total;
    uint2 ex = exp_block_scan<4>(mine, red, total);
    ex.x += (unsigned)A.ptile[tile];
    for (int k = 0; k < 8; k++) {
      if (i0 + k < TB) A.pcur[i0 + k] = (int)ex.x;
      ex.x += (unsigned)v[k];
    }
  }
}

__global__ __launch_bounds__(MERGE_THREADS) void merge_fill_kernel(MergeArgs A)
{
  const int t = blockIdx.x * MERGE_THREADS + threadIdx.x;
  if (t >= scene_T(A.a.s)) return;
  const int c = A.cls[t];
  if (c < 0) return;
  const int at = atomicAdd(&A.pcur[c], 1);
  if (at >= 0 && at < A.a.s.max_tracks) A.plist[at] = t;     // always: the lists hold T_A entries at the most
}

// The live observations that track t of scene S owns, appended to the union from position `pos` on: sink(p, key, id) per
// element in ascending slot.  The same in every lane of the wavefront; returns the new length.
template <class Sink>
__device__ __forceinline__ int merge_gather(const MergeScene &S, int source, const int *owner, int t, int pos, Sink sink)
{
  const int lane = threadIdx.x & 63;
  const int off = S.s.track_offsets[t], end = S.s.track_offsets[t + 1];
  if (!tri_range_ok(off, end, scene_O(S.s))) return pos;      // before it addresses anything
  for (long long o0 = off; o0 < end; o0 += 64) {
    const long long o = o0 + lane;
    bool ok = o < end && owner[o] == t;
    TrackObs ob{};
    if (ok) {
      ob = track_obs_load(S.s.obs + o);
      ok = merge_live(ob.frame, S.s.nimages);
    }
    const unsigned long long mask = __ballot(ok);
    if (ok)
      sink(pos + __popcll(mask & ((1ull << lane) - 1ull)), merge_key(ob.frame, S.fshift, ob.record),
           merge_id(source, (int)o));
    pos += __popcll(mask);
  }
  return pos;
}

// the union of merged index i: B-track i and its partners, or the ALONE A-track i - T_B
template <class Sink>
__device__ __forceinline__ int merge_gather_union(const MergeArgs &A, long long i, int TB, int pbeg, int pend, Sink sink)
{
  if (i >= TB) return merge_gather(A.a, 1, A.owner_a, (int)(i - TB), 0, sink);
  int n = merge_gather(A.b, 0, A.owner_b, (int)i, 0, sink);
  for (int p = pbeg; p < pend; p++) {
    const int t = A.plist[p];
    if (t >= 0 && t < scene_T(A.a.s)) n = merge_gather(A.a, 1, A.owner_a, t, n, sink);
  }
  return n;
}

// The two rules of a union (rule 3: which element is kept, and its place) over the n gathered elements, all pairs;
// returns this lane's number of kept elements.  key, id and flag are the LDS staging or the piece of temp memory: each
// call site is inlined with its own address space.
__device__ __forceinline__ int merge_rank_union(const MergeArgs &A, int n, const long long *key, const unsigned *id,
                                                int *flag, bool in_lds)
{
  const int lane = threadIdx.x & 63;
  for (int e0 = 0; e0 < n; e0 += 64) {
    const int e = e0 + lane;
    const bool have = e < n;
    const long long mykey = have ? key[e] : 0;
    const unsigned myid = have ? id[e] : 0u;
    bool loses = false;
    for (int j = 0; j < n; j++) loses = loses || merge_loses(mykey, myid, key[j], id[j]);
    if (have) flag[e] = !loses;
  }
  if (in_lds) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    __threadfence();                           // the flags are read by the other lanes below
  }
  int m = 0;
  for (int e0 = 0; e0 < n; e0 += 64) {
    const int e = e0 + lane;
    if (e >= n) continue;                      // no cross-lane operation below
    const long long mykey = key[e];
    const unsigned myid = id[e];
    int r = 0;
    for (int j = 0; j < n; j++) r += flag[j] != 0 && key[j] < mykey;
    const bool kept = flag[e] != 0;
    ((myid >> 31) ? A.rank_a : A.rank_b)[myid & 0x7fffffffu] = kept ? r : ~r;
    m += kept;
  }
  return m;
}

__global__ __launch_bounds__(MERGE_THREADS) void merge_union_kernel(MergeArgs A)
{
  __shared__ long long s_key[MERGE_WAVES][MERGE_STAGE];
  __shared__ unsigned s_id[MERGE_WAVES][MERGE_STAGE];
  __shared__ int s_flag[MERGE_WAVES][MERGE_STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long i = (long long)blockIdx.x * MERGE_WAVES + wave;
  const int TB = scene_T(A.b.s), TA = scene_T(A.a.s);
  if (i >= (long long)TB + TA) return;          // the same in every lane of the wavefront; no workgroup barrier below
  int pbeg = 0, pend = 0;
  if (i >= TB) {
    if (A.cls[i - TB] != MERGE_ALONE) {         // no merged track of its own
      if (lane == 0) A.len[i] = -1;
      return;
    }
  } else {
    pend = A.pcur[i];
    pbeg = pend - A.pcount[i];
    if (pbeg < 0 || pbeg > pend || pend > A.a.s.max_tracks) pbeg = pend = 0;   // never: the lists are this call's own
  }
  long long *key = s_key[wave];
  unsigned *id = s_id[wave];
  int *flag = s_flag[wave];
  const int n = merge_gather_union(A, i, TB, pbeg, pend, [&](int p, long long k, unsigned d) {
    if (p < MERGE_STAGE) { key[p] = k; id[p] = d; }
  });
  int m = 0;
  if (n <= MERGE_STAGE) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    m = merge_rank_union(A, n, key, id, flag, true);
  } else {
    // a piece of temp memory of its own: every slot has one owner and every A-track one union, so the pieces of all
    // long unions together hold a.max_obs + b.max_obs elements at the most
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(A.spill_used, (unsigned long long)n);
    base = __shfl(base, 0, 64);
    if (base + (unsigned long long)n <= (unsigned long long)A.spill_cap) {      // always; checked all the same
      long long *gkey = A.spill_key + base;
      unsigned *gid = A.spill_id + base;
      merge_gather_union(A, i, TB, pbeg, pend, [&](int p, long long k, unsigned d) { gkey[p] = k; gid[p] = d; });
      __threadfence();                         // the elements are read by the other lanes
      m = merge_rank_union(A, n, gkey, gid, A.spill_flag + base, false);
    }
  }
  m = wave_sum(m);
  if (lane != 0) return;
  A.len[i] = m;
  A.dup[i] = n - m;
  atomicAdd(&A.tile[i / MERGE_TILE], ((unsigned long long)(unsigned)m << 32) | 1ull);   // at most 2048 per tile: no carry
}

__global__ __launch_bounds__(256) void merge_number_kernel(MergeArgs A)
{
  __shared__ uint2 red[4];
  __shared__ int s_longest[4];
  const int TB = scene_T(A.b.s), TA = scene_T(A.a.s);
  const long long ntot = (long long)TB + TA;
  const MergeOut &Q = A.out;
  int longest = 0, dups = 0, alone = 0, cut = 0, tmax = 0, omax = 0;
  for (int tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
    const long long i0 = (long long)tile * MERGE_TILE + threadIdx.x * 8;
    int v[8];
    uint2 mine = make_uint2(0, 0);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      v[k] = i0 + k < ntot ? A.len[i0 + k] : -1;     // len[] is written below T_B + T_A only
      mine.x += v[k] >= 0; mine.y += v[k] >= 0 ? (unsigned)v[k] : 0u;
    }
    uint2 total;
    uint2 ex = exp_block_scan<4>(mine, red, total);
    const unsigned long long before = A.tile[tile];
    ex.x += (unsigned)before; ex.y += (unsigned)(before >> 32);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const long long i = i0 + k;
      if (i >= ntot) continue;
      const int m = v[k];
      if (m < 0) {
        A.newoff[i] = -1;
        continue;
      }
      const long long tn = ex.x, off = ex.y;
      ex.x += 1; ex.y += (unsigned)m;
      const bool written = merge_written(tn, off, m, Q.max_tracks, Q.max_obs);
      A.newoff[i] = written ? (int)off : -1;
      if (i >= TB) Q.track_map_a[i - TB] = written ? (int)tn : MERGE_CUT;
      if (!written) {
        cut++;
        continue;
      }
      const MergeScene &S = i < TB ? A.b : A.a;
      const int t = (int)(i < TB ? i : i - TB);
      Q.track_offsets[tn + 1] = (int)(off + m);
      Q.point_views[tn] = S.point_views[t];
      Q.point_status[tn] = S.s.point_status[t];
      const unsigned *src = reinterpret_cast<const unsigned *>(S.s.points) + 4 * (size_t)t;
      unsigned *dst = reinterpret_cast<unsigned *>(Q.points) + 4 * (size_t)tn;
      dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
      tmax = max(tmax, (int)tn + 1);           // the written tracks are a prefix, so the largest of these is T' and O'
      omax = max(omax, (int)(off + m));
      longest = max(longest, m);
      dups += A.dup[i];
      alone += i >= TB;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    longest = max(longest, __shfl_xor(longest, o, 64));
    tmax = max(tmax, __shfl_xor(tmax, o, 64));
    omax = max(omax, __shfl_xor(omax, o, 64));
  }
  dups = wave_sum(dups); alone = wave_sum(alone); cut = wave_sum(cut);
  if ((threadIdx.x & 63) == 0) {
    s_longest[threadIdx.x >> 6] = longest;
    if (tmax) atomicMax(&Q.export_summary[2], tmax);
    if (omax) atomicMax(&Q.export_summary[3], omax);
    if (dups) atomicAdd(&Q.summary[5], dups);
    if (alone) atomicAdd(&Q.summary[3], alone);
    if (cut) atomicAdd(&Q.summary[6], cut);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) longest = max(longest, s_longest[w]);
    if (longest) atomicMax(&Q.export_summary[4], longest);
  }
}

// one lane per slot of A, slot of B, A-track, record and image, in this order; nothing of one part waits for another
__global__ __launch_bounds__(MERGE_THREADS) void merge_write_kernel(MergeArgs A, long long n_slots_a, long long n_slots_b,
                                                                    long long n_tracks_a, long long n_records)
{
  long long k = (long long)blockIdx.x * MERGE_THREADS + threadIdx.x;
  const MergeOut &Q = A.out;
  const int TB = scene_T(A.b.s);
  const MergeTables M = merge_tables(A);
  int partners = 0, from_a = 0;
  if (k < n_slots_a + n_slots_b) {
    const int source = k < n_slots_a;
    const MergeScene &S = source ? A.a : A.b;
    const int o = (int)(source ? k : k - n_slots_a);
    if (o < scene_O(S.s)) {
      bool kept;
      const int m = merge_slot_map(S, source, M, TB, o, &kept);
      int *obs_map = source ? Q.obs_map_a : Q.obs_map_b;
      if (obs_map) obs_map[o] = m;
      if (kept && m < Q.max_obs) {             // m < O' always: the rank of a kept element is below its track's length
        const TrackObs ob = track_obs_load(S.s.obs + o);
        reinterpret_cast<int4 *>(Q.obs)[m] =
            make_int4(ob.frame + S.fshift, ob.record, __float_as_int(ob.xpos), __float_as_int(ob.ypos));
      }
    }
  } else if ((k -= n_slots_a + n_slots_b) < n_tracks_a) {
    const int t = (int)k;
    if (t < scene_T(A.a.s)) {
      const int c = A.cls[t];
      if (c != MERGE_ALONE) {                  // an ALONE track got its entry with its number
        const bool written = c >= 0 && A.newoff[c] >= 0;
        Q.track_map_a[t] = c < 0 ? c : written ? c : MERGE_CUT;
        partners = written;
      }
    }
  } else if ((k -= n_tracks_a) < n_records) {
    Q.record_obs[k] = merge_record(A.a, A.b, M, TB, (int)k);
  } else if ((k -= n_records) < Q.nimages) {
    int src;
    const int from = merge_camera_source(A.a, A.b, (int)k, &src);
    unsigned w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int pair = POSEGRAPH_UNSET;
    if (from >= 0) {
      const MergeScene &S = from ? A.a : A.b;
      const unsigned *in = reinterpret_cast<const unsigned *>(S.s.cam) + 12 * (size_t)src;
#pragma unroll
      for (int j = 0; j < 12; j++) w[j] = in[j];
      pair = from ? MERGE_CAM_MERGED : S.s.cam_pair[src];
      from_a = from;
    }
    unsigned *out = reinterpret_cast<unsigned *>(Q.cam) + 12 * (size_t)k;
#pragma unroll
    for (int j = 0; j < 12; j++) out[j] = w[j];
    Q.cam_pair[k] = pair;
    if (k == 0) {                              // T' and O' are final: the numbering is an earlier launch
      Q.summary[0] = Q.export_summary[2];
      Q.summary[1] = Q.export_summary[3];
    }
  }
  partners = wave_sum(partners); from_a = wave_sum(from_a);
  if ((threadIdx.x & 63) == 0) {
    if (partners) atomicAdd(&Q.summary[2], partners);
    if (from_a) atomicAdd(&Q.summary[7], from_a);
  }
}

size_t merge_align16(size_t v) { return (v + 15) / 16 * 16; }

struct MergeSizes {
  size_t slots, tracks_a, tracks_b, merged, nptiles, ntiles;
};

MergeSizes merge_sizes(int max_tracks_a, int max_obs_a, int max_tracks_b, int max_obs_b)
{
  MergeSizes z;
  z.slots = (size_t)max_obs_a + (size_t)max_obs_b;
  z.tracks_a = (size_t)max_tracks_a;
  z.tracks_b = (size_t)max_tracks_b;
  z.merged = z.tracks_a + z.tracks_b;
  z.nptiles = (z.tracks_b + MERGE_TILE - 1) / MERGE_TILE;
  z.ntiles = (z.merged + MERGE_TILE - 1) / MERGE_TILE;
  return z;
}

}  // namespace

size_t merge_scenes_batch_tmp_bytes(int max_tracks_a, int max_obs_a, int max_tracks_b, int max_obs_b)
{
  const MergeSizes z = merge_sizes(max_tracks_a, max_obs_a, max_tracks_b, max_obs_b);
  return merge_align16(4 * z.slots) * 4 + merge_align16(8 * z.slots) +          // owners, ranks, spill ids, flags; keys
         2 * merge_align16(4 * z.tracks_a) + 2 * merge_align16(4 * z.tracks_b) +  // cls, plist; pcount, pcur
         3 * merge_align16(4 * z.merged) + merge_align16(8 * z.nptiles) + merge_align16(8 * z.ntiles) + 16;
}

// Enqueue misift_merge_scenes_batch on the context stream (common.hpp): three memsets and ten launches.
int launch_merge_scenes_batch(misift_ctx *ctx, const MergeIn &in)
{
  const int mta = in.a.s.max_tracks, moa = in.a.s.max_obs, mtb = in.b.s.max_tracks, mob = in.b.s.max_obs;
  const int rc = misift_ensure_tmp(ctx, merge_scenes_batch_tmp_bytes(mta, moa, mtb, mob));
  if (rc) return rc;
  const MergeSizes z = merge_sizes(mta, moa, mtb, mob);
  MergeArgs A{};
  A.a = in.a; A.b = in.b; A.map = in.map; A.accept = in.accept; A.out = in.out;
  char *t = reinterpret_cast<char *>(ctx->d_match_tmp);
  const auto take = [&](size_t bytes) { char *p = t; t += merge_align16(bytes); return p; };
  // the owners of both scenes lie side by side (one memset to -1), and so does everything that starts at zero
  char *owners = take(4 * z.slots);
  A.owner_a = reinterpret_cast<int *>(owners);
  A.owner_b = A.owner_a + moa;
  char *zeros = t;
  A.pcount = reinterpret_cast<int *>(take(4 * z.tracks_b));
  A.ptile = reinterpret_cast<unsigned long long *>(take(8 * z.nptiles));
  A.tile = reinterpret_cast<unsigned long long *>(take(8 * z.ntiles));
  A.spill_used = reinterpret_cast<unsigned long long *>(take(16));
  const size_t zero_bytes = (size_t)(t - zeros);
  A.rank_a = reinterpret_cast<int *>(take(4 * z.slots));
  A.rank_b = A.rank_a + moa;
  A.spill_id = reinterpret_cast<unsigned *>(take(4 * z.slots));
  A.spill_flag = reinterpret_cast<int *>(take(4 * z.slots));
  A.spill_key = reinterpret_cast<long long *>(take(8 * z.slots));
  A.cls = reinterpret_cast<int *>(take(4 * z.tracks_a));
  A.plist = reinterpret_cast<int *>(take(4 * z.tracks_a));
  A.pcur = reinterpret_cast<int *>(take(4 * z.tracks_b));
  A.len = reinterpret_cast<int *>(take(4 * z.merged));
  A.dup = reinterpret_cast<int *>(take(4 * z.merged));
  A.newoff = reinterpret_cast<int *>(take(4 * z.merged));
  A.nptiles = (int)z.nptiles; A.ntiles = (int)z.ntiles; A.spill_cap = (long long)z.slots;
  HIP_TRY(hipMemsetAsync(owners, 0xff, 4 * z.slots, ctx->stream));
  HIP_TRY(hipMemsetAsync(zeros, 0, zero_bytes, ctx->stream));
  HIP_TRY(hipMemsetAsync(in.out.summary, 0, 8 * sizeof(int), ctx->stream));
  const int ncu = ctx->num_cus > 0 ? ctx->num_cus : 256;
  const auto blocks = [](long long n, int per) { return dim3((unsigned)((n + per - 1) / per)); };
  int lrc;
  {
    LaunchScope ls(ctx, "merge_owner");
    launch_track_candidates(ctx, in.a.s, A.owner_a, nullptr);
    launch_track_candidates(ctx, in.b.s, A.owner_b, nullptr);
    if ((lrc = ls.finish())) return lrc;
  }
  {
    LaunchScope ls(ctx, "merge_partners");
    hipLaunchKernelGGL(merge_class_kernel, blocks(mta, MERGE_THREADS), dim3(MERGE_THREADS), 0, ctx->stream, A);
    hipLaunchKernelGGL(merge_tile_scan_kernel, dim3(1), dim3(MERGE_SCAN_WG), 0, ctx->stream, A, A.ptile, A.nptiles, 0);
    hipLaunchKernelGGL(merge_partner_kernel, dim3(A.nptiles < 8 * ncu ? A.nptiles : 8 * ncu), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(merge_fill_kernel, blocks(mta, MERGE_THREADS), dim3(MERGE_THREADS), 0, ctx->stream, A);
    if ((lrc = ls.finish())) return lrc;
  }
  {
    LaunchScope ls(ctx, "merge_union");
    hipLaunchKernelGGL(merge_union_kernel, blocks((long long)z.merged, MERGE_WAVES), dim3(MERGE_THREADS), 0, ctx->stream, A);
    if ((lrc = ls.finish())) return lrc;
  }
  {
    LaunchScope ls(ctx, "merge_number");
    hipLaunchKernelGGL(merge_tile_scan_kernel, dim3(1), dim3(MERGE_SCAN_WG), 0, ctx->stream, A, A.tile, A.ntiles, 1);
    hipLaunchKernelGGL(merge_number_kernel, dim3(A.ntiles < 8 * ncu ? A.ntiles : 8 * ncu), dim3(256), 0, ctx->stream, A);
    if ((lrc = ls.finish())) return lrc;
  }
  LaunchScope ls(ctx, "merge_write");
  const long long nrec = in.out.record_obs ? in.out.max_records : 0;
  const long long items = (long long)z.slots + mta + nrec + in.out.nimages;
  hipLaunchKernelGGL(merge_write_kernel, blocks(items, MERGE_THREADS), dim3(MERGE_THREADS), 0, ctx->stream, A,
                     (long long)moa, (long long)mob, (long long)mta, nrec);
  return ls.finish();
}

extern "C" int misift_test_merge_capacity(void) { return MERGE_STAGE; }

// kernels_tracks.hip — feature tracks of a pair-indexed match batch (misift_link_tracks_batch): the connected components
// of the accepted matches over all pairs, as a lock-free union-find on the global record index g(f, r) = base(f) + r.
// Further down: misift_export_tracks_batch, which turns the labels into compact observation lists.
//
// One memset and five launches, whatever npairs and whatever the data:
//   memset                    the (root, frame) table of tracks_frames_kernel to all-ones (= empty);
//   tracks_init_kernel        parent[g] = g, len[g] = frames[g] = 0 for every valid record; per pair the range-checked
//                             (base1, rows, base2, n2) the hook reads, copied out of the pinned pair list; summary = 0;
//   tracks_hook_kernel        one lane per (pair, row): the gates, then find both roots and link the larger root under
//                             the smaller with a compare-and-swap, retried from the new roots when another lane got there
//                             first.  parent[x] <= x always, so the root of a component ends as its smallest index.  Every
//                             access to parent[] in this launch is an agent-scope relaxed atomic (the XCDs' L2s are not
//                             coherent, a CU's L1 is never refreshed): a stale parent is still an ancestor, and the
//                             compare-and-swap itself is decided in memory.  No lane waits for another workgroup;
//   tracks_label_kernel       per valid record: walk to the root (plain loads: the hook launch is over), track[g] = root,
//                             len[root] += 1;
//   tracks_frames_kernel      per valid record of a track longer than 1: insert the full 64-bit key (root, frame) into an
//                             open-addressed table of 2 * max_records slots; the lane whose insert took the slot adds 1 to
//                             frames[root].  Keys are compared whole, so there is no false positive.  A singleton's
//                             frames is 1 without the table;
//   tracks_summary_kernel     per root: the summary's sums and maximum; per frame: the dropped ones.
// Every sum is an integer sum and every label a minimum, so all outputs are functions of the edge set alone: byte-identical
// from run to run whatever the dispatch order.
//
// Every index that comes from device data (counts, offsets, row counts, match) is range-checked before it is used: a
// frame takes part only if all its records lie in [0, max_records), and an edge only if both its frames do.  The root
// walks are bounded by max_records steps, so corrupt input cannot hang the device.
#include <stdint.h>
#include "common.hpp"
#include "scan_core.hpp"

namespace {

constexpr unsigned long long TRK_EMPTY = ~0ull;

struct TrkPair {          // one pair, range-checked: rows < rows1 of it are candidates, matches in [0, n2) are valid
  int base1, rows1, base2, n2;
};

struct TrkArgs {
  BatchLayout set;        // recs unused (the records are not an argument); counts / offsets / stride of the batch
  int nframes, max_records;
  const int *pairs;       // pinned host copy, npairs x 2
  int npairs, max_pts;
  const SiftPointD *rows;
  const int *row_counts;
  float min_score, max_ambiguity, max_error;
  int use_error;
  int *parent;            // temp, max_records
  TrkPair *pinfo;         // temp, npairs
  unsigned long long *table;   // temp, table_slots
  unsigned table_slots;
  int *track, *len, *frames, *summary;
};

// Frame f of the batch: n = its record count, base = its first global index; false when it holds records that do not all
// lie in [0, max_records) (such a frame takes no part).  An empty frame is always fine and has base 0.
__device__ __forceinline__ bool trk_frame(const TrkArgs &A, int f, int &base, int &n)
{
  n = max(A.set.counts[f], 0);
  const long long b = A.set.base(f);
  const bool ok = n == 0 || (b >= 0 && b + n <= (long long)A.max_records);
  base = ok && n > 0 ? (int)b : 0;
  return ok;
}

__device__ __forceinline__ int trk_load(int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x as far as this lane can see, inside the hook launch; halves the path on the way (fetch_min: parent[] only
// ever moves towards the root, and a root is never written here, since gp < p <= x there).
__device__ __forceinline__ int trk_find_atomic(int *parent, int x, int bound)
{
  for (int s = 0; s < bound; s++) {
    const int p = trk_load(parent + x);
    if (p == x) break;
    const int gp = trk_load(parent + p);
    if (gp == p) return p;
    __hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = gp;
  }
  return x;
}

__global__ __launch_bounds__(256) void tracks_init_kernel(TrkArgs A)
{
  for (int f = blockIdx.y; f < A.nframes; f += gridDim.y) {
    int base, n;
    if (!trk_frame(A, f, base, n)) continue;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
      const int g = base + r;
      A.parent[g] = g;
      A.len[g] = 0;
      A.frames[g] = 0;
    }
  }
  const long long tid = ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
  const long long nthreads = (long long)gridDim.x * gridDim.y * 256;
  if (tid < 8) A.summary[tid] = 0;
  for (long long i = tid; i < A.npairs; i += nthreads) {
    const int f1 = A.pairs[2 * i], f2 = A.pairs[2 * i + 1];      // checked by the host: in [0, nframes)
    TrkPair P;
    int n1;
    const bool ok1 = trk_frame(A, f1, P.base1, n1);
    const bool ok2 = trk_frame(A, f2, P.base2, P.n2);
    P.rows1 = ok1 && ok2 ? max(min(min(A.row_counts[i], n1), A.max_pts), 0) : 0;
    if (!ok2) P.n2 = 0;
    A.pinfo[i] = P;
  }
}

__global__ __launch_bounds__(256) void tracks_hook_kernel(TrkArgs A)
{
  const long long total = (long long)A.npairs * A.max_pts;
  const long long step = (long long)gridDim.x * 256;
  int accepted = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    const int pi = (int)(i / A.max_pts), r = (int)(i - (long long)pi * A.max_pts);
    const TrkPair P = A.pinfo[pi];
    if (r >= P.rows1) continue;
    const SiftPointD &row = A.rows[i];
    const int m = row.match;
    bool ok = m >= 0 && m < P.n2 && row.score > A.min_score && row.ambiguity < A.max_ambiguity;   // matching.cu:1035
    if (ok && A.use_error) ok = row.match_error < A.max_error;
    if (!ok) continue;
    accepted++;
    int a = trk_find_atomic(A.parent, P.base1 + r, A.max_records);
    int b = trk_find_atomic(A.parent, P.base2 + m, A.max_records);
    // each failed compare-and-swap means another lane linked `hi` meanwhile; the bound only guards against corrupt memory
    for (int tries = 0; a != b && tries < A.max_records; tries++) {
      const int hi = max(a, b), lo = min(a, b);
      int expect = hi;
      if (__hip_atomic_compare_exchange_strong(A.parent + hi, &expect, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT))
        break;
      a = trk_find_atomic(A.parent, expect, A.max_records);      // expect: the parent `hi` has now
      b = trk_find_atomic(A.parent, lo, A.max_records);
    }
  }
  // per wavefront: one add of the lanes' accepted rows
  for (int o = 32; o > 0; o >>= 1) accepted += __shfl_xor(accepted, o);
  if ((threadIdx.x & 63) == 0 && accepted > 0) atomicAdd(A.summary + 0, accepted);
}

__global__ __launch_bounds__(256) void tracks_label_kernel(TrkArgs A)
{
  for (int f = blockIdx.y; f < A.nframes; f += gridDim.y) {
    int base, n;
    if (!trk_frame(A, f, base, n)) continue;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
      const int g = base + r;
      int x = g;
      for (int s = 0; s < A.max_records; s++) {
        const int p = A.parent[x];
        if (p == x) break;
        x = p;
      }
      A.track[g] = x;
      atomicAdd(A.len + x, 1);
    }
  }
}

__device__ __forceinline__ unsigned trk_hash(unsigned long long k)
{
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (unsigned)k;
}

__global__ __launch_bounds__(256) void tracks_frames_kernel(TrkArgs A)
{
  for (int f = blockIdx.y; f < A.nframes; f += gridDim.y) {
    int base, n;
    if (!trk_frame(A, f, base, n)) continue;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
      const int root = A.track[base + r];
      if (A.len[root] == 1) {                                    // a singleton: its root is this record
        A.frames[root] = 1;
        continue;
      }
      const unsigned long long key = ((unsigned long long)(unsigned)root << 32) | (unsigned)f;
      unsigned slot = (unsigned)(((unsigned long long)trk_hash(key) * A.table_slots) >> 32);
      // at most max_records keys in 2 * max_records slots: an empty slot always turns up
      for (unsigned probes = 0; probes < A.table_slots; probes++) {
        const unsigned long long old = atomicCAS(A.table + slot, TRK_EMPTY, key);
        if (old == TRK_EMPTY) {
          atomicAdd(A.frames + root, 1);
          break;
        }
        if (old == key) break;
        slot = slot + 1 == A.table_slots ? 0 : slot + 1;
      }
    }
  }
}

__global__ __launch_bounds__(256) void tracks_summary_kernel(TrkArgs A)
{
  int tracks = 0, records = 0, bad = 0, longest = 0, dropped = 0;
  for (int f = blockIdx.y; f < A.nframes; f += gridDim.y) {
    int base, n;
    if (!trk_frame(A, f, base, n)) {
      if (blockIdx.x == 0 && threadIdx.x == 0) dropped++;
      continue;
    }
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
      const int g = base + r;
      if (A.track[g] != g) continue;
      const int len = A.len[g];
      longest = max(longest, len);
      if (len < 2) continue;
      tracks++;
      records += len;
      bad += len != A.frames[g];
    }
  }
  // per wavefront, then per workgroup through LDS: the adds of a launch all go to the same five words, which serve them
  // one at a time
  for (int o = 32; o > 0; o >>= 1) {
    tracks += __shfl_xor(tracks, o);
    records += __shfl_xor(records, o);
    bad += __shfl_xor(bad, o);
    longest = max(longest, __shfl_xor(longest, o));
    dropped += __shfl_xor(dropped, o);
  }
  __shared__ int red[4][5];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave][0] = tracks; red[wave][1] = records; red[wave][2] = bad; red[wave][3] = longest; red[wave][4] = dropped;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) {
      tracks += red[w][0]; records += red[w][1]; bad += red[w][2];
      longest = max(longest, red[w][3]);
      dropped += red[w][4];
    }
    if (tracks) atomicAdd(A.summary + 1, tracks);
    if (records) atomicAdd(A.summary + 2, records);
    if (bad) atomicAdd(A.summary + 3, bad);
    if (longest) atomicMax(A.summary + 4, longest);
    if (dropped) atomicAdd(A.summary + 5, dropped);
  }
}

size_t trk_align16(size_t v) { return (v + 15) / 16 * 16; }

// ---------------------------------------------------------------------------------------------------------------------
// misift_export_tracks_batch: the labels of misift_link_tracks_batch turned into a compact array of tracks, each with its
// observations (frame, record, xpos, ypos) stored contiguously in ascending order of the global index.
//
// One memset and six launches, whatever the data:
//   memset                        sel[] and cursor[] (8 bytes per record of max_records) to 0: a slot that is no frame's
//                                 valid record contributes zeros to the scan;
//   tracks_export_select_kernel   per valid record g: sel[g] = len if g is a selected root (track[g] == g, len >= min_len,
//                                 len == frames when consistent_only), else 0.  One array carries both scanned values:
//                                 min_len >= 1, so sel[g] > 0 is the "selected" flag;
//   tracks_export_reduce_kernel   per tile of 2048 indices: (selected roots, their lengths) summed into tile[];
//   tracks_export_scan_kernel     ONE workgroup: the exclusive prefix sum of tile[] in place, 1024 tiles per step with a
//                                 running carry, so any max_records is covered; then summary[0..7] (the totals, the
//                                 dropped frames, zeros for the words the next launch adds to) and track_offsets[0] = 0;
//   tracks_export_apply_kernel    per tile: the exclusive scan inside the tile on top of tile[], which gives every
//                                 selected root its number t and its offset off.  The root tests the capacity rule on
//                                 its own (t < max_tracks, off + len <= max_obs); a written root stores track_root[t],
//                                 track_offsets[t + 1] = off + len and place[g] = off, every other index place[g] = -1.
//                                 summary[2..4] are integer sums / a maximum, reduced per workgroup through LDS first;
//   tracks_export_place_kernel    per valid record of a written track: members[off + cursor[root]++] = g.  The order
//                                 inside a segment is whatever the atomics gave;
//   tracks_export_write_kernel    per valid record of a written track: its rank = the entries of its track's segment
//                                 that are smaller than g, which no longer depends on that order; the observation goes
//                                 to obs[off + rank] as one 16-byte store and record_obs[g] = off + rank; every other
//                                 valid record gets record_obs[g] = -1.  A consistent track is at most nframes long, so
//                                 the count is short where it matters; an inconsistent track of len records costs
//                                 len * len compares (4097 records: 17 M, still far below a millisecond of the chip).
// The scan is reduce / scan of the tile sums / apply in separate launches: no workgroup waits for another one.
//
// Arrays that no misift_link_tracks_batch call wrote: a length is accepted only in [1, max_records], a root index only
// in [0, max_records), a track is written only if its whole segment lies in [0, min(max_obs, max_records)), a member is
// placed only below its track's length, and a rank is used only below it.  The sums are unsigned (they wrap instead of
// overflowing), and every loop is bounded by a capacity.  So such arrays give unspecified contents inside the
// capacities and nothing else.
constexpr int EXP_TILE = 2048;      // indices per scan tile: 256 lanes x 8
constexpr int EXP_SCAN_WG = 1024;   // tile sums per step of the one-workgroup scan

struct ExpArgs {
  TrkArgs T;              // set (recs: xpos / ypos of the written records), nframes, max_records, track, len, frames, summary
  int min_len, consistent_only, max_tracks, max_obs;
  int cap;                // min(max_obs, max_records): the members array holds max_records entries
  int ntiles;
  int *sel;               // temp, max_records: len of a selected root, else 0
  int *cursor;            // temp, max_records: members placed so far, per root
  int *place;             // temp, max_records: off of a written root, else -1
  int *members;           // temp, max_records: the global indices of the written tracks' members, one segment per track
  uint2 *tile;            // temp, ntiles: (selected roots, their lengths) per tile, then their exclusive prefix sums
  int *track_offsets, *track_root, *record_obs;
  int4 *obs;
};

// exp_wave_scan and exp_block_scan: scan_core.hpp

__global__ __launch_bounds__(256) void tracks_export_select_kernel(ExpArgs E)
{
  const TrkArgs &A = E.T;
  for (int f = blockIdx.y; f < A.nframes; f += gridDim.y) {
    int base, n;
    if (!trk_frame(A, f, base, n)) continue;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
      const int g = base + r;
      if (A.track[g] != g) continue;
      const int len = A.len[g];
      if (len < E.min_len || len > A.max_records) continue;
      if (E.consistent_only && len != A.frames[g]) continue;
      E.sel[g] = len;
    }
  }
}

// The 8 entries of sel[] a lane owns in tile `tile`; zeros beyond max_records.
__device__ __forceinline__ void exp_load8(const ExpArgs &E, int tile, int v[8])
{
  const long long i0 = (long long)tile * EXP_TILE + threadIdx.x * 8;
  if (i0 + 8 <= E.T.max_records) {
    const int4 a = *reinterpret_cast<const int4 *>(E.sel + i0), b = *reinterpret_cast<const int4 *>(E.sel + i0 + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    for (int k = 0; k < 8; k++) v[k] = i0 + k < E.T.max_records ? E.sel[i0 + k] : 0;
  }
}

__global__ __launch_bounds__(256) void tracks_export_reduce_kernel(ExpArgs E)
{
  __shared__ uint2 red[4];
  for (int tile = blockIdx.x; tile < E.ntiles; tile += gridDim.x) {
    int v[8];
    exp_load8(E, tile, v);
    uint2 s = make_uint2(0, 0);
    for (int k = 0; k < 8; k++) { s.x += v[k] > 0; s.y += (unsigned)v[k]; }
    for (int o = 32; o > 0; o >>= 1) { s.x += __shfl_xor(s.x, o); s.y += __shfl_xor(s.y, o); }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
      E.tile[tile] = make_uint2(red[0].x + red[1].x + red[2].x + red[3].x, red[0].y + red[1].y + red[2].y + red[3].y);
  }
}

__global__ __launch_bounds__(EXP_SCAN_WG) void tracks_export_scan_kernel(ExpArgs E)
{
  __shared__ uint2 red[EXP_SCAN_WG / 64];
  __shared__ int dropped_by_wave[EXP_SCAN_WG / 64];
  const TrkArgs &A = E.T;
  uint2 carry = make_uint2(0, 0);
  for (int t0 = 0; t0 < E.ntiles; t0 += EXP_SCAN_WG) {
    const int t = t0 + threadIdx.x;
    const uint2 v = t < E.ntiles ? E.tile[t] : make_uint2(0, 0);
    uint2 total;
    const uint2 ex = exp_block_scan<EXP_SCAN_WG / 64>(v, red, total);
    if (t < E.ntiles) E.tile[t] = make_uint2(carry.x + ex.x, carry.y + ex.y);
    carry.x += total.x; carry.y += total.y;
  }
  int dropped = 0;
  for (int f = threadIdx.x; f < A.nframes; f += EXP_SCAN_WG) {
    int base, n;
    dropped += !trk_frame(A, f, base, n);
  }
  for (int o = 32; o > 0; o >>= 1) dropped += __shfl_xor(dropped, o);
  if ((threadIdx.x & 63) == 0) dropped_by_wave[threadIdx.x >> 6] = dropped;
  __syncthreads();
  if (threadIdx.x == 0) {
    dropped = 0;
    for (int w = 0; w < EXP_SCAN_WG / 64; w++) dropped += dropped_by_wave[w];
    A.summary[0] = (int)carry.x;
    A.summary[1] = (int)carry.y;
    A.summary[2] = A.summary[3] = A.summary[4] = 0;
    A.summary[5] = dropped;
    A.summary[6] = A.summary[7] = 0;
    E.track_offsets[0] = 0;
  }
}

__global__ __launch_bounds__(256) void tracks_export_apply_kernel(ExpArgs E)
{
  __shared__ uint2 red[4];
  __shared__ int stat[4][3];
  int tracks = 0, obs = 0, longest = 0;
  for (int tile = blockIdx.x; tile < E.ntiles; tile += gridDim.x) {
    int v[8];
    exp_load8(E, tile, v);
    uint2 mine = make_uint2(0, 0);
    for (int k = 0; k < 8; k++) { mine.x += v[k] > 0; mine.y += (unsigned)v[k]; }
    uint2 total;
    uint2 ex = exp_block_scan<4>(mine, red, total);
    const uint2 before = E.tile[tile];
    ex.x += before.x; ex.y += before.y;
    const long long i0 = (long long)tile * EXP_TILE + threadIdx.x * 8;
    for (int k = 0; k < 8; k++) {
      if (i0 + k >= E.T.max_records) break;
      const int len = v[k];
      int at = -1;
      if (len > 0) {
        const int t = (int)ex.x, off = (int)ex.y;
        if (t >= 0 && t < E.max_tracks && off >= 0 && (long long)off + len <= (long long)E.cap) {
          at = off;
          E.track_root[t] = (int)(i0 + k);
          E.track_offsets[t + 1] = off + len;
          tracks++;
          obs += len;
          longest = max(longest, len);
        }
        ex.x += 1; ex.y += (unsigned)len;
      }
      E.place[i0 + k] = at;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    tracks += __shfl_xor(tracks, o);
    obs += __shfl_xor(obs, o);
    longest = max(longest, __shfl_xor(longest, o));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { stat[wave][0] = tracks; stat[wave][1] = obs; stat[wave][2] = longest; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) {
      tracks += stat[w][0]; obs += stat[w][1];
      longest = max(longest, stat[w][2]);
    }
    if (tracks) atomicAdd(E.T.summary + 2, tracks);
    if (obs) atomicAdd(E.T.summary + 3, obs);
    if (longest) atomicMax(E.T.summary + 4, longest);
  }
}

// The offset of the written track record g belongs to and its length, or -1: its label is no index, or its root is not
// written.
__device__ __forceinline__ int exp_segment(const ExpArgs &E, int g, int &root, int &len)
{
  root = E.T.track[g];
  if (root < 0 || root >= E.T.max_records) return -1;
  const int at = E.place[root];
  len = at >= 0 ? E.sel[root] : 0;          // place[root] >= 0 only where apply saw sel[root] = len in [1, max_records]
  return at;
}

__global__ __launch_bounds__(256) void tracks_export_place_kernel(ExpArgs E)
{
  const TrkArgs &A = E.T;
  for (int f = blockIdx.y; f < A.nframes; f += gridDim.y) {
    int base, n;
    if (!trk_frame(A, f, base, n)) continue;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
      const int g = base + r;
      int root, len;
      const int at = exp_segment(E, g, root, len);
      if (at < 0) continue;
      const int k = atomicAdd(E.cursor + root, 1);
      if (k >= 0 && k < len) E.members[at + k] = g;              // at + len <= cap, by the apply launch
    }
  }
}

__global__ __launch_bounds__(256) void tracks_export_write_kernel(ExpArgs E)
{
  const TrkArgs &A = E.T;
  for (int f = blockIdx.y; f < A.nframes; f += gridDim.y) {
    int base, n;
    if (!trk_frame(A, f, base, n)) continue;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
      const int g = base + r;
      int root, len;
      const int at = exp_segment(E, g, root, len);
      int slot = -1;
      if (at >= 0) {
        const int placed = min(max(E.cursor[root], 0), len);     // == len for arrays the linker wrote
        int rank = 0;
        for (int k = 0; k < placed; k++) rank += E.members[at + k] < g;
        if (rank < len) slot = at + rank;
      }
      if (slot >= 0) {
        const SiftPointD &rec = A.set.recs[g];
        E.obs[slot] = make_int4(f, r, __float_as_int(rec.xpos), __float_as_int(rec.ypos));
      }
      if (E.record_obs) E.record_obs[g] = slot;
    }
  }
}

}  // namespace

// Enqueue misift_link_tracks_batch on the context stream (common.hpp): one memset, five launches.
int launch_link_tracks_batch(misift_ctx *ctx, int npairs, const int *h_pairs, const void *d_rows,
                             const int *d_row_counts, int max_pts, const BatchLayout &set, int nframes, int max_records,
                             float min_score, float max_ambiguity, float max_error, int *d_track, int *d_track_len,
                             int *d_track_frames, int *d_summary)
{
  const size_t parent_bytes = trk_align16(sizeof(int) * (size_t)max_records);
  const size_t pinfo_bytes = trk_align16(sizeof(TrkPair) * (size_t)npairs);
  const size_t table_bytes = sizeof(unsigned long long) * 2 * (size_t)max_records;
  int rc = misift_ensure_tmp(ctx, parent_bytes + pinfo_bytes + table_bytes);
  if (rc) return rc;
  TrkArgs A;
  A.set = set; A.nframes = nframes; A.max_records = max_records;
  A.pairs = h_pairs; A.npairs = npairs; A.max_pts = max_pts;
  A.rows = reinterpret_cast<const SiftPointD *>(d_rows);
  A.row_counts = d_row_counts;
  A.min_score = min_score; A.max_ambiguity = max_ambiguity; A.max_error = max_error;
  A.use_error = max_error < __builtin_huge_valf();                // +inf: match_error is not read
  char *t = reinterpret_cast<char *>(ctx->d_match_tmp);
  A.parent = reinterpret_cast<int *>(t);
  A.pinfo = reinterpret_cast<TrkPair *>(t + parent_bytes);
  A.table = reinterpret_cast<unsigned long long *>(t + parent_bytes + pinfo_bytes);
  A.table_slots = 2u * (unsigned)max_records;
  A.track = d_track; A.len = d_track_len; A.frames = d_track_frames; A.summary = d_summary;
  HIP_TRY(hipMemsetAsync(A.table, 0xFF, table_bytes, ctx->stream));
  // the counts live on the device: enough workgroups per frame to cover a large frame in a few strides
  const int ncu = ctx->num_cus > 0 ? ctx->num_cus : 256;
  const int gy = nframes < 1 ? 1 : (nframes < 65535 ? nframes : 65535);
  int gx = 8 * ncu / gy;
  gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
  const dim3 fgrid(gx, gy);
  {
    LaunchScope ls(ctx, "tracks_init");
    hipLaunchKernelGGL(tracks_init_kernel, fgrid, dim3(256), 0, ctx->stream, A);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    const long long need = ((long long)npairs * max_pts + 255) / 256;
    const long long cap = 16LL * ncu;
    const int grid = (int)(need < 1 ? 1 : (need < cap ? need : cap));
    LaunchScope ls(ctx, "tracks_hook");
    hipLaunchKernelGGL(tracks_hook_kernel, dim3(grid), dim3(256), 0, ctx->stream, A);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, "tracks_label");
    hipLaunchKernelGGL(tracks_label_kernel, fgrid, dim3(256), 0, ctx->stream, A);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, "tracks_frames");
    hipLaunchKernelGGL(tracks_frames_kernel, fgrid, dim3(256), 0, ctx->stream, A);
    rc = ls.finish();
    if (rc) return rc;
  }
  LaunchScope ls(ctx, "tracks_summary");
  hipLaunchKernelGGL(tracks_summary_kernel, fgrid, dim3(256), 0, ctx->stream, A);
  return ls.finish();
}

// Enqueue misift_export_tracks_batch on the context stream (common.hpp): one memset, six launches.
int launch_export_tracks_batch(misift_ctx *ctx, const BatchLayout &set, int nframes, int max_records, const int *d_track,
                               const int *d_track_len, const int *d_track_frames, int min_len, int consistent_only,
                               int max_tracks, int max_obs, int *d_track_offsets, int *d_track_root, void *d_obs,
                               int *d_record_obs, int *d_summary)
{
  const size_t ints_bytes = trk_align16(sizeof(int) * (size_t)max_records);
  const int ntiles = (int)(((long long)max_records + EXP_TILE - 1) / EXP_TILE);
  int rc = misift_ensure_tmp(ctx, 4 * ints_bytes + sizeof(uint2) * (size_t)ntiles);
  if (rc) return rc;
  ExpArgs E;
  E.T = TrkArgs{};
  E.T.set = set; E.T.nframes = nframes; E.T.max_records = max_records;
  E.T.track = const_cast<int *>(d_track); E.T.len = const_cast<int *>(d_track_len);     // read only here
  E.T.frames = const_cast<int *>(d_track_frames);
  E.T.summary = d_summary;
  E.min_len = min_len; E.consistent_only = consistent_only; E.max_tracks = max_tracks; E.max_obs = max_obs;
  E.cap = max_obs < max_records ? max_obs : max_records;
  E.ntiles = ntiles;
  char *t = reinterpret_cast<char *>(ctx->d_match_tmp);
  E.sel = reinterpret_cast<int *>(t);
  E.cursor = reinterpret_cast<int *>(t + ints_bytes);
  E.place = reinterpret_cast<int *>(t + 2 * ints_bytes);
  E.members = reinterpret_cast<int *>(t + 3 * ints_bytes);
  E.tile = reinterpret_cast<uint2 *>(t + 4 * ints_bytes);
  E.track_offsets = d_track_offsets; E.track_root = d_track_root; E.record_obs = d_record_obs;
  E.obs = reinterpret_cast<int4 *>(d_obs);
  HIP_TRY(hipMemsetAsync(E.sel, 0, 2 * ints_bytes, ctx->stream));
  const int ncu = ctx->num_cus > 0 ? ctx->num_cus : 256;
  const int gy = nframes < 1 ? 1 : (nframes < 65535 ? nframes : 65535);
  int gx = 8 * ncu / gy;
  gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
  const dim3 fgrid(gx, gy);                                       // per frame, as the linker's
  const dim3 tgrid(ntiles < 8 * ncu ? ntiles : 8 * ncu);          // per tile of the index space
  {
    LaunchScope ls(ctx, "tracks_export_select");
    hipLaunchKernelGGL(tracks_export_select_kernel, fgrid, dim3(256), 0, ctx->stream, E);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, "tracks_export_reduce");
    hipLaunchKernelGGL(tracks_export_reduce_kernel, tgrid, dim3(256), 0, ctx->stream, E);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, "tracks_export_scan");
    hipLaunchKernelGGL(tracks_export_scan_kernel, dim3(1), dim3(EXP_SCAN_WG), 0, ctx->stream, E);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, "tracks_export_apply");
    hipLaunchKernelGGL(tracks_export_apply_kernel, tgrid, dim3(256), 0, ctx->stream, E);
    rc = ls.finish();
    if (rc) return rc;
  }
  {
    LaunchScope ls(ctx, "tracks_export_place");
    hipLaunchKernelGGL(tracks_export_place_kernel, fgrid, dim3(256), 0, ctx->stream, E);
    rc = ls.finish();
    if (rc) return rc;
  }
  LaunchScope ls(ctx, "tracks_export_write");
  hipLaunchKernelGGL(tracks_export_write_kernel, fgrid, dim3(256), 0, ctx->stream, E);
  return ls.finish();
}

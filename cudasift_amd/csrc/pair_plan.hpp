// pair_plan.hpp — the work list of the batched pair matchers (misift_match_batch, misift_match_batch_i8,
// misift_match_pairs_batch, misift_match_pairs_batch_i8).
//
// pair_plan_kernel (kernels_match.hip), one workgroup, reads the pairs' counts and offsets on the device and writes a
// header and one PairPlan per pair: the pair's shape, its column chunking and the exclusive prefix sums of its work
// items and row blocks.  The work list is implicit: item i belongs to the last pair with item0 <= i (pair_find) and is
// (row block, column chunk) of that pair.  The matchers differ only in their PairShape.  Columns are cut into chunks
// only when the row blocks of the whole call do not reach the shape's target; the cut then leaves fewer than
// 2 * target items, so the partials buffer has a bound the host knows (pair_partial_items).
#pragma once
#include "common.hpp"

struct PairShape {
  int rows;                      // rows per row block
  int tile;                      // columns per tile, the unit of the column chunks
  int round;                     // columns that take part: n2 rounded down to a multiple of this (1: all of them)
  int target;                    // work items one call is cut into when its row blocks are fewer
};

struct PairPlan {
  int n1, n2, off1, off2;        // frame sizes (records, counts < 0 -> 0) and first records
  int ncols, ntiles;             // columns that take part, tiles
  int nrb, nchunks, tpc;         // row blocks, column chunks, tiles per chunk
  int item0, rb0;                // first work item / first row block of the pair (entry npairs: the totals)
  int pad;
};
constexpr int PAIR_HDR_INTS = 4; // plan header: items, chunk count C, row blocks, 0 — then PairPlan[npairs + 1]

__host__ __device__ __forceinline__ void pair_shape(const PairShape &S, int n1, int n2, int &ncols, int &ntiles,
                                                    int &nrb)
{
  if (n1 <= 0 || n2 <= 0) { ncols = 0; ntiles = 0; nrb = 0; return; }     // matching.cu:1095-1096: pair left untouched
  ncols = S.round * (n2 / S.round);
  ntiles = (ncols + S.tile - 1) / S.tile;
  nrb = (n1 + S.rows - 1) / S.rows;
}
// chunks per row block for a call of R row blocks: 1 when they reach the target, else ceil(target / R), so that
// R * C < target + R < 2 * target
__host__ __device__ __forceinline__ int pair_batch_chunks(const PairShape &S, long long R)
{
  const long long t = S.target;
  if (R <= 0 || R >= t) return 1;
  return (int)((t + R - 1) / R);
}
__host__ __device__ __forceinline__ void pair_chunks(int ntiles, int C, int &nchunks, int &tpc)
{
  if (ntiles <= 0 || C <= 1) { nchunks = 1; tpc = ntiles > 0 ? ntiles : 1; return; }
  nchunks = C < ntiles ? C : ntiles;
  tpc = (ntiles + nchunks - 1) / nchunks;
  nchunks = (ntiles + tpc - 1) / tpc;                   // no empty chunk
}
inline int pair_partial_items(const PairShape &S) { return 2 * S.target; }

// the last pair whose prefix value (item0 or rb0) is <= v (pairs without work share their successor's value)
template <bool ROWBLOCKS>
__device__ __forceinline__ int pair_find(const PairPlan *__restrict__ plan, int npairs, int v)
{
  int lo = 0, hi = npairs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((ROWBLOCKS ? plan[mid].rb0 : plan[mid].item0) <= v) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// bytes of the device plan of npairs pairs
size_t pair_plan_bytes(int npairs);
// The head of a batched matcher's launches on the context stream (PairOut, PairRows: common.hpp): the temp buffer
// (misift_ensure_tmp: part_bytes of partials, then the mutual check's npairs x max_pts column keys, returned in *keys,
// else NULL), the plan kernel, profiled as `plan_name`, and the memset of the keys.  h_pairs: pinned host memory the
// kernel reads (the caller keeps it unchanged until the kernel has run); d_plan: pair_plan_bytes(npairs) bytes.
// Pair-indexed calls run the capped plan (pair_plan_capped_kernel): a pair with more than max_pts records on a side
// gets no work and pad = 1; rows.num_matched (may be NULL) starts at 0, or -1 for such a pair.
int launch_pair_head(misift_ctx *ctx, const char *plan_name, const PairShape &S, PairOut mode, size_t part_bytes,
                     int npairs, const int *h_pairs, const BatchLayout &set1, const BatchLayout &set2,
                     const PairRows &rows, void *d_plan, unsigned long long **keys);
// The same plan on the host for pairs of n1[i] x n2[i] records (the test hooks): plan5[5 i ..] = first item, row blocks,
// tiles, chunks, tiles per chunk of pair i.
int pair_plan_host(const PairShape &S, int npairs, const int *n1, const int *n2, int *plan5, int *nitems, int *chunks,
                   int *partial_items_bound);

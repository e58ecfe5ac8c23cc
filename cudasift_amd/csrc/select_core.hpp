// select_core.hpp — the rules of misift_select_pairs_batch (preemptive matching: which frame pairs are worth matching),
// compiled by the kernels (kernels_select.hip) and by the host hook misift_test_select_pairs, so that both sides decide
// by the same code: the key of a record, the order of the chosen records, the vote test of a row, and the order of a
// frame's neighbours.  Integer rules but for the gate, which is the fp32 expression of i8_write_row (kernels_match_i8.hip)
// under the gate of misift_link_tracks_batch; the translation units are built with -ffp-contract=off.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#define SELECT_MAX_TOP 256        // MISIFT_SELECT_MAX_TOP
#define SELECT_MAX_FRAMES 4096    // MISIFT_SELECT_MAX_FRAMES

// Stage 1.  The key of a record: the bit pattern of its scale if scale > 0, else 0.  Positive floats order as their bit
// patterns, a NaN compares false (key 0), +inf is the largest key.
__host__ __device__ inline unsigned select_key(float scale)
{
  unsigned bits;
  memcpy(&bits, &scale, sizeof(bits));
  return scale > 0.0f ? bits : 0u;
}

// (key a, index ia) stands before (key b, index ib): key descending, then index ascending.  The order of the chosen
// records of a frame (stage 1) and, with key = V[f][g] and index = g, of the neighbours of a frame (stage 3).
__host__ __device__ inline bool select_before(unsigned ka, int ia, unsigned kb, int ib)
{
  return ka > kb || (ka == kb && ia < ib);
}

// Stage 2.  A row whose best score is `best` (> 0, at its smallest column m) and whose runner-up is `second`, and which
// is column m's best row, votes iff the row misift_match_pairs_batch_i8 writes for it passes the gate of
// misift_link_tracks_batch: score > min_score and ambiguity < max_ambiguity.
__host__ __device__ inline bool select_vote(int best, int second, float min_score, float max_ambiguity)
{
  const float score = (float)best * 0x1p-16f;                       // exact: best < 2^22
  const float ambiguity = ((float)second * 0x1p-16f) / (score + 1e-6f);
  return score > min_score && ambiguity < max_ambiguity;
}

// Stage 3.  g is a candidate neighbour of f iff g != f and V[f][g] >= min_votes; its key in select_before is V[f][g]
// (>= 1), and 0 for every other g, so that no other g is ever among the first of the order.
__host__ __device__ inline unsigned select_neighbour_key(int f, int g, int votes, int min_votes)
{
  return g != f && votes >= min_votes ? (unsigned)votes : 0u;
}

// localize_core.hpp — the rules of misift_describe_points_batch and of the candidates of misift_localize_frames_batch,
// for host and device: which observation contributes to a point's descriptor, the rounded mean of a byte, which point is
// described, what its record holds, and which match row is a candidate.  The kernels (kernels_localize.hip) and the
// host-only test hooks (misift_test_describe_points, misift_test_localize_candidates) compile these same functions, so
// what a CPU test pins is what the device runs.  The definitions, step by step, are in include/misift.h.
//
// Everything here is integer work, comparisons and bit copies; no floating-point arithmetic.  Every index that comes from
// the caller's arrays (T, O, offsets, frames, records, counts, frame offsets, match) is range-checked before it
// addresses anything.
#pragma once
#include <stdint.h>
#include <string.h>
#include "triangulate_core.hpp"

constexpr int LOC_DESC_BYTES = 128;            // an 8-bit descriptor row
constexpr int LOC_REC_WORDS = 144;             // a 576-byte record in 32-bit words

// what misift_describe_points_batch is given: the scene (cam, cam_pair, intrinsics and nimages of S are not used) and the
// record batch its observations index
struct DescribeIn {
  TrackScene s;
  const signed char *q;                        // 128 bytes per record of the batch
  int nframes;
  const int *counts, *offsets;                 // offsets NULL: frame f starts at record f * stride
  int stride, max_records;
};

struct DescribeOut {
  signed char *scene_q;                        // max_tracks x 128
  uint32_t *scene_recs;                        // max_tracks x 144 words
  int *scene_count, *members, *summary;
};

// Frame f of the batch, f in [0, nframes): n = max(count, 0) and base = its first global record; false when its records
// do not all lie in [0, max_records) (such a frame takes no part).  The rule of misift_link_tracks_batch.
FUND_HD bool loc_frame(const DescribeIn &D, int f, long long &base, int &n)
{
  const int c = D.counts[f];
  n = c > 0 ? c : 0;
  base = D.offsets ? (long long)D.offsets[f] : (long long)f * D.stride;
  return n == 0 || (base >= 0 && base + n <= (long long)D.max_records);
}

// whether an observation CONTRIBUTES; row = its global record, in [0, max_records)
FUND_HD bool loc_contributes(const DescribeIn &D, const TrackObs &ob, long long &row)
{
  row = 0;
  if (!(ob.frame >= 0 && ob.frame < D.nframes)) return false;               // before it addresses anything
  long long base;
  int n;
  if (!loc_frame(D, ob.frame, base, n)) return false;
  if (!(ob.record >= 0 && ob.record < n)) return false;
  row = base + ob.record;
  return true;
}

// the range of track t < T in d_obs, empty for a track that is not VALID
FUND_HD bool loc_track_range(const TrackScene &S, int t, int &off, int &end)
{
  off = S.track_offsets[t];
  end = S.track_offsets[t + 1];
  if (tri_range_ok(off, end, scene_O(S))) return true;
  off = end = 0;
  return false;
}

// the mean of m > 0 bytes whose sum is `sum`, half rounded up: in [0, 127] for bytes in [0, 127]
FUND_HD int loc_mean(long long sum, long long m) { return (int)((2 * sum + m) / (2 * m)); }

FUND_HD uint32_t loc_bits(float v)
{
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}

// whether point t < T is DESCRIBED, given its track is valid and has m contributing observations
FUND_HD bool loc_described(const TrackScene &S, int t, bool valid, int m)
{
  if (!valid || m <= 0 || S.point_status[t] != TRI_OK) return false;
  const float *X = S.points + 4 * (size_t)t;
  return fundamental_finite(X[0]) && fundamental_finite(X[1]) && fundamental_finite(X[2]);
}

// One match row as a candidate of misift_localize_frames_batch: the gate of the homography gather, the point it names
// and the positions.  row: the 144 words of a record.
struct LocCandidate {
  float x, y, X, Y, Z;
  int t;
};
FUND_HD bool loc_candidate(const float *row, int T, const float *points, const int *point_status, float min_score,
                           float max_ambiguity, LocCandidate &c)
{
  if (!(row[6] > min_score && row[7] < max_ambiguity)) return false;        // score, ambiguity: a NaN fails
  int t;
  memcpy(&t, row + 8, 4);                                                   // match
  if (!(t >= 0 && t < T)) return false;                                     // before it addresses anything
  if (point_status[t] != TRI_OK) return false;
  const float *P = points + 4 * (size_t)t;
  c.x = row[0]; c.y = row[1];
  c.X = P[0]; c.Y = P[1]; c.Z = P[2];
  c.t = t;
  return fundamental_finite(c.X) && fundamental_finite(c.Y) && fundamental_finite(c.Z) && fundamental_finite(c.x) &&
         fundamental_finite(c.y);
}

// misift_describe_points_batch on host arrays, track after track
inline void describe_points_host(const DescribeIn &D, const DescribeOut &out)
{
  const TrackScene &S = D.s;
  const int T = scene_T(S);
  long long described = 0, contributing = 0, idle = 0;
  for (int t = 0; t < T; t++) {
    int off, end;
    const bool valid = loc_track_range(S, t, off, end);
    long long sum[LOC_DESC_BYTES] = {0};
    int m = 0;
    for (int o = off; o < end; o++) {
      long long row;
      if (!loc_contributes(D, S.obs[o], row)) { idle++; continue; }
      const signed char *q = D.q + LOC_DESC_BYTES * row;
      for (int k = 0; k < LOC_DESC_BYTES; k++) sum[k] += q[k];
      m++;
    }
    const bool desc = loc_described(S, t, valid, m);
    signed char *sq = out.scene_q + LOC_DESC_BYTES * (size_t)t;
    for (int k = 0; k < LOC_DESC_BYTES; k++) sq[k] = desc ? (signed char)loc_mean(sum[k], m) : 0;
    uint32_t *rec = out.scene_recs + LOC_REC_WORDS * (size_t)t;
    for (int k = 0; k < LOC_REC_WORDS; k++) rec[k] = 0;
    if (desc) {
      const float *X = S.points + 4 * (size_t)t;
      for (int k = 0; k < 3; k++) rec[k] = loc_bits(X[k]);                  // xpos, ypos, scale
      described++;
      contributing += m;
    }
    out.members[t] = m;
  }
  out.scene_count[0] = T;
  for (int k = 0; k < 8; k++) out.summary[k] = 0;
  out.summary[0] = T;
  out.summary[1] = (int)described;
  out.summary[2] = (int)contributing;
  out.summary[3] = (int)idle;
}

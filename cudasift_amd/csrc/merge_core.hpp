// merge_core.hpp — the rules of misift_merge_scenes_batch, for host and device: the class of a track of scene A, which
// observation is live and its key, which of two elements of a union is kept, the capacity rule, which scene gives an
// image its camera, and what becomes of a slot.  The kernels (kernels_merge.hip) and the host-only test hook
// (misift_test_merge_scenes) compile these same functions, so what a CPU test pins is what the device runs.  The
// definition, rule by rule, is in include/misift.h.
//
// Everything here is integer work and bit copies: no floating-point arithmetic at all.
//
// The two scenes are stated through the track-scene description the track chain shares (TrackScene, scene_T, scene_O,
// scene_track_owns, tri_range_ok: triangulate_core.hpp), with what only this call reads beside it.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "triangulate_core.hpp"

// MISIFT_CAM_MERGED of include/misift.h (which this header does not see on the sanitizer build)
#define MERGE_CAM_MERGED (-4)

enum {
  MERGE_NOT_VALID = -1, MERGE_CONFLICT = -2, MERGE_REJECTED = -3, MERGE_BAD_MAP = -4, MERGE_NOT_LIVE = -5, MERGE_CUT = -6,
  MERGE_ALONE = -8                             // internal: the class word of an ALONE track (a PARTNER's is its B-track)
};

// one input scene: the shared description (intrinsics NULL: the caller lays the merged ones out) and what only the
// merge reads
struct MergeScene {
  TrackScene s;
  const int *point_views;                      // max_tracks
  const int *record_obs;                       // max_records, or NULL
  int max_records, fshift, rshift;
};

struct MergeOut {
  int max_tracks, max_obs, nimages, max_records;
  int *track_offsets;                          // max_tracks + 1
  TrackObs *obs;                               // max_obs
  int *export_summary;                         // 8
  float *points;                               // max_tracks x 4
  int *point_views, *point_status;             // max_tracks
  float *cam;                                  // nimages x 12
  int *cam_pair;                               // nimages
  int *track_map_a;                            // a.max_tracks
  int *obs_map_a, *obs_map_b;                  // a.max_obs, b.max_obs; may be NULL
  int *record_obs;                             // max_records; may be NULL
  int *summary;                                // 8
};

struct MergeIn {
  MergeScene a, b;
  const int *map;                              // a.max_tracks, from misift_correspond_tracks_batch
  const int *accept;                           // a.max_tracks, or NULL
  MergeOut out;
};

// rule 1: the frame of a live observation lies in [0, nimages); checked before the shift is added
FUND_HD bool merge_live(int frame, int nimages) { return frame >= 0 && frame < nimages; }

// rule 1: the key of a live observation.  frame + fshift < nimages_out, so the sum does not overflow and the key is >= 0
FUND_HD long long merge_key(int frame, int fshift, int record)
{
  return (long long)(((unsigned long long)(unsigned)(frame + fshift) << 32) | (unsigned long long)(unsigned)record);
}

// (source, slot) of an element as one word that orders as the pair does: source 0 is scene B, 1 is scene A
FUND_HD unsigned merge_id(int source, int slot) { return ((unsigned)source << 31) | (unsigned)slot; }

// rule 2: a negative class, the B-track of a PARTNER, or MERGE_ALONE.  `accept` may be NULL.
FUND_HD int merge_class(bool valid, int map, int TB, const int *accept, int t)
{
  if (!valid) return MERGE_NOT_VALID;
  if (map == -2) return MERGE_CONFLICT;
  if (map < -2 || map >= TB) return MERGE_BAD_MAP;
  if (map >= 0 && accept && accept[t] == 0) return MERGE_REJECTED;
  return map >= 0 ? map : MERGE_ALONE;
}

// rule 3: element (key, id) loses to element (key2, id2) of the same union
FUND_HD bool merge_loses(long long key, unsigned id, long long key2, unsigned id2) { return key2 == key && id2 < id; }

// rule 4: merged track number tn holding len observations from off on is written
FUND_HD bool merge_written(long long tn, long long off, int len, int max_tracks_out, int max_obs_out)
{
  return tn < max_tracks_out && off + len <= max_obs_out;
}

// rule 5, cameras: 0 when scene B gives image i' its camera (*src = its index there), 1 when scene A does, -1 for neither
FUND_HD int merge_camera_source(const MergeScene &A, const MergeScene &B, int i, int *src)
{
  const long long ib = (long long)i - B.fshift, ia = (long long)i - A.fshift;
  if (ib >= 0 && ib < B.s.nimages && B.s.cam_pair[ib] != POSEGRAPH_UNSET) { *src = (int)ib; return 0; }
  if (ia >= 0 && ia < A.s.nimages && A.s.cam_pair[ia] != POSEGRAPH_UNSET) { *src = (int)ia; return 1; }
  *src = -1;
  return -1;
}

// What the numbering leaves per merged index i (B-track i for i < T_B, A-track i - T_B beyond): the new offset of a
// written track, -1 otherwise; cls[t]: merge_class of A-track t; rank[o] per slot of a live observation of a merged
// track: r = the kept elements of its union with a smaller key, stored as r for a kept element and ~r for a duplicate.
struct MergeTables {
  const int *owner_a, *owner_b;                // per slot, -1 for none
  const int *cls;                              // per A-track
  const int *rank_a, *rank_b;                  // per slot
  const int *newoff;                           // per merged index
};

// rule 5, d_obs_map_a / d_obs_map_b: what becomes of slot o < O of scene S (source 1 = A, 0 = B).  *kept: the slot's
// own bytes go to the returned slot.
FUND_HD int merge_slot_map(const MergeScene &S, int source, const MergeTables &M, int TB, int o, bool *kept)
{
  *kept = false;
  const int t = (source ? M.owner_a : M.owner_b)[o];
  if (t < 0) return MERGE_NOT_VALID;
  long long i = t;
  if (source) {
    const int c = M.cls[t];
    if (c < 0 && c != MERGE_ALONE) return c;
    i = c == MERGE_ALONE ? (long long)TB + t : c;
  }
  const int off = M.newoff[i];
  if (off < 0) return MERGE_CUT;
  if (!merge_live(S.s.obs[o].frame, S.s.nimages)) return MERGE_NOT_LIVE;
  const int v = (source ? M.rank_a : M.rank_b)[o];
  *kept = v >= 0;
  return off + (v >= 0 ? v : ~v);
}

// rule 5, d_record_obs_out: entry g of the merged record index
FUND_HD int merge_record(const MergeScene &A, const MergeScene &B, const MergeTables &M, int TB, int g)
{
  for (int source = 0; source < 2; source++) {
    const MergeScene &S = source ? A : B;
    const long long gs = (long long)g - S.rshift;
    if (gs < 0 || gs >= S.max_records) continue;
    const int o = S.record_obs[gs];
    if (o < 0 || o >= scene_O(S.s)) continue;
    bool kept;
    const int m = merge_slot_map(S, source, M, TB, o, &kept);
    if (m >= 0) return m;
  }
  return -1;
}

// The whole call on host arrays, one track after the other.
inline void merge_scenes_host(const MergeIn &in)
{
  const MergeScene &A = in.a, &B = in.b;
  const MergeOut &Q = in.out;
  const int TA = scene_T(A.s), OA = scene_O(A.s), TB = scene_T(B.s), OB = scene_O(B.s);
  std::vector<int> owner_a(OA, -1), owner_b(OB, -1), cls(TA, 0), rank_a(OA, 0), rank_b(OB, 0);
  for (int t = 0; t < TA; t++) scene_track_owns(A.s, owner_a.data(), t);
  for (int t = 0; t < TB; t++) scene_track_owns(B.s, owner_b.data(), t);
  int sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<std::vector<int>> partners(TB);
  for (int t = 0; t < TA; t++) {
    const bool valid = tri_range_ok(A.s.track_offsets[t], A.s.track_offsets[t + 1], OA);
    cls[t] = merge_class(valid, in.map[t], TB, in.accept, t);
    if (cls[t] >= 0) partners[cls[t]].push_back(t);
    else if (cls[t] != MERGE_ALONE) sum[4]++;
  }
  // the unions: per merged index the kept length (-1: no merged track), the duplicates and the ranks
  const long long ntot = (long long)TB + TA;
  std::vector<int> len(ntot, -1), dup(ntot, 0), newoff(ntot, -1);
  struct Elem { long long key; unsigned id; };
  std::vector<Elem> u;
  const auto gather = [&](const MergeScene &S, int source, const int *owner, int t) {
    const int off = S.s.track_offsets[t], end = S.s.track_offsets[t + 1];
    if (!tri_range_ok(off, end, scene_O(S.s))) return;
    for (int o = off; o < end; o++)
      if (owner[o] == t && merge_live(S.s.obs[o].frame, S.s.nimages))
        u.push_back(Elem{merge_key(S.s.obs[o].frame, S.fshift, S.s.obs[o].record), merge_id(source, o)});
  };
  for (long long i = 0; i < ntot; i++) {
    u.clear();
    if (i < TB) {
      gather(B, 0, owner_b.data(), (int)i);
      for (int t : partners[i]) gather(A, 1, owner_a.data(), t);
    } else {
      const int t = (int)(i - TB);
      if (cls[t] != MERGE_ALONE) continue;
      gather(A, 1, owner_a.data(), t);
    }
    const size_t n = u.size();
    std::vector<char> kept(n, 1);
    for (size_t e = 0; e < n; e++)
      for (size_t j = 0; j < n && kept[e]; j++)
        if (merge_loses(u[e].key, u[e].id, u[j].key, u[j].id)) kept[e] = 0;
    int m = 0;
    for (size_t e = 0; e < n; e++) {
      int r = 0;
      for (size_t j = 0; j < n; j++) r += kept[j] && u[j].key < u[e].key;
      const int slot = (int)(u[e].id & 0x7fffffffu);
      ((u[e].id >> 31) ? rank_a : rank_b)[slot] = kept[e] ? r : ~r;
      m += kept[e];
    }
    len[i] = m;
    dup[i] = (int)n - m;
  }
  // numbering with the capacity rule
  long long tn = 0, off = 0, Tn = 0, On = 0;
  int longest = 0;
  Q.track_offsets[0] = 0;
  for (long long i = 0; i < ntot; i++) {
    if (len[i] < 0) continue;
    const bool written = merge_written(tn, off, len[i], Q.max_tracks, Q.max_obs);
    if (written) {
      newoff[i] = (int)off;
      Q.track_offsets[tn + 1] = (int)(off + len[i]);
      const MergeScene &S = i < TB ? B : A;
      const int t = (int)(i < TB ? i : i - TB);
      memcpy(Q.points + 4 * (size_t)tn, S.s.points + 4 * (size_t)t, 4 * sizeof(float));
      Q.point_views[tn] = S.point_views[t];
      Q.point_status[tn] = S.s.point_status[t];
      Tn = tn + 1;
      On = off + len[i];
      longest = std::max(longest, len[i]);
      sum[5] += dup[i];
      if (i >= TB) sum[3]++;
    } else {
      sum[6]++;
    }
    if (i >= TB) Q.track_map_a[i - TB] = written ? (int)tn : MERGE_CUT;
    tn++;
    off += len[i];
  }
  const MergeTables M{owner_a.data(), owner_b.data(), cls.data(), rank_a.data(), rank_b.data(), newoff.data()};
  for (int t = 0; t < TA; t++) {
    if (cls[t] == MERGE_ALONE) continue;
    const bool written = cls[t] >= 0 && newoff[cls[t]] >= 0;
    Q.track_map_a[t] = cls[t] < 0 ? cls[t] : written ? cls[t] : MERGE_CUT;
    sum[2] += written;
  }
  for (int source = 0; source < 2; source++) {
    const MergeScene &S = source ? A : B;
    int *obs_map = source ? Q.obs_map_a : Q.obs_map_b;
    for (int o = 0; o < (source ? OA : OB); o++) {
      bool kept;
      const int m = merge_slot_map(S, source, M, TB, o, &kept);
      if (obs_map) obs_map[o] = m;
      if (kept) {
        const TrackObs ob = S.s.obs[o];
        Q.obs[m] = TrackObs{ob.frame + S.fshift, ob.record, ob.xpos, ob.ypos};
      }
    }
  }
  if (Q.record_obs)
    for (int g = 0; g < Q.max_records; g++) Q.record_obs[g] = merge_record(A, B, M, TB, g);
  for (int i = 0; i < Q.nimages; i++) {
    int src;
    const int from = merge_camera_source(A, B, i, &src);
    if (from < 0) {
      memset(Q.cam + 12 * (size_t)i, 0, 12 * sizeof(float));
      Q.cam_pair[i] = POSEGRAPH_UNSET;
    } else {
      const MergeScene &S = from ? A : B;
      memcpy(Q.cam + 12 * (size_t)i, S.s.cam + 12 * (size_t)src, 12 * sizeof(float));
      Q.cam_pair[i] = from ? MERGE_CAM_MERGED : S.s.cam_pair[src];
      sum[7] += from;
    }
  }
  long long total = 0;
  for (long long i = 0; i < ntot; i++) total += len[i] > 0 ? len[i] : 0;
  const int es[8] = {(int)tn, (int)total, (int)Tn, (int)On, longest, 0, 0, 0};
  memcpy(Q.export_summary, es, sizeof es);
  sum[0] = (int)Tn;
  sum[1] = (int)On;
  memcpy(Q.summary, sum, sizeof sum);
}

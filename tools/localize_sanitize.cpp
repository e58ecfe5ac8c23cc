// localize_sanitize.cpp — the host side of misift_describe_points_batch and the candidate rule of
// misift_localize_frames_batch under the address and undefined-behaviour sanitizers, on the CPU: localize_core.hpp over a
// few thousand random and hostile scenes and row sets.  Every array is a heap allocation of exactly the stated size, so
// an index that escapes its range check is a reported error.  A stand-alone program; nothing of the GPU is touched.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Icudasift_amd/csrc tools/localize_sanitize.cpp -o build/localize_sanitize && build/localize_sanitize
#include <climits>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>
#include "localize_core.hpp"

namespace {
std::mt19937 rng(12345);
int pick(int lo, int hi) { return (int)(lo + rng() % (unsigned)(hi - lo + 1)); }
// an index that is mostly usable and sometimes hostile
int hostile(int hi)
{
  switch (rng() % 16) {
    case 0: return -1;
    case 1: return hi;
    case 2: return INT_MAX;
    case 3: return INT_MIN;
    case 4: return hi + pick(1, 1000);
    case 5: return -pick(2, 1000);
    default: return hi > 0 ? pick(0, hi - 1) : 0;
  }
}
float hostile_float()
{
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  switch (rng() % 12) {
    case 0: return nan;
    case 1: return inf;
    case 2: return -inf;
    case 3: return 3.4e38f;
    default: return (float)pick(-1000, 1000) / 7.0f;
  }
}
}  // namespace

int main()
{
  long described = 0, contributing = 0, idle = 0, scenes = 0;
  for (int round = 0; round < 3000; round++) {
    const int max_tracks = pick(1, 40), max_obs = pick(1, 300), nframes = pick(0, 6);
    const bool packed = rng() % 2;
    const int max_records = pick(1, 400);
    std::vector<int> offs(max_tracks + 1), status(max_tracks), counts(nframes ? nframes : 1), foffs(nframes ? nframes : 1);
    std::vector<TrackObs> obs(max_obs);
    std::vector<float> points(4 * (size_t)max_tracks);
    std::vector<signed char> q(128 * (size_t)max_records);
    int summary_in[8] = {0};
    const bool wild = round % 3 == 0;
    // T and O from the "device": below, at, beyond and under the capacities, and negative
    summary_in[2] = wild ? hostile(max_tracks + 1) : max_tracks;
    summary_in[3] = wild ? hostile(max_obs + 1) : max_obs;
    int at = 0;
    for (int t = 0; t <= max_tracks; t++) {
      offs[t] = wild && rng() % 8 == 0 ? hostile(max_obs + 1) : at;   // overlapping, descending, beyond O
      at = at + pick(0, 2 * max_obs / max_tracks + 1);
      if (at > max_obs) at = max_obs;
    }
    for (int t = 0; t < max_tracks; t++) {
      status[t] = rng() % 8 == 0 ? pick(1, 4) : 0;
      for (int k = 0; k < 4; k++) points[4 * (size_t)t + k] = hostile_float();
    }
    int base = 0;
    for (int f = 0; f < nframes; f++) {
      counts[f] = rng() % 6 == 0 ? hostile(max_records) : pick(0, max_records / (nframes + 1) + 1);
      foffs[f] = rng() % 6 == 0 ? hostile(max_records) : base;
      if (counts[f] > 0 && base < INT_MAX - counts[f]) base += counts[f];
    }
    const int stride = packed ? -1 : (rng() % 6 == 0 ? INT_MAX : pick(0, max_records / (nframes + 1) + 1));
    for (TrackObs &o : obs) {
      o.frame = hostile(nframes);
      o.record = hostile(max_records / (nframes + 1) + 1);
      o.xpos = hostile_float();
      o.ypos = hostile_float();
    }
    for (signed char &b : q) b = (signed char)(round % 5 == 0 ? 127 : pick(0, 127));
    DescribeIn in;
    in.s = TrackScene{max_tracks, max_obs, 0, offs.data(), obs.data(), summary_in, points.data(), status.data(),
                      nullptr, nullptr, nullptr};
    in.q = q.data();
    in.nframes = nframes;
    in.counts = counts.data();
    in.offsets = packed ? foffs.data() : nullptr;
    in.stride = stride;
    in.max_records = max_records;
    std::vector<signed char> scene_q(128 * (size_t)max_tracks, 0x5a);
    std::vector<uint32_t> recs(LOC_REC_WORDS * (size_t)max_tracks, 0x5a5a5a5au);
    std::vector<int> members(max_tracks, 0x5a5a5a5a);
    int scene_count = -77, summary[8];
    describe_points_host(in, DescribeOut{scene_q.data(), recs.data(), &scene_count, members.data(), summary});
    const int T = scene_T(in.s);
    if (scene_count != T || summary[0] != T) return 1;
    long desc = 0, contrib = 0;
    for (int t = 0; t < max_tracks; t++) {
      const bool untouched = t >= T;
      bool zero = true;
      for (int k = 0; k < 128; k++) {
        const signed char b = scene_q[128 * (size_t)t + k];
        if (untouched ? b != 0x5a : b < 0) return 2;             // the mean of bytes in [0, 127] lies there too
        zero = zero && b == 0;
      }
      if (untouched ? members[t] != 0x5a5a5a5a : members[t] < 0) return 3;
      const uint32_t *r = recs.data() + LOC_REC_WORDS * (size_t)t;
      for (int k = 3; k < LOC_REC_WORDS; k++)
        if (r[k] != (untouched ? 0x5a5a5a5au : 0u)) return 4;
      if (!untouched && (r[0] || r[1] || r[2] || !zero)) {       // described: status 0, finite, members
        if (status[t] != 0 || members[t] <= 0) return 5;
        for (int k = 0; k < 3; k++)
          if (!fundamental_finite(points[4 * (size_t)t + k]) || r[k] != loc_bits(points[4 * (size_t)t + k])) return 6;
        desc++;
        contrib += members[t];
      }
    }
    // a described point may be all zero with zero coordinates; the summary counts it, so it can only be larger
    if (summary[1] < desc || summary[2] < contrib || summary[3] < 0) return 7;
    described += summary[1]; contributing += summary[2]; idle += summary[3];
    scenes++;
  }

  // the candidate rule over hostile rows
  long rows_seen = 0, cands = 0;
  for (int round = 0; round < 2000; round++) {
    const int T = pick(0, 50), nrows = pick(0, 64);
    std::vector<float> points(4 * (size_t)(T ? T : 1));
    std::vector<int> status(T ? T : 1);
    for (int t = 0; t < T; t++) {
      status[t] = rng() % 6 == 0 ? pick(1, 4) : 0;
      for (int k = 0; k < 4; k++) points[4 * (size_t)t + k] = hostile_float();
    }
    std::vector<float> rows(LOC_REC_WORDS * (size_t)(nrows ? nrows : 1), 0.0f);
    for (int i = 0; i < nrows; i++) {
      float *r = rows.data() + LOC_REC_WORDS * (size_t)i;
      r[0] = hostile_float(); r[1] = hostile_float();
      r[6] = rng() % 4 == 0 ? hostile_float() : 0.99f;
      r[7] = rng() % 4 == 0 ? hostile_float() : 0.5f;
      const int m = hostile(T);
      memcpy(r + 8, &m, 4);
      LocCandidate c;
      const bool ok = loc_candidate(r, T, points.data(), status.data(), 0.85f, 0.95f, c);
      rows_seen++;
      if (!ok) continue;
      cands++;
      if (m < 0 || m >= T || c.t != m || status[m] != 0) return 8;
      if (!(r[6] > 0.85f) || !(r[7] < 0.95f)) return 9;
      const float v[5] = {c.x, c.y, c.X, c.Y, c.Z};
      for (float f : v)
        if (!fundamental_finite(f)) return 10;
    }
  }
  // the mean: every sum of up to 301 bytes, by the definition
  for (int m = 1; m <= 301; m += (m < 9 ? 1 : 73))
    for (long long s = 0; s <= 127LL * m; s++) {
      const int got = loc_mean(s, m);
      if (got < 0 || got > 127 || 2 * m * (long long)got > 2 * s + m || 2 * m * (long long)(got + 1) <= 2 * s + m) return 11;
    }
  if (loc_mean(127LL * INT_MAX, INT_MAX) != 127) return 12;      // the largest track there can be
  printf("localize_sanitize: %ld scenes (%ld described points, %ld contributing and %ld other observations), "
         "%ld rows (%ld candidates): clean\n", scenes, described, contributing, idle, rows_seen, cands);
  return 0;
}

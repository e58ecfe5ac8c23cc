// merge_sanitize.cpp — the host side of misift_merge_scenes_batch under the address and undefined-behaviour sanitizers, on
// the CPU: merge_core.hpp over hostile offsets, counts, frames, records, map and accept values, record indices, shifts
// and capacities, every array allocated at exactly its stated size.  A stand-alone program; nothing of the GPU is touched.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Icudasift_amd/csrc tools/merge_sanitize.cpp -o build/merge_sanitize && build/merge_sanitize
#include <cstdio>
#include <limits>
#include <vector>
#include "merge_core.hpp"

namespace {

const int LO = std::numeric_limits<int>::min(), HI = std::numeric_limits<int>::max();

struct Rng {
  unsigned long long s;
  unsigned next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); }
  int below(int n) { return (int)(next() % (unsigned)n); }
  // a value that is mostly in [0, n) and sometimes hostile
  int hostile(int n)
  {
    const int picks[] = {LO, HI, -1, -2, -3, n, n + 1, 0};
    return below(8) == 0 ? picks[below(8)] : below(n > 0 ? n : 1);
  }
};

struct Scene {
  int mt, mo, n, mr;
  std::vector<int> off, summary, views, status, pair, rec;
  std::vector<TrackObs> obs;
  std::vector<float> points, cam;
  MergeScene view(int fshift, int rshift, bool records) const
  {
    const TrackScene s{mt, mo, n, off.data(), obs.data(), summary.data(), points.data(), status.data(), cam.data(),
                       pair.data(), nullptr};
    return MergeScene{s, views.data(), records ? rec.data() : nullptr, mr, fshift, rshift};
  }
};

Scene make_scene(Rng &g, int mt, int mo, int n, int mr, bool hostile)
{
  Scene S{mt, mo, n, mr, {}, {}, {}, {}, {}, {}, {}, {}, {}};
  S.off.resize(mt + 1);
  int at = 0;
  for (int t = 0; t <= mt; t++) {
    S.off[t] = hostile && g.below(9) == 0 ? g.hostile(mo) : at;
    at += g.below(5);
    if (at > mo) at = mo;
  }
  const int T = hostile ? g.hostile(mt + 1) : g.below(mt + 1), O = hostile ? g.hostile(mo + 1) : S.off[T < 0 ? 0 : T];
  S.summary = {0, 0, T, O, 0, 0, 0, 0};
  S.obs.resize(mo);
  for (auto &o : S.obs) o = TrackObs{hostile ? g.hostile(n) : g.below(n), hostile ? g.hostile(6) : g.below(6), 1.5f, -2.5f};
  S.points.assign(4 * (size_t)mt, 0.25f);
  S.views.assign(mt, 3);
  S.status.assign(mt, 0);
  S.cam.assign(12 * (size_t)n, 0.5f);
  S.pair.resize(n);
  for (auto &p : S.pair) p = g.below(4) - 2;
  S.rec.resize(mr);
  for (auto &r : S.rec) r = hostile ? g.hostile(mo) : g.below(mo) - (g.below(3) == 0);
  return S;
}

}  // namespace

int main()
{
  Rng g{12345};
  long runs = 0, written = 0, kept = 0, dropped = 0;
  for (int round = 0; round < 4000; round++) {
    const bool hostile = round % 2 == 1;
    const int mta = 1 + g.below(round % 7 == 0 ? 300 : 12), moa = 1 + g.below(round % 5 == 0 ? 700 : 40);
    const int mtb = 1 + g.below(round % 11 == 0 ? 300 : 12), mob = 1 + g.below(round % 3 == 0 ? 700 : 40);
    const int na = 1 + g.below(6), nb = 1 + g.below(6), fa = g.below(4), fb = g.below(4);
    const int mra = 1 + g.below(50), mrb = 1 + g.below(50), ra = g.below(20), rb = g.below(20);
    const Scene A = make_scene(g, mta, moa, na, mra, hostile), B = make_scene(g, mtb, mob, nb, mrb, hostile);
    std::vector<int> map(mta), accept(mta);
    for (auto &m : map) m = g.below(3) == 0 ? g.hostile(mtb) : g.below(mtb + 1) - 1;
    for (auto &a : accept) a = g.below(3) - 1;
    const int nout = std::max(na + fa, nb + fb) + g.below(2), mro = std::max(mra + ra, mrb + rb) + g.below(2);
    const int mto = 1 + g.below(mta + mtb + 2), moo = 1 + g.below(moa + mob + 2);
    std::vector<int> offs(mto + 1, -77), es(8, -77), views(mto, -77), status(mto, -77), pair(nout, -77), tmap(mta, -77);
    std::vector<int> omap_a(moa, -77), omap_b(mob, -77), rec(mro, -77), sum(8, -77);
    std::vector<TrackObs> obs(moo);
    std::vector<float> points(4 * (size_t)mto), cam(12 * (size_t)nout);
    const bool records = round % 4 != 0;
    MergeIn in{A.view(fa, ra, records), B.view(fb, rb, records), map.data(), round % 3 ? accept.data() : nullptr,
               MergeOut{mto, moo, nout, mro, offs.data(), obs.data(), es.data(), points.data(), views.data(), status.data(),
                        cam.data(), pair.data(), tmap.data(), round % 5 ? omap_a.data() : nullptr,
                        round % 6 ? omap_b.data() : nullptr, records ? rec.data() : nullptr, sum.data()}};
    merge_scenes_host(in);
    // what the call states about its own outputs
    const int Tn = sum[0], On = sum[1];
    if (Tn < 0 || Tn > mto || On < 0 || On > moo || es[2] != Tn || es[3] != On || es[0] < Tn || offs[0] != 0) return 1;
    if (Tn > 0 && offs[Tn] != On) return 2;
    for (int t = 0; t < Tn; t++)
      if (offs[t] > offs[t + 1]) return 3;
    for (int o = 0; o < On; o++)
      if (obs[o].frame < 0 || obs[o].frame >= nout) return 4;
    for (int t = 0; t < scene_T(in.a.s); t++)
      if (tmap[t] < MERGE_CUT || tmap[t] >= Tn) return 5;
    if (records)
      for (int r : rec)
        if (r < -1 || r >= On) return 6;
    if (sum[6] != es[0] - Tn) return 7;
    runs++; written += Tn; kept += On; dropped += sum[4];
  }
  std::printf("merge_sanitize: %ld merges; %ld tracks and %ld observations written, %ld tracks dropped; clean\n", runs,
              written, kept, dropped);
  return 0;
}

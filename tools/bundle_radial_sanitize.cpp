// bundle_radial_sanitize.cpp — the host side of misift_adjust_bundle_radial_batch and misift_undistort_obs_batch under the
// address and undefined-behaviour sanitizers, on the CPU: the rules of bundle_core.hpp through the bodies of the two test
// hooks (bundle_host.hpp) over planted scenes and over hostile offsets, counts, frames, positions, cameras, points,
// groups, flags and coefficients, every array allocated at exactly its stated size.  A stand-alone program; nothing of
// the GPU is touched.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Icudasift_amd/csrc tools/bundle_radial_sanitize.cpp -o build/bundle_radial_sanitize && build/bundle_radial_sanitize
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "bundle_host.hpp"

namespace {

const int LO = std::numeric_limits<int>::min(), HI = std::numeric_limits<int>::max();
const float FINF = std::numeric_limits<float>::infinity(), FNAN = std::numeric_limits<float>::quiet_NaN();

struct Rng {
  unsigned long long s;
  unsigned next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); }
  int below(int n) { return (int)(next() % (unsigned)n); }
  float unit() { return (float)(next() & 0xffffff) / 16777216.0f; }
  float sym(float a) { return a * (2.0f * unit() - 1.0f); }
  // a value that is mostly in [0, n) and sometimes hostile
  int hostile(int n)
  {
    const int picks[] = {LO, HI, -1, -2, -3, n, n + 1, 0};
    return below(8) == 0 ? picks[below(8)] : below(n > 0 ? n : 1);
  }
  float hostile_float(float v)
  {
    const float picks[] = {FNAN, FINF, -FINF, 1e20f, -1e20f, 0.0f, -0.0f, 3e38f};
    return below(16) == 0 ? picks[below(8)] : v;
  }
};

struct Scene {
  int mt, mo, n, G;
  std::vector<int> off, summary, status, pair, hold, group, radial;
  std::vector<TrackObs> obs;
  std::vector<float> points, cam, K, k0;
};

// cameras along the x axis looking down z, points in front of them, tracks of 2 to 4 neighbouring images, the positions
// displaced by a planted lens; hostile: any of it may be replaced by a hostile value
Scene make_scene(Rng &g, int ntracks, int n, int G, bool hostile)
{
  Scene S;
  S.n = n; S.G = G; S.mt = ntracks + g.below(3) + 1;
  for (int i = 0; i < n; i++) {
    const float c[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, -0.3f * (float)i + g.sym(0.01f), g.sym(0.01f), g.sym(0.01f)};
    for (float v : c) S.cam.push_back(hostile ? g.hostile_float(v) : v);
    const float k[4] = {500.0f, 510.0f, 320.0f, 240.0f};
    for (float v : k) S.K.push_back(v);
    S.pair.push_back(i == 0 ? POSEGRAPH_ROOT : hostile && g.below(9) == 0 ? POSEGRAPH_UNSET : i - 1);
    S.group.push_back(G > 0 ? g.below(G + 1) - 1 : -1);
  }
  if (n > 1) S.hold.push_back(1);
  for (int j = 0; j < G; j++) {
    S.radial.push_back(g.below(3) != 0);
    S.k0.push_back(g.below(3) == 0 ? g.sym(0.2f) : 0.0f);
  }
  S.off.push_back(0);
  for (int t = 0; t < ntracks; t++) {
    const float X[3] = {g.sym(1.0f) + 0.15f * (float)n, g.sym(0.8f), 4.0f + g.unit()};
    const int len = 2 + g.below(3), first = g.below(n > len ? n - len + 1 : 1);
    for (int v = 0; v < len && first + v < n; v++) {
      const int i = first + v;
      const float xc = X[0] - 0.3f * (float)i, u = 500.0f * xc / X[2] + 320.0f, w = 510.0f * X[1] / X[2] + 240.0f;
      const float dx = u - 320.0f, dy = w - 240.0f, r2 = (dx / 500.0f) * (dx / 500.0f) + (dy / 510.0f) * (dy / 510.0f);
      TrackObs ob{i, t, u - dx * 0.1f * r2 + g.sym(0.5f), w - dy * 0.1f * r2 + g.sym(0.5f)};
      if (hostile) {
        ob.frame = g.below(7) == 0 ? g.hostile(n) : ob.frame;
        ob.xpos = g.hostile_float(ob.xpos);
        ob.ypos = g.hostile_float(ob.ypos);
      }
      S.obs.push_back(ob);
    }
    S.off.push_back((int)S.obs.size());
    for (int j = 0; j < 3; j++) S.points.push_back(hostile ? g.hostile_float(X[j] + g.sym(0.05f)) : X[j] + g.sym(0.05f));
    S.points.push_back(0.0f);
    S.status.push_back(hostile ? g.below(5) : 0);
  }
  S.mo = (int)S.obs.size() + g.below(3) + 1;
  const int T = ntracks, O = (int)S.obs.size();
  S.obs.resize(S.mo, TrackObs{0, 0, 0.0f, 0.0f});
  while ((int)S.off.size() < S.mt + 1) S.off.push_back(O);
  S.points.resize(4 * (size_t)S.mt, 0.0f);
  S.status.resize(S.mt, 0);
  if (hostile)
    for (auto &o : S.off) o = g.below(9) == 0 ? g.hostile(S.mo + 1) : o;
  S.summary = {0, 0, hostile ? g.hostile(S.mt + 1) : T, hostile ? g.hostile(S.mo + 1) : O, 0, 0, 0, 0};
  return S;
}

int run(Rng &g, const Scene &S, int loss, int num_loops, int cg_iters, float max_error, bool lists)
{
  std::vector<float> cam_out(12 * (size_t)S.n), points_out(4 * (size_t)S.mt), cam_rms(2 * (size_t)S.n),
      history(4 * (size_t)(num_loops > 0 ? num_loops : 1)), cost(2), weight(S.mo), kout(4 * (size_t)S.n);
  std::vector<int> cam_obs(S.n), cam_status(S.n), point_obs(S.mt), summary(8), focal(3 * (size_t)(S.G > 0 ? S.G : 1)),
      radial(3 * (size_t)(S.G > 0 ? S.G : 1));
  const bool weights = g.below(2), grouped = S.G > 0;
  BundleCall c{};
  c.max_tracks = S.mt; c.max_obs = S.mo; c.track_offsets = S.off.data(); c.obs = S.obs.data();
  c.export_summary = S.summary.data(); c.points = S.points.data(); c.point_status = S.status.data();
  c.nimages = S.n; c.cam = S.cam.data(); c.cam_pair = S.pair.data(); c.intrinsics = S.K.data();
  c.nhold = (int)S.hold.size(); c.hold = S.hold.data(); c.min_views = 2; c.min_obs = 3; c.num_loops = num_loops;
  c.cg_iters = cg_iters; c.max_error = max_error; c.lambda0 = 1e-3f; c.orthonormalise = g.below(2); c.loss = loss;
  c.loss_scale = 2.0f; c.ngroups = S.G; c.group = grouped ? S.group.data() : nullptr; c.radial_call = true;
  c.radial = lists && grouped ? S.radial.data() : nullptr; c.k0 = lists && grouped ? S.k0.data() : nullptr;
  c.cam_out = cam_out.data(); c.points_out = points_out.data(); c.cam_obs = cam_obs.data();
  c.cam_status = cam_status.data(); c.cam_rms = cam_rms.data(); c.point_obs = point_obs.data();
  c.history = history.data(); c.cost = cost.data(); c.obs_weight = weights ? weight.data() : nullptr;
  c.summary = summary.data(); c.intrinsics_out = kout.data(); c.focal_out = focal.data(); c.radial_out = radial.data();
  const bool ok = bundle_host(c);
  if (!ok) return 0;
  // the list undistorted under what the call left, out of place and in place
  std::vector<TrackObs> out(S.mo), same(S.obs);
  if (!bundle_host_undistort(S.mo, S.obs.data(), S.summary.data(), S.n, S.K.data(), S.G,
                             S.G > 0 ? S.group.data() : nullptr, radial.data(), out.data()))
    return 0;
  bundle_host_undistort(S.mo, same.data(), S.summary.data(), S.n, S.K.data(), S.G, S.G > 0 ? S.group.data() : nullptr,
                        radial.data(), same.data());
  const int O = scene_clamp(S.summary[3], S.mo);
  for (int o = 0; o < O; o++)
    if (out[o].frame != same[o].frame || out[o].record != same[o].record) return -1;
  return 1 + summary[6];
}

// Step 5 for the coefficients alone, on states no scene of this program reaches: a trial k_g + x_k that overflows (or is
// NaN) must raise BAD and one that is finite must not, a held or dead coefficient is copied whatever x_k holds
bool trial_rule()
{
  int ctl[BUNDLE_CTL] = {0}, fcount[BUNDLE_MAX_GROUPS] = {5, 5, 5, 0, 5, 0, 0, 0};
  int rad[BUNDLE_MAX_GROUPS] = {1, 1, 0, 1, 1, 0, 0, 0};
  float ks[2 * BUNDLE_MAX_GROUPS] = {3e38f, -0.1f, 3e38f, 3e38f, 1.0f}, kvec[5 * BUNDLE_MAX_GROUPS] = {0.0f};
  BundleData D{};
  D.ngroups = 5; D.ctl = ctl; D.fcount = fcount; D.rad = rad; D.ks = ks; D.kvec = kvec;
  float *x = bundle_kvec(D, BUNDLE_X);
  x[0] = 3e38f; x[1] = 0.25f; x[2] = 3e38f; x[3] = 3e38f; x[4] = FNAN;
  const bool want[5] = {true, false, false, false, true};
  for (int g = 0; g < 5; g++) {
    ctl[BUNDLE_BAD] = 0;
    bundle_radial_trial(D, g);
    const float e = ks[BUNDLE_MAX_GROUPS + g];
    if ((ctl[BUNDLE_BAD] != 0) != want[g]) return false;
    if (g == 0 && !std::isinf(e)) return false;
    if (g == 1 && e != -0.1f + 0.25f) return false;
    if ((g == 2 || g == 3) && e != 3e38f) return false;
    if (g == 4 && !std::isnan(e)) return false;
  }
  return true;
}

}  // namespace

int main()
{
  if (!trial_rule()) {
    std::printf("bundle_radial_trial: a trial coefficient was not kept, turned away or copied as the definition says\n");
    return 1;
  }
  Rng g{20240611ull};
  int ran = 0, kept = 0, refused = 0;
  for (int round = 0; round < 160; round++) {
    const bool hostile = round >= 40;
    const int n = 2 + g.below(7), G = g.below(4) == 0 ? 0 : 1 + g.below(n < BUNDLE_MAX_GROUPS ? n : BUNDLE_MAX_GROUPS);
    const Scene S = make_scene(g, g.below(60), n, G, hostile);
    const int r = run(g, S, g.below(3), g.below(4), g.below(6), g.below(3) ? FINF : 50.0f, g.below(5) != 0);
    if (r < 0) {
      std::printf("round %d: undistort in place and out of place disagree\n", round);
      return 1;
    }
    ran++;
    refused += r == 0;
    kept += r > 1;
  }
  // the maximum number of groups, all of them radial
  {
    const Scene S = make_scene(g, 120, 8, BUNDLE_MAX_GROUPS, false);
    kept += run(g, S, 0, 4, 10, FINF, true) > 1;
    ran++;
  }
  std::printf("bundle_radial_sanitize: %d scenes, %d with a kept step, %d refused as invalid\n", ran, kept, refused);
  return kept >= 20 && refused == 0 ? 0 : 1;
}

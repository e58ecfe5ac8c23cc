// align_sanitize.cpp — the host side of misift_align_points_batch, misift_correspond_tracks_batch and
// misift_transform_scene_batch under the address and undefined-behaviour sanitizers, on the CPU: align_core.hpp over
// hostile seeds, coordinates, transforms and offsets, the refit with the 256 slots one after another.  A stand-alone
// program; nothing of the GPU is touched.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Icudasift_amd/csrc tools/align_sanitize.cpp -o build/align_sanitize && build/align_sanitize
#include <cstdio>
#include <limits>
#include <vector>
#include "align_core.hpp"

namespace {
struct Cand {
  const std::vector<float> &a, &b;             // n x 3 each
  void load(int p, float (&x)[3], float (&y)[3]) const
  {
    for (int k = 0; k < 3; k++) { x[k] = a[3 * (size_t)p + k]; y[k] = b[3 * (size_t)p + k]; }
  }
};
}  // namespace

int main()
{
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  // the draw: every seed kind, the smallest n and a large one
  long drawn = 0;
  for (unsigned seed : {0u, 1u, 12345u, 0x7fffffffu, 0xffffffffu})
    for (int n : {3, 4, 5, 1000, 0x7fffffff}) {
      LibcRand<LibcRandArrayRing> g;
      g.seed(seed);
      const FastMod31 fm((uint32_t)n);
      for (int loop = 0; loop < 200; loop++) {
        int p[3];
        align_draw3(g, fm, p);
        for (int k = 0; k < 3; k++)
          if (p[k] < 0 || p[k] >= n) return 1;
        if (p[0] == p[1] || p[0] == p[2] || p[1] == p[2]) return 2;
        drawn++;
      }
    }
  // the solve over hostile triples: every value in every place
  const float vals[] = {0, 1, -1, 4, 0.5f, 1e20f, -1e20f, 1e30f, 1e-40f, 3e38f, -3e38f, 1e-20f, nan, inf, -inf};
  const int nv = sizeof vals / sizeof vals[0];
  int valid = 0, invalid = 0;
  for (int i = 0; i < nv; i++)
    for (int j = 0; j < nv; j++)
      for (int at = 0; at < 18; at++) {
        float a[3][3] = {{1, 2, 3}, {-2, 0.5f, 1}, {0.25f, -3, 2}}, b[3][3] = {{2, 4, 6.5f}, {-4, 1, 2}, {0.5f, -6, 4}};
        (at < 9 ? a : b)[(at % 9) / 3][at % 3] = vals[i];
        (at < 9 ? b : a)[((at + j) % 9) / 3][(at + j) % 3] = vals[j];
        float h[ALIGN_PARAMS];
        const bool ok = align_solve3(a, b, h);
        for (int k = 0; k < ALIGN_PARAMS; k++) {
          unsigned u;
          __builtin_memcpy(&u, &h[k], sizeof u);
          if (ok ? !fundamental_finite(h[k]) : u != 0x7fc00000u) return 3;
        }
        (ok ? valid : invalid)++;
      }
  // the refit over n candidates either side of the slots, hostile ones among them, from good and bad transforms
  static FundamentalHostExec ex;
  long members = 0;
  for (int n : {0, 1, 3, 255, 256, 257, 1025}) {
    std::vector<float> a(3 * (size_t)n), b(3 * (size_t)n);
    for (int p = 0; p < n; p++)
      for (int k = 0; k < 3; k++) {
        a[3 * p + k] = (float)((p * 7 + k * 13) % 29) - 14.0f;
        b[3 * p + k] = 2.0f * a[3 * p + k] + (float)k + ((p % 11 == 0) ? vals[(p + k) % nv] : 0.0f);
      }
    const Cand cand{a, b};
    const float starts[][ALIGN_PARAMS] = {{1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 2, 2},
                                          {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
                                          {nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan},
                                          {1, 0, 0, 0, 1, 0, 0, 0, 1, inf, 0, 0, 3e38f}};
    for (const auto &start : starts)
      for (float thresh2 : {0.0025f, 1.0f, 3e38f, inf})
        for (int loops : {0, 1, 5}) {
          float h[ALIGN_PARAMS], rms;
          for (int k = 0; k < ALIGN_PARAMS; k++) h[k] = start[k];
          int c = -1, kept = -1;
          align_refit(ex, cand, n, thresh2, loops, h, c, kept, rms);
          if (c < 0 || c > n || kept < 0 || kept > loops) return 4;
          members += c;
        }
  }
  // the transforms
  const float sims[][ALIGN_PARAMS] = {{0, -1, 0, 1, 0, 0, 0, 0, 1, 1, 2, 3, 1.5f},
                                      {nan, 0, 0, 0, inf, 0, 0, 0, 1, 3e38f, -3e38f, 0, 3e38f}};
  for (const auto &sim : sims)
    for (int i = 0; i < nv; i++) {
      float cam[12], out[12], Y[3];
      for (int k = 0; k < 12; k++) cam[k] = vals[(i + k) % nv];
      align_transform_camera(sim, cam, out);
      const float X[3] = {vals[i], vals[(i + 1) % nv], vals[(i + 2) % nv]};
      align_transform_point(sim, X, Y);
      for (int k = 0; k < 12; k++) {
        unsigned u;
        __builtin_memcpy(&u, &out[k], sizeof u);
        if ((u & 0x7fffffffu) > 0x7f800000u && u != 0x7fc00000u) return 5;
      }
    }
  // the track of a slot under good and hostile offsets: the answer is verified, nothing outside off[0 .. T] is read
  const int lo = std::numeric_limits<int>::min(), hi = std::numeric_limits<int>::max();
  const std::vector<std::vector<int>> offs = {{0}, {0, 3}, {0, 3, 5, 9, 9, 12}, {0, -3, hi, 2, lo, 7}, {5, 4, 3, 2, 1, 0},
                                              {hi, hi, hi, hi}, {lo, lo, lo}};
  int found = 0;
  for (const auto &off : offs) {
    const int T = (int)off.size() - 1;
    for (int o : {lo, -1, 0, 1, 2, 3, 4, 8, 9, 11, 12, hi}) {
      const int t = align_track_of(off.data(), T, o);
      if (t < -1 || t >= T) return 6;
      if (t >= 0 && !(off[t] <= o && o < off[t + 1])) return 7;
      found += t >= 0;
    }
  }
  std::printf("align_sanitize: %ld draws; solves valid %d invalid %d; %ld members; %d slots placed; clean\n", drawn, valid,
              invalid, members, found);
  return 0;
}

// pose_planar_sanitize.cpp — the host side of misift_recover_pose_planar_batch under the address and undefined-behaviour
// sanitizers, on the CPU: pose_planar_core.hpp and the bodies of the two test hooks over hostile homographies,
// intrinsics and records.  A stand-alone program; nothing of the GPU is touched.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Icudasift_amd/csrc tools/pose_planar_sanitize.cpp -o build/pose_planar_sanitize && build/pose_planar_sanitize
#include <cstdio>
#include <limits>
#include <vector>
#include "pose_planar_core.hpp"

int main()
{
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float K[][8] = {{1500, 1500, 960, 540, 1200, 1250, 900, 500}, {1, 1, 0, 0, 1, 1, 0, 0},
                        {1e-30f, 1e30f, -1e20f, 1e20f, 3e38f, 1e-38f, 0, 0}};
  const float Hs[][9] = {{1.02f, 0.01f, -30, -0.02f, 0.98f, 12, 1e-5f, -2e-5f, 1},
                         {0, 0, 0, 0, 0, 0, 0, 0, 0},
                         {1, 0, 0, 0, nan, 0, 0, 0, 1},
                         {1, 0, inf, 0, 1, 0, 0, 0, 1},
                         {3e38f, 3e38f, 3e38f, 3e38f, 3e38f, 3e38f, 3e38f, 3e38f, 3e38f},
                         {-1, 0, 0, 0, 1, 0, 0, 0, 1},
                         {1, 0, 0, 0, 1, 0, 0, 0, 0},
                         {0, 0, 3, 0, 0, 2, 0, 0, 1},
                         {1, 0, 0, 0, 1, 0, 0, 0, 1},
                         {1, 0, 0, 0, 1, 0, 0, 0, 2},
                         {2, 0, 0, 0, 2, 0, 0, 0, 1},
                         {1, 0, 0.5f, 0, 1, 0, 0, 0, 1},
                         {1e-20f, 0, 5e-21f, 0, 1e-20f, 0, 0, 0, 1e-20f},
                         {1e20f, 0, 5e19f, 0, 1e20f, 0, 0, 0, 1e20f},
                         {1, 0, 0, 0, 1, 0, 1, 0, -4}};
  const float vals[] = {0, 1, -1, 4, 0.5f, 960, 540, 1e30f, -1e30f, 1e-40f, 3e38f, nan, inf, -inf};
  const int nv = sizeof vals / sizeof vals[0];
  std::vector<float> xy;
  std::vector<unsigned char> gate;
  for (int i = 0; i < nv; i++)
    for (int j = 0; j < nv; j++) {
      const float row[4] = {vals[i], vals[j], vals[(i + j) % nv], vals[(i * j) % nv]};
      xy.insert(xy.end(), row, row + 4);
      gate.push_back((i + j) % 5 != 0);
    }
  const int n = (int)gate.size();
  std::vector<unsigned char> h_in(n), f_in(n), votes(4 * (size_t)n);
  int models[4] = {0, 0, 0, 0}, counted = 0;
  for (const auto &k8 : K)
    for (const auto &h9 : Hs)
      for (float mb : {0.0f, 0.02f, 10.0f}) {
        float out[84];
        int model = 7;
        planar_hook_decompose(h9, k8, mb, out, &model);
        if (model < -1 || model > 2 || model == 0) return 1;
        models[model + 1]++;
        for (int pass = 0; pass < 2; pass++) {
          int dec[9];
          planar_hook_vote(h9, pass ? Hs[0] : nullptr, out, k8, xy.data(), gate.data(), n, 3.0f, pass ? 1e-3f : 3.0f,
                           0.8f, 4, h_in.data(), f_in.data(), votes.data(), dec);
          for (int i = 0; i < n; i++) counted += h_in[i] + f_in[i] + votes[4 * i] + votes[4 * i + 3];
          if (dec[7] < 0 || dec[7] > 3 || dec[8] < 0 || dec[8] > 3 || (dec[7] < 2) == (dec[8] < 2)) return 4;
        }
        int v4[4] = {counted & 3, 2, 2, counted & 1}, best, alt;
        planar_pick(v4, best, alt);
        if (best < 0 || best > 3 || alt < 0 || alt > 3 || (best < 2) == (alt < 2)) return 2;
        if (planar_candidate(counted, n, true, 3, mb) && counted < 3) return 3;
      }
  std::printf("pose_planar_sanitize: invalid %d, planar %d, rotation %d; %d flags set; clean\n", models[0], models[2],
              models[3], counted);
  return 0;
}

// scan_core.hpp — the prefix-sum helpers of the reduce / scan / apply launches: misift_export_tracks_batch
// (kernels_tracks.hip) numbers its tracks with them, misift_filter_tracks_batch (kernels_filter.hip) its survivors.  A
// pair (count, length) is scanned at once; the sums are unsigned, so they wrap instead of overflowing.  Each file that
// includes this compiles its own copy.
#pragma once
#include "common.hpp"

namespace {

// Inclusive prefix sum over the wavefront.
__device__ __forceinline__ uint2 exp_wave_scan(uint2 v)
{
  const int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned x = __shfl_up(v.x, o), y = __shfl_up(v.y, o);
    if (lane >= o) { v.x += x; v.y += y; }
  }
  return v;
}

// Exclusive prefix sum of v over a workgroup of NW wavefronts; total = the workgroup's sum.  red: NW entries of LDS.
template <int NW>
__device__ __forceinline__ uint2 exp_block_scan(uint2 v, uint2 *red, uint2 &total)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint2 inc = exp_wave_scan(v);
  __syncthreads();                                               // red[] of an earlier round has been read
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  uint2 before = make_uint2(0, 0);
  total = make_uint2(0, 0);
  for (int w = 0; w < NW; w++) {
    const uint2 r = red[w];
    if (w < wave) { before.x += r.x; before.y += r.y; }
    total.x += r.x; total.y += r.y;
  }
  return make_uint2(before.x + inc.x - v.x, before.y + inc.y - v.y);
}

}  // namespace

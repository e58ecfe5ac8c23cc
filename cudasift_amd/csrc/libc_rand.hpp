// libc_rand.hpp — glibc's rand() and FindHomography's sample draw, restated for host and device.
//
// The reference draws the four points of each RANSAC hypothesis with `rand() % numValid` (matching.cu:1041-1053), where
// only the device knows numValid in a batch.  So a batch draws each frame's stream on the device from its own seed,
// exactly as glibc's random_r draws it after srand(seed) (the default TYPE_3 state: 31 words, separation 3):
//   r[0] = seed (0 -> 1);  r[i] = 16807 r[i-1] mod (2^31 - 1), i = 1..30 (Schrage's form as glibc writes it);
//   r[31..33] = r[0..2];   r[i] = r[i-31] + r[i-3] mod 2^32;   the k-th rand() is r[344 + k] >> 1.
// The recurrence needs the last 31 words only, so the state is a ring of 32 words (word i lives in slot i & 31).  Where the
// ring is stored is a parameter: an array on the host (the test hooks misift_test_libc_rand and
// misift_test_homography_samples, misift_test_fundamental_samples), one word per lane of a wavefront on the device
// (homography.hip, kernels_fundamental.hip), so the code a CPU test pins is the code the kernel runs.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LIBC_RAND_HD __host__ __device__ __forceinline__
#else
#define LIBC_RAND_HD inline
#endif

// host storage of the ring
struct LibcRandArrayRing {
  uint32_t w[32];
  LIBC_RAND_HD uint32_t get(uint32_t slot) const { return w[slot]; }
  LIBC_RAND_HD void set(uint32_t slot, uint32_t v) { w[slot] = v; }
};

#if defined(__HIPCC__)
// device storage of the ring: word `slot` is the register of lane `slot` of a wavefront; all 64 lanes run the draw (every
// index is wave-uniform)
struct LibcRandWaveRing {
  uint32_t w;
  __device__ uint32_t get(uint32_t slot) const { return (uint32_t)__builtin_amdgcn_readlane((int)w, (int)slot); }
  __device__ void set(uint32_t slot, uint32_t v) { w = (threadIdx.x & 63) == slot ? v : w; }
};
#endif

template <class Ring>
struct LibcRand {
  Ring ring;
  uint32_t i;                      // index of the next word of the recurrence

  LIBC_RAND_HD void seed(uint32_t s)                      // srand(s): glibc __srandom_r
  {
    int32_t word = (int32_t)(s == 0 ? 1u : s);
    ring.set(0, (uint32_t)word);
    for (uint32_t k = 1; k < 31; k++) {
      const int32_t hi = word / 127773, lo = word % 127773;
      word = 16807 * lo - 2836 * hi;
      if (word < 0) word += 2147483647;
      ring.set(k, (uint32_t)word);
    }
    ring.set(31, ring.get(0));                             // r[31..33] = r[0..2] (slots 31, 0, 1)
    ring.set(0, ring.get(1));
    ring.set(1, ring.get(2));
    i = 34;
    for (int k = 0; k < 310; k++) step();                  // glibc discards 10 x 31 words
  }
  LIBC_RAND_HD uint32_t step()
  {
    const uint32_t v = ring.get((i - 31) & 31) + ring.get((i - 3) & 31);
    ring.set(i & 31, v);
    i++;
    return v;
  }
  LIBC_RAND_HD int next() { return (int)(step() >> 1); }   // rand()
};

// n % d for n < 2^31 and 2 <= d < 2^31 without an integer division: q = floor(n * m / 2^(31 + l)) with l = ceil(log2 d),
// m = ceil(2^(31 + l) / d) < 2^32, which is exact for 31-bit n (Granlund & Montgomery 1994, theorem 4.2).
struct FastMod31 {
  uint32_t d, m, shift;            // shift = l - 1: q = mulhi(n, m) >> shift
  LIBC_RAND_HD explicit FastMod31(uint32_t divisor) : d(divisor)
  {
    uint32_t l = 1;
    while (l < 31 && (1u << l) < divisor) l++;
    m = (uint32_t)((((uint64_t)1 << (31 + l)) + divisor - 1) / divisor);
    shift = l - 1;
  }
  LIBC_RAND_HD uint32_t mod(uint32_t n) const
  {
    const uint32_t q = (uint32_t)(((uint64_t)n * m) >> 32) >> shift;
    return n - q * d;
  }
};

// One hypothesis' four distinct positions in the ordered list of valid points, in the reference's call order
// (matching.cu:1041-1053).  num_valid >= 8.
template <class Ring>
LIBC_RAND_HD void homography_draw4(LibcRand<Ring> &g, const FastMod31 &fm, int (&p)[4])
{
  int p1 = (int)fm.mod((uint32_t)g.next());
  int p2 = (int)fm.mod((uint32_t)g.next());
  int p3 = (int)fm.mod((uint32_t)g.next());
  int p4 = (int)fm.mod((uint32_t)g.next());
  while (p2 == p1) p2 = (int)fm.mod((uint32_t)g.next());
  while (p3 == p1 || p3 == p2) p3 = (int)fm.mod((uint32_t)g.next());
  while (p4 == p1 || p4 == p2 || p4 == p3) p4 = (int)fm.mod((uint32_t)g.next());
  p[0] = p1; p[1] = p2; p[2] = p3; p[3] = p4;
}

// One fundamental-matrix hypothesis' eight distinct positions in the ordered list of valid points: eight draws first,
// then p[1] .. p[7] in turn are redrawn while they repeat an earlier position.  num_valid >= 8.
template <class Ring>
LIBC_RAND_HD void fundamental_draw8(LibcRand<Ring> &g, const FastMod31 &fm, int (&p)[8])
{
  int p0 = (int)fm.mod((uint32_t)g.next()), p1 = (int)fm.mod((uint32_t)g.next());
  int p2 = (int)fm.mod((uint32_t)g.next()), p3 = (int)fm.mod((uint32_t)g.next());
  int p4 = (int)fm.mod((uint32_t)g.next()), p5 = (int)fm.mod((uint32_t)g.next());
  int p6 = (int)fm.mod((uint32_t)g.next()), p7 = (int)fm.mod((uint32_t)g.next());
  while (p1 == p0) p1 = (int)fm.mod((uint32_t)g.next());
  while (p2 == p0 || p2 == p1) p2 = (int)fm.mod((uint32_t)g.next());
  while (p3 == p0 || p3 == p1 || p3 == p2) p3 = (int)fm.mod((uint32_t)g.next());
  while (p4 == p0 || p4 == p1 || p4 == p2 || p4 == p3) p4 = (int)fm.mod((uint32_t)g.next());
  while (p5 == p0 || p5 == p1 || p5 == p2 || p5 == p3 || p5 == p4) p5 = (int)fm.mod((uint32_t)g.next());
  while (p6 == p0 || p6 == p1 || p6 == p2 || p6 == p3 || p6 == p4 || p6 == p5) p6 = (int)fm.mod((uint32_t)g.next());
  while (p7 == p0 || p7 == p1 || p7 == p2 || p7 == p3 || p7 == p4 || p7 == p5 || p7 == p6)
    p7 = (int)fm.mod((uint32_t)g.next());
  p[0] = p0; p[1] = p1; p[2] = p2; p[3] = p3; p[4] = p4; p[5] = p5; p[6] = p6; p[7] = p7;
}

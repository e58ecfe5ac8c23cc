// epipolar_core.hpp — the arithmetic of misift_match_epipolar_batch, for host and device: the epipolar line of a set-1
// row, the exact gate of one set-2 record, and the band around the line that the gather walks.  The kernel
// (kernels_guided.hip) and the host-only test hooks (misift_test_epipolar_gate, _gather) compile these same functions,
// so what a CPU test pins is what the device runs.
//
// Line and gate are fp32 with every operation rounded: only + and *, no fmaf, and the build's -ffp-contract=off keeps
// the compiler from fusing.  The order of every sum is written out; tests restate it in numpy.  The band is double.
//
// Convention: (x2, y2, 1) . F . (x1, y1, 1)^T = 0, F row-major in 9 floats (fundamental_core.hpp).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define EPI_HD __host__ __device__ __forceinline__
#else
#define EPI_HD inline
#endif

// false for NaN and +-inf
EPI_HD bool epipolar_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

// The line of row (x, y) in image 2, a0 x2 + a1 y2 + a2 = 0: the `a` terms of fundamental_sampson, and n2 = |(a0, a1)|^2.
struct EpipolarLine {
  float a0, a1, a2, n2;
};

EPI_HD EpipolarLine epipolar_line(const float *F, float x, float y)
{
  EpipolarLine L;
  L.a0 = F[0] * x + F[1] * y + F[2];
  L.a1 = F[3] * x + F[4] * y + F[5];
  L.a2 = F[6] * x + F[7] * y + F[8];
  L.n2 = L.a0 * L.a0 + L.a1 * L.a1;
  return L;
}

// a row whose line has a non-finite term (an overflowing n2 included) has no candidate
EPI_HD bool epipolar_line_ok(const EpipolarLine &L)
{
  return epipolar_finite(L.a0) && epipolar_finite(L.a1) && epipolar_finite(L.a2) && epipolar_finite(L.n2);
}

// Record (x2, y2) is a candidate of a row with a valid line iff e*e < r2 * n2, r2 = fl(radius * radius): the squared
// distance to the line against radius^2, without the division.  A NaN comparison is false, n2 == 0 admits nothing, a
// right-hand side of +inf admits every finite e*e; a non-finite x2 or y2 makes e*e +inf or NaN, never a candidate.
EPI_HD bool epipolar_gate(const EpipolarLine &L, float x2, float y2, float r2)
{
  const float e = x2 * L.a0 + y2 * L.a1 + L.a2;
  return e * e < r2 * L.n2;
}

// The band |a u + b v + c| <= w in coordinates (u, v) = (x2 - x0, y2 - y0) relative to the corner (x0, y0) of the
// frame's bounding box, in double.  rp = r' = r (1 + 2^-10) + 1e-20 is the disc gather's half-width; X and Y bound |x2|
// and |y2| over the box.  w exceeds what a record that passes the gate can reach (kernels_guided.hip proves it):
//   w = r' (sqrt(a0^2 + a1^2) + 2^-70) + 2^-20 (|a0| X + |a1| Y + |a2|) + 2^-70
struct EpipolarBand {
  double a, b, c, w;
  double ainv, binv;              // 1 / a, 1 / b: +-inf for a zero coefficient (an exactly horizontal / vertical line)
};

EPI_HD EpipolarBand epipolar_band(const EpipolarLine &L, double rp, double x0, double y0, double X, double Y)
{
  EpipolarBand B;
  B.a = (double)L.a0;
  B.b = (double)L.a1;
  B.c = B.a * x0 + B.b * y0 + (double)L.a2;
  const double n = sqrt(B.a * B.a + B.b * B.b);
  B.w = rp * (n + 0x1p-70) + 0x1p-20 * (fabs(B.a) * X + fabs(B.b) * Y + fabs((double)L.a2)) + 0x1p-70;
  B.ainv = 1.0 / B.a;
  B.binv = 1.0 / B.b;
  return B;
}

// The extent [lo, hi] of the band along the axis s whose coefficient is k (kinv = 1 / k), taken over t in [t0, t1] on
// the other axis (coefficient m): the s with |k s + m t + c| <= w for some such t.  -c - m t is linear in t, so its
// extremes lie at t0 and t1; +-w widens them; the division by k maps the interval, swapping its ends when k < 0.
// Returns 0 when no s in [0, smax] qualifies, 1 with [lo, hi] (either end may be +-inf), 2 when an end is a NaN
// (0 * inf: k == 0 with the band's edge exactly on the interval), which the caller takes as "everything".
// k == 0 needs no branch: the products are +-inf by the sign of the numerators, so a band that contains the whole s
// axis gives [-inf, +inf] and one that misses the t interval gives lo = hi = +-inf, outside [0, smax].
EPI_HD int epipolar_extent(double kinv, double m, double c, double w, double t0, double t1, double smax, double &lo,
                           double &hi)
{
  const double b0 = -c - m * t0, b1 = -c - m * t1;
  const double nmin = fmin(b0, b1) - w, nmax = fmax(b0, b1) + w;
  const double p = nmin * kinv, q = nmax * kinv;
  if (p != p || q != q) return 2;
  lo = fmin(p, q);
  hi = fmax(p, q);
  return (hi < 0.0 || lo > smax) ? 0 : 1;
}

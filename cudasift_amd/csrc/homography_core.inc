// homography_core.inc — the two bodies that the single-call kernels (misift_find_homography,
// misift_improve_homography) and the batch kernels (misift_find_homography_batch, misift_improve_homography_batch) of
// homography.hip share as text: the hypothesis solve and the improve rounds.  Each inclusion defines exactly one of the
// HOMO_CORE_* macros and gets that fragment, in place, inside a kernel body, with the variable names the fragment's
// comment lists.  Everything else the kernels share is a function: the gather and the pick in ransac_batch.hpp, the
// inlier test in homography.hip.
//
// Textual rather than inline functions: written as __forceinline__ functions, these two compiled into a different
// instruction stream (homo_solve_kernel 127 -> 90 VGPRs, 272 -> 560 bytes of scratch); with the fragments their
// disassembly is unchanged.

#if defined(HOMO_CORE_SOLVE)
// Hypothesis idx (one lane): the 4 points valid[sample[k * num_loops + idx]], A h = b by the 8x8 Crout LU (lu8) and the
// inverse (lu8_unit_solve), h -> homo[r * num_loops + idx].  Expects coord, stride, valid, sample, num_loops, idx, homo.
  float m[8][8], inv[8][8], rhs[8], x[8];
  int perm[8];
  for (int i = 0; i < 4; i++) {
    const int pt = valid[sample[i * num_loops + idx]];
    const float x1 = coord[0 * stride + pt], y1 = coord[1 * stride + pt];
    const float x2 = coord[2 * stride + pt], y2 = coord[3 * stride + pt];
    float *r1 = m[2 * i], *r2 = m[2 * i + 1];
    r1[0] = x1; r1[1] = y1; r1[2] = 1.0f; r1[3] = 0.0f; r1[4] = 0.0f; r1[5] = 0.0f;
    r1[6] = -x2 * x1; r1[7] = -x2 * y1;
    r2[0] = 0.0f; r2[1] = 0.0f; r2[2] = 0.0f; r2[3] = x1; r2[4] = y1; r2[5] = 1.0f;
    r2[6] = -y2 * x1; r2[7] = -y2 * y1;
    rhs[2 * i] = x2;
    rhs[2 * i + 1] = y2;
  }
  lu8(m, perm);
  for (int c = 0; c < 8; c++) {
    lu8_unit_solve(m, perm, c, x);
    for (int r = 0; r < 8; r++) inv[r][c] = x[r];
  }
  for (int r = 0; r < 8; r++) {
    float s = 0.0f;
    for (int k = 0; k < 8; k++) s = fmaf(inv[r][k], rhs[k], s);
    homo[r * num_loops + idx] = s;
  }

#elif defined(HOMO_CORE_IMPROVE)
// One 64-lane workgroup: P.num_loops rounds of ImproveHomography from the start P.a0 over the P.npts records at P.pts,
// then match_error of every record through pts_rw.  Expects P (ImproveArgs), pts_rw; leaves lane, s_A[0..7] (LDS: the
// solution) and numfit (every lane: records within the limit).
  __shared__ double s_M[64], s_X[8], s_A[8];
  const int lane = threadIdx.x;
  // lane -> accumulator: lanes 0..35 = M[r][c] for r <= c (row-major upper triangle), lanes 36..43 = X[r]
  int r = 0, c = 0;
  bool is_m = lane < 36, is_x = lane >= 36 && lane < 44;
  if (is_m) {
    int k = lane;
    for (r = 0; r < 8; r++) {
      const int len = 8 - r;
      if (k < len) { c = r + k; break; }
      k -= len;
    }
  } else if (is_x) {
    r = lane - 36;
  }
  if (lane < 8) s_A[lane] = P.a0[lane];
  __syncthreads();
  for (int loop = 0; loop < P.num_loops; loop++) {
    const double A0 = s_A[0], A1 = s_A[1], A2 = s_A[2], A3 = s_A[3], A4 = s_A[4], A5 = s_A[5], A6 = s_A[6], A7 = s_A[7];
    double acc = 0.0;
    for (int i = 0; i < P.npts; i++) {
      const SiftPointD &pt = P.pts[i];
      const float x = pt.xpos, y = pt.ypos, mx = pt.match_xpos, my = pt.match_ypos;
      if (pt.score < P.min_score || pt.ambiguity > P.max_ambiguity) continue;
      const float den = A6 * x + A7 * y + 1.0f;
      const float dx = (A0 * x + A1 * y + A2) / den - mx;
      const float dy = (A3 * x + A4 * y + A5) / den - my;
      const float err = dx * dx + dy * dy;
      const float wei = (err < P.limit ? 1.0f : 0.0f);
      const double xd = x, yd = y;
      const double p6 = -x * mx, p7 = -y * mx, q6 = -x * my, q7 = -y * my;      // float products, then widened
      // Y1 = (x, y, 1, 0, 0, 0, p6, p7), Y2 = (0, 0, 0, x, y, 1, q6, q7)
      const double y1r = pick8(r, xd, yd, 1.0, 0.0, 0.0, 0.0, p6, p7), y2r = pick8(r, 0.0, 0.0, 0.0, xd, yd, 1.0, q6, q7);
      if (is_m) {
        const double y1c = pick8(c, xd, yd, 1.0, 0.0, 0.0, 0.0, p6, p7), y2c = pick8(c, 0.0, 0.0, 0.0, xd, yd, 1.0, q6, q7);
        acc += (y1c * y1r * wei);
        acc += (y2c * y2r * wei);
      } else if (is_x) {
        acc += y1r * mx * wei;
        acc += y2r * my * wei;
      }
    }
    if (is_m) { s_M[r * 8 + c] = acc; s_M[c * 8 + r] = acc; }
    if (is_x) s_X[r] = acc;
    __syncthreads();
    if (lane == 0) {                                    // cv::solve(M, X, A, DECOMP_CHOLESKY), geomFuncs.cpp:55
      double L[64], B[8];
      for (int k = 0; k < 64; k++) L[k] = s_M[k];
      for (int k = 0; k < 8; k++) B[k] = s_X[k];
      bool ok = true;
      for (int i = 0; i < 8 && ok; i++)
        for (int j = 0; j <= i; j++) {
          double s = L[i * 8 + j];
          for (int k = 0; k < j; k++) s -= L[i * 8 + k] * L[j * 8 + k];
          if (i == j) {
            if (!(s > 0)) { ok = false; break; }
            L[i * 8 + i] = sqrt(s);
          } else {
            L[i * 8 + j] = s / L[j * 8 + j];
          }
        }
      if (ok) {
        for (int i = 0; i < 8; i++) {
          double s = B[i];
          for (int k = 0; k < i; k++) s -= L[i * 8 + k] * B[k];
          B[i] = s / L[i * 8 + i];
        }
        for (int i = 7; i >= 0; i--) {
          double s = B[i];
          for (int k = i + 1; k < 8; k++) s -= L[k * 8 + i] * B[k];
          B[i] = s / L[i * 8 + i];
        }
        for (int k = 0; k < 8; k++) s_A[k] = B[k];
      } else {
        for (int k = 0; k < 8; k++) s_A[k] = 0.0;       // cv::solve zeroes the solution when the factorisation fails
      }
    }
    __syncthreads();
  }
  const double A0 = s_A[0], A1 = s_A[1], A2 = s_A[2], A3 = s_A[3], A4 = s_A[4], A5 = s_A[5], A6 = s_A[6], A7 = s_A[7];
  int numfit = 0;
  for (int i = lane; i < P.npts; i += 64) {
    SiftPointD &pt = pts_rw[i];
    const float x = pt.xpos, y = pt.ypos;
    const float den = A6 * x + A7 * y + 1.0;
    const float dx = (A0 * x + A1 * y + A2) / den - pt.match_xpos;
    const float dy = (A3 * x + A4 * y + A5) / den - pt.match_ypos;
    const float err = dx * dx + dy * dy;
    if (err < P.limit) numfit++;
    pt.match_error = sqrtf(err);
  }
  for (int m = 32; m > 0; m >>= 1) numfit += __shfl_xor(numfit, m, 64);

#else
#error "homography_core.inc: define one HOMO_CORE_* fragment before including"
#endif

// homography_core.inc — the arithmetic FindHomography and ImproveHomography share between the single-call kernels
// (misift_find_homography, misift_improve_homography) and the batch kernels (misift_find_homography_batch,
// misift_improve_homography_batch) in homography.hip.  Each inclusion defines exactly one of the HOMO_CORE_* macros and
// gets that fragment, in place, inside a kernel body.
//
// Textual rather than inline functions: written as __forceinline__ functions, the single-call gather, solve, count and
// improve kernels compiled into a different instruction stream (homo_solve_kernel 127 -> 90 VGPRs, 272 -> 560 bytes of
// scratch); with the fragments their disassembly is unchanged.

#if defined(HOMO_CORE_GATHER)
// One 1024-thread workgroup: SoA coordinates coord[k * stride + i] of the npts records at pts, and the ORDERED list of the
// valid ones (ballot/popcount compaction keeps index order, which the rand() % numValid sampling depends on).  Expects pts,
// npts, stride, min_score, max_ambiguity, coord, valid; leaves tid and base_s (LDS) = the number of valid points.
  __shared__ int wave_cnt[16];
  __shared__ int base_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int i0 = 0; i0 < npts; i0 += 1024) {
    const int i = i0 + tid;
    bool ok = false;
    if (i < npts) {
      const float *p = pts + (size_t)i * PT_WORDS;
      coord[0 * stride + i] = p[OFF_XPOS];
      coord[1 * stride + i] = p[OFF_YPOS];
      coord[2 * stride + i] = p[OFF_MXPOS];
      coord[3 * stride + i] = p[OFF_MYPOS];
      ok = p[OFF_SCORE] > min_score && p[OFF_AMBIG] < max_ambiguity;      // matching.cu:1035
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = base_s;
    for (int w = 0; w < wave; w++) off += wave_cnt[w];
    if (ok) valid[off + __popcll(m & ((1ull << lane) - 1ull))] = i;
    __syncthreads();
    if (tid == 0) {
      int s = 0;
      for (int w = 0; w < 16; w++) s += wave_cnt[w];
      base_s += s;
    }
    __syncthreads();
  }

#elif defined(HOMO_CORE_SOLVE)
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

#elif defined(HOMO_CORE_INLIER)
// The inlier test of TestHomographies (matching.cu:975-990) with its round-toward-zero products.  Expects a[8] (the
// hypothesis), x1, y1, x2, y2 (one stored match), thresh2, cnt; adds 1 to cnt for an inlier.
    const float nomx = mul_rz(a[0], x1) + mul_rz(a[1], y1) + a[2];
    const float nomy = mul_rz(a[3], x1) + mul_rz(a[4], y1) + a[5];
    const float deno = mul_rz(a[6], x1) + mul_rz(a[7], y1) + 1.0f;
    const float errx = mul_rz(x2, deno) - nomx;
    const float erry = mul_rz(y2, deno) - nomy;
    const float err2 = mul_rz(errx, errx) + mul_rz(erry, erry);
    cnt += err2 < mul_rz(thresh2, mul_rz(deno, deno)) ? 1 : 0;

#elif defined(HOMO_CORE_PICK)
// One 1024-thread workgroup: the first hypothesis with the largest count (strict '>' scan of matching.cu:1063-1068).
// Expects counts, num_loops; leaves tid and, in thread 0, best = count in the high word, (INT_MAX - index) in the low word
// (the max key is the largest count at the smallest index).
  __shared__ unsigned long long best_s[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long best = 0;
  for (int i = tid; i < num_loops; i += 1024) {
    const unsigned long long key = ((unsigned long long)(unsigned)counts[i] << 32) | (unsigned)(0x7fffffff - i);
    best = key > best ? key : best;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(best, off, 64);
    best = o > best ? o : best;
  }
  if (lane == 0) best_s[wave] = best;
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < 16; w++) best = best_s[w] > best ? best_s[w] : best;

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

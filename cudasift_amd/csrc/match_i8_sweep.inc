// match_i8_sweep.inc — the tile loop of the int8 matchers (kernels_match_i8.hip), included into match_i8_kernel<MODE>.
// Textual, as match_sweep.inc: the loop keeps its instruction stream whatever the kernel around it adds.
//
// Expects in scope: A (q1, q2), P (the pair's plan, wave-uniform), wave, lane, c, h, row0 (the wave's first row), t0 / t1
// (the item's tiles) and red.  Leaves (M, I, S2) = (best score, frame-local column, second score) of the row the lane
// owns (row0 + own).  I8_COL_KEYS(t, acc0, acc1) is what the includer does with the scores of tile t besides the rows'
// top two: nothing, or the column keys of the mutual check (i8_colkey_tile).
    v4i a[2][4];
#pragma unroll
    for (int ai = 0; ai < 2; ai++) {
      const int row = row0 + 32 * ai + c;
      if (row < P.n1) {
        const v4i *p = reinterpret_cast<const v4i *>(A.q1 + ((size_t)P.off1 + row) * 128 + 64 * h);
#pragma unroll
        for (int s = 0; s < 4; s++) a[ai][s] = p[s];
      } else {
#pragma unroll
        for (int s = 0; s < 4; s++) a[ai][s] = (v4i){0, 0, 0, 0};
      }
    }
    const int8_t *q2 = A.q2 + (size_t)P.off2 * 128 + 64 * h;
    int M = 0, I = -1, S2 = 0;
    for (int w0 = t0; w0 < t1; w0 += I8_WIN) {
      const int w1 = min(w0 + I8_WIN, t1);
      unsigned b1[2][16], b2[2][16];
#pragma unroll
      for (int ai = 0; ai < 2; ai++)
#pragma unroll
        for (int r = 0; r < 16; r++) { b1[ai][r] = 0u; b2[ai][r] = 0u; }
      // set-2 tiles ping-pong between two register sets, each loaded one tile ahead of its use.  Only the pair's last
      // tile can be partial: it runs on its own after the loop, its lanes past the last column zeroed (S = 0 never counts).
      v4i bA[4], bB[4];
      auto load = [&](v4i (&b)[4], int t) {
        const v4i *p = reinterpret_cast<const v4i *>(q2 + (size_t)(t * I8_TILE + c) * 128);
#pragma unroll
        for (int s = 0; s < 4; s++) b[s] = p[s];
      };
      auto tile = [&](v4i (&b)[4], int t) {
        v16i acc0 = {}, acc1 = {};
#pragma unroll
        for (int s = 0; s < 4; s++) {
          acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[0][s], b[s], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[1][s], b[s], acc1, 0, 0, 0);
        }
        const unsigned kc = __builtin_amdgcn_readfirstlane(I8_OFF + (unsigned)(I8_WIN - 1 - (t - w0)));
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const unsigned k0 = ((unsigned)acc0[r] << 9) + kc, k1 = ((unsigned)acc1[r] << 9) + kc;
          b2[0][r] = max(min(b1[0][r], b2[0][r]), min(max(b1[0][r], b2[0][r]), k0));
          b1[0][r] = max(b1[0][r], k0);
          b2[1][r] = max(min(b1[1][r], b2[1][r]), min(max(b1[1][r], b2[1][r]), k1));
          b1[1][r] = max(b1[1][r], k1);
        }
        I8_COL_KEYS(t, acc0, acc1);
      };
      const int wf = min(w1, P.n2 / I8_TILE);             // tiles [w0, wf) are full
      if (w0 < wf) load(bA, w0);
      for (int t = w0; t < wf; t += 2) {           // unconditional loads (the last ones repeat tile wf - 1): static vmcnt
        load(bB, min(t + 1, wf - 1));
        tile(bA, t);
        if (t + 1 >= wf) break;
        load(bA, min(t + 2, wf - 1));
        tile(bB, t + 1);
      }
      if (wf < w1) {
        const bool live = wf * I8_TILE + c < P.n2;
        if (live) load(bA, wf);
        else {
#pragma unroll
          for (int s = 0; s < 4; s++) bA[s] = (v4i){0, 0, 0, 0};
        }
        tile(bA, wf);
      }
      // fold the window: lane (c, h) reads row register c of the 32 lanes of its half
#pragma unroll
      for (int ai = 0; ai < 2; ai++)
#pragma unroll
        for (int r = 0; r < 16; r++) red[wave][16 * ai + r][lane] = make_uint2(b1[ai][r], b2[ai][r]);
      __syncthreads();
      for (int l = 0; l < 32; l++) {
        const uint2 e = red[wave][c][32 * h + l];
        const bool v1 = e.x >= I8_VALID;
        const int s1 = v1 ? (int)((e.x - I8_OFF) >> 9) : 0;
        const int j1 = v1 ? (w0 + I8_WIN - 1 - (int)(e.x & (I8_WIN - 1))) * I8_TILE + l : -1;
        const int s2 = e.y >= I8_VALID ? (int)((e.y - I8_OFF) >> 9) : 0;
        i8_take(M, I, S2, s1, j1, s2);
      }
      __syncthreads();                           // red is rewritten by the next window / item
    }

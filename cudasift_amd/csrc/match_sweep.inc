// match_sweep.inc — the column sweep of one matcher workgroup, included into the body of match_kernel (misift_match,
// misift_match_rows, the sharded matcher) and of match_batch_kernel<MODE> (misift_match_batch, misift_match_pairs_batch)
// in kernels_match.hip.
//
// Textual rather than an inline function: the sweep as a __forceinline__ function compiled into a different instruction
// stream and register allocation of match_kernel (251 -> 256 VGPRs), and match_kernel's code is measured and must not move.
//
// Expects in scope: pts1 (set 1 records), set2 (floats), G (MatchGeom), rb (row block of 128 rows relative to
// G.row_begin, 0 <= rb * 128 < G.row_count), st0 / st1 (virtual super-tiles to sweep), tid, wave, lane, half, col,
// Bs[2][MT_SUPER * MT_BSTRIDE] (LDS).  Leaves in scope mx[16], sec[16], ix[16]: per lane (4c + j, half) and accumulator
// row r, the exact top-2 of class c over the swept columns.  Bs is not read any more after the last barrier of the sweep.
//
// Column keys (match_batch_kernel only: MT_COL_KEYS defined, as a constant expression that enables them in its mutual
// mode — where it is false nothing of them is compiled): for every swept
// column c < G.ncols, one vector global_atomic_max_u64 per wavefront of colkey(best score of the wavefront's 32 rows,
// its smallest row) into ck_keys[c] (kernels_match.hip: colkey_step / colkey_flush).  Expects ck_keys, ck_row0 (the
// row of accumulator register 0 of this lane: rb * 128 + wave * 32 + 4 * half) and ck_last (n1 - 1) in scope.  Where
// MT_COL_KEYS is not defined the sweep is the one match_kernel compiles.
  // ---- A fragment: row (lane&31) of this wave, k = 2t + half, t = 0..63
  const int row_local = rb * MT_ROWS_PER_BLOCK + wave * 32 + col;          // within [0,row_count)
  const int row_ld = G.row_begin + min(row_local, G.row_count - 1);
  float a[64];
  {
    const float4 *src = reinterpret_cast<const float4 *>(pts1[row_ld].data);
#if MT_A_SWAP
    // The two lanes of a row fetch adjacent float4s (k = 8i..8i+3 | 8i+4..8i+7) and trade the halves they do not need
    // with v_permlane32_swap (lanes 32-63 of the first operand <-> lanes 0-31 of the second): 16 loads per lane
    // instead of 32 of which half of every float4 was thrown away — the row fetch is the head of a small launch's
    // critical path and bound by the texture addresser (32 cache lines per instruction: rows are 576 bytes apart).
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const float4 v = src[2 * i + half];
      const auto xy = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v.x), __builtin_bit_cast(unsigned, v.y), false, false);
      const auto zw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v.z), __builtin_bit_cast(unsigned, v.w), false, false);
      a[4 * i + 0] = __builtin_bit_cast(float, (unsigned)xy[0]);       // k = 8i     | 8i + 1
      a[4 * i + 1] = __builtin_bit_cast(float, (unsigned)zw[0]);       // k = 8i + 2 | 8i + 3
      a[4 * i + 2] = __builtin_bit_cast(float, (unsigned)xy[1]);       // k = 8i + 4 | 8i + 5
      a[4 * i + 3] = __builtin_bit_cast(float, (unsigned)zw[1]);       // k = 8i + 6 | 8i + 7
    }
#else
#pragma unroll
    for (int j = 0; j < 32; j++) {
      const float4 v = src[j];
      a[2 * j] = half ? v.y : v.x;
      a[2 * j + 1] = half ? v.w : v.z;
    }
#endif
  }
  // ---- per-lane running top-2 for 16 rows (accumulator register r <-> row (r&3)+8*(r>>2)+4*half)
  float mx[16], sec[16];
  int ix[16];
#pragma unroll
  for (int r = 0; r < 16; r++) { mx[r] = 0.0f; sec[r] = 0.0f; ix[r] = -1; }

  // ---- B staging: thread -> (column scol + 8j, float4 index f4), j = 0..7
  const int scol = tid >> 5, f4 = tid & 31;
  float4 stage[MT_STAGE];
#ifndef MT_LEAN_STAGING
#define MT_LEAN_STAGING 1
#endif
#ifndef MT_TOP2_FILTER
#define MT_TOP2_FILTER 0
#endif
#if MT_LEAN_STAGING
  // r06: the staging costs the SIMD VALU time the matrix pipe does not get back (SQ counters: MFMA busy + VALU issuing ~ 1 of
  // the launch's SIMD-cycles).  (a) one 32-bit byte offset per thread and load (clamp + v_mad_u32_u24) against a wave-uniform
  // (SGPR) tile base instead of clamp + 64-bit multiply-add + 64-bit shift-add per load; (b) the even-k / odd-k halves of a staged float4 go to LDS as ds_write2_b32
  // x,z | y,w — two separate registers each — instead of ds_write2_b64 of register PAIRS the compiler has to assemble with
  // three v_mov per float4.  24 + 8 of the ~196 non-MFMA VALU instructions per super-tile and wavefront.
  const unsigned vconst = (unsigned)G.data_off2 * 4u + (unsigned)f4 * 16u;
  auto gload = [&](int st) {
    const int c0 = tile_col0(G, st);                                         // wave-uniform
    const char *sb = reinterpret_cast<const char *>(set2) + (size_t)c0 * (size_t)G.stride2 * 4u;
    const int last = G.n2 - 1 - c0;                                          // (scalar) the clamp matters in a partial last super-tile only
#pragma unroll
    for (int j = 0; j < MT_STAGE; j++) {
      const unsigned rel = (unsigned)min(scol + 2 * MT_WG_WAVES * j, last);
      stage[j] = *reinterpret_cast<const float4 *>(sb + (__umul24(rel, (unsigned)G.stride2 * 4u) + vconst));
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int j = 0; j < MT_STAGE; j++) {
      float *d = &Bs[buf][(scol + 2 * MT_WG_WAVES * j) * MT_BSTRIDE + 2 * f4];       // k = 4*f4 .. 4*f4+3
      const unsigned a = (unsigned)(size_t)(__attribute__((address_space(3))) float *)d;
      asm volatile("ds_write2_b32 %0, %1, %2 offset1:1" :: "v"(a), "v"(stage[j].x), "v"(stage[j].z) : "memory");            // even k -> half 0
      asm volatile("ds_write2_b32 %0, %1, %2 offset0:64 offset1:65" :: "v"(a), "v"(stage[j].y), "v"(stage[j].w) : "memory"); // odd k -> half 1
    }
  };
  // the compiler's wait-count bookkeeping does not see the DS stores issued from inline asm: before a barrier that publishes
  // them, wait for them by hand
#define MT_LDS_STORES_DONE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#else
  auto gload = [&](int st) {
#pragma unroll
    for (int j = 0; j < MT_STAGE; j++) {
      const int p2 = min(tile_col0(G, st) + scol + 2 * MT_WG_WAVES * j, G.n2 - 1);
      stage[j] = reinterpret_cast<const float4 *>(set2 + (size_t)p2 * G.stride2 + G.data_off2)[f4];
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int j = 0; j < MT_STAGE; j++) {
      float *d = &Bs[buf][(scol + 2 * MT_WG_WAVES * j) * MT_BSTRIDE + 2 * f4];       // k = 4*f4 .. 4*f4+3
      *reinterpret_cast<float2 *>(d) = make_float2(stage[j].x, stage[j].z);        // even k -> half 0
      *reinterpret_cast<float2 *>(d + 64) = make_float2(stage[j].y, stage[j].w);   // odd k  -> half 1
    }
  };
#define MT_LDS_STORES_DONE() do { } while (0)
#endif

#ifndef MT_PIPE_EPILOGUE
#define MT_PIPE_EPILOGUE 1
#endif
#ifndef MT_EARLY_STORE
#define MT_EARLY_STORE 1
#endif
#ifndef MT_EARLY_STORE_AT
#define MT_EARLY_STORE_AT 10
#endif
// timing-only experiments (wrong results): what the barrier / the LDS store / the global loads cost (tools/variants.sh)
#ifndef MT_EXP_NOBARRIER
#define MT_EXP_NOBARRIER 0
#endif
#ifndef MT_EXP_NOSTORE
#define MT_EXP_NOSTORE 0
#endif
#ifndef MT_EXP_NOGLOAD
#define MT_EXP_NOGLOAD 0
#endif
#if defined(MT_COL_KEYS) && (MT_TOP2_FILTER || !MT_PIPE_EPILOGUE)
#error "the column keys live in the pipelined epilogue without MT_TOP2_FILTER"
#endif
#if (MT_EXP_NOBARRIER || MT_EXP_NOSTORE || MT_EXP_NOGLOAD) && !defined(MISIFT_TIMING_ONLY_BUILD)
#error "MT_EXP_* are timing-only experiments that compute WRONG results: build them with -DMISIFT_TIMING_ONLY_BUILD (tools/variants.sh), never into libmisift.so"
#endif
  if (st0 < st1) {
    gload(st0);
#if MT_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    MT_STAMP_MAX(2);               // rows of set 1 and the first super-tile have arrived
#endif
    lstore(0);
  }
  MT_LDS_STORES_DONE();
  __syncthreads();
  MT_STAMP_MAX(3);                 // first super-tile staged
#if MT_PIPE_EPILOGUE
  // Software pipeline over the super-tiles (r03): the top-2 update of tile t-1 (128 VALU instructions on its 32 finished
  // accumulator registers) is issued BETWEEN the MFMAs of tile t instead of after them, so a wavefront's matrix pipe
  // never waits for its own epilogue.  Two accumulator sets alternate (the loop body is instantiated for both, no
  // register copies): 32 more VGPRs, still 2 wavefronts per SIMD.
  auto tile = [&](const int st, floatx16 &acc0, floatx16 &acc1, const floatx16 &prev0, const floatx16 &prev1,
                  const bool have_prev) __attribute__((always_inline)) {
    const int buf = (st - st0) & 1;
#if !MT_EXP_NOGLOAD
    gload(min(st + 1, st1 - 1));
#endif
    const float4 *b0 = reinterpret_cast<const float4 *>(&Bs[buf][col * MT_BSTRIDE + half * 64]);
    const float4 *b1 = reinterpret_cast<const float4 *>(&Bs[buf][(col + 32) * MT_BSTRIDE + half * 64]);
    acc0 = floatx16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    acc1 = floatx16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int pc0 = tile_col0(G, st - 1) + col, pc1 = pc0 + 32;          // columns of the previous tile
    const bool do0 = have_prev && pc0 < G.ncols, do1 = have_prev && pc1 < G.ncols;
#ifdef MT_COL_KEYS
    float kb = 0.0f;               // column key of the previous tile's column pc0 (slots 0-6), then pc1 (slots 8-14)
    int kr = 0;
#endif
    float4 p0 = b0[0], p1 = b1[0], q0, q1;
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      q0 = b0[i + 1]; q1 = b1[i + 1];
      __builtin_amdgcn_sched_barrier(0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 0], p0.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 0], p1.x, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 1], p0.y, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 1], p1.y, acc1, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      // previous tile, ascending column order within the residue class: its columns 0-31 (chain 0) during the first
      // four slots of this tile's k-loop, columns 32-63 (chain 1) during the last four; four rows per slot
      {
        const int t4 = 4 * ((i >> 1) & 3);
#if MT_TOP2_FILTER
        // r06: a score changes a lane's top two only if it beats the running SECOND best — after a few hundred columns that
        // is rare (2/n per lane), so the three instructions behind the compare run only when some lane of the wavefront needs
        // them (wave-uniform branch): on 100 000 columns ~17 % of the row updates.  Exact: a score that is not above `sec`
        // (or is NaN) leaves (mx, sec, ix) untouched in top2_update as well.
        if (i < 8) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const float sc = prev0[t4 + r];
            if (__builtin_amdgcn_ballot_w64(do0 && sc > sec[t4 + r]) != 0ull) {
              if (do0) top2_update(sc, pc0, mx[t4 + r], sec[t4 + r], ix[t4 + r]);
            }
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const float sc = prev1[t4 + r];
            if (__builtin_amdgcn_ballot_w64(do1 && sc > sec[t4 + r]) != 0ull) {
              if (do1) top2_update(sc, pc1, mx[t4 + r], sec[t4 + r], ix[t4 + r]);
            }
          }
        }
#else
        if (i < 8) {
          if (do0) {
#pragma unroll
            for (int r = 0; r < 4; r++) top2_update(prev0[t4 + r], pc0, mx[t4 + r], sec[t4 + r], ix[t4 + r]);
#ifdef MT_COL_KEYS
            if constexpr (MT_COL_KEYS) {
#pragma unroll
              for (int r = 0; r < 4; r++) colkey_step(prev0[t4 + r], t4 + r, kb, kr);
              if (i == 6) colkey_flush(ck_keys + pc0, kb, kr, ck_row0, ck_last, half);
            }
#endif
          }
        } else {
          if (do1) {
#pragma unroll
            for (int r = 0; r < 4; r++) top2_update(prev1[t4 + r], pc1, mx[t4 + r], sec[t4 + r], ix[t4 + r]);
#ifdef MT_COL_KEYS
            if constexpr (MT_COL_KEYS) {
              if (i == 8) { kb = 0.0f; kr = 0; }
#pragma unroll
              for (int r = 0; r < 4; r++) colkey_step(prev1[t4 + r], t4 + r, kb, kr);
              if (i == 14) colkey_flush(ck_keys + pc1, kb, kr, ck_row0, ck_last, half);
            }
#endif
          }
        }
#endif
      }
      __builtin_amdgcn_sched_barrier(0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 2], p0.z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 2], p1.z, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 3], p0.w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 3], p1.w, acc1, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (i + 2 < 16) { p0 = b0[i + 2]; p1 = b1[i + 2]; }
      __builtin_amdgcn_sched_barrier(0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 4], q0.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 4], q1.x, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 5], q0.y, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 5], q1.y, acc1, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
#if MT_EARLY_STORE
      // the next tile's operands go to the other LDS buffer in the MIDDLE of this tile's MFMA stream (the loads were
      // issued at its start; that buffer's readers all passed the previous barrier): nothing but the barrier itself is
      // left between the last MFMA of this tile and the first operand read of the next
#if !MT_EXP_NOSTORE
      if (i == MT_EARLY_STORE_AT) lstore(buf ^ 1);
#endif
      __builtin_amdgcn_sched_barrier(0);
#endif
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 6], q0.z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 6], q1.z, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 7], q0.w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 7], q1.w, acc1, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
#if !MT_EARLY_STORE
    lstore(buf ^ 1);
#endif
#if !MT_EXP_NOBARRIER
    MT_LDS_STORES_DONE();
    __syncthreads();
#endif
  };
  {
    floatx16 A0, A1, B0, B1;
    int st = st0;
    bool have = false;
    for (; st + 1 < st1; st += 2) {
      tile(st, A0, A1, B0, B1, have);
      tile(st + 1, B0, B1, A0, A1, true);
      have = true;
    }
    if (st < st1) {                       // an odd tile left: it finishes B, then its own results are in A
      tile(st, A0, A1, B0, B1, have);
      const int c0 = tile_col0(G, st) + col, c1 = c0 + 32;
      if (c0 < G.ncols) {
#pragma unroll
        for (int r = 0; r < 16; r++) top2_update(A0[r], c0, mx[r], sec[r], ix[r]);
#ifdef MT_COL_KEYS
        if constexpr (MT_COL_KEYS) colkey_tile(ck_keys + c0, A0, ck_row0, ck_last, half);
#endif
      }
      if (c1 < G.ncols) {
#pragma unroll
        for (int r = 0; r < 16; r++) top2_update(A1[r], c1, mx[r], sec[r], ix[r]);
#ifdef MT_COL_KEYS
        if constexpr (MT_COL_KEYS) colkey_tile(ck_keys + c1, A1, ck_row0, ck_last, half);
#endif
      }
    } else if (have) {                    // the last tile of an even count sits in B
      const int c0 = tile_col0(G, st1 - 1) + col, c1 = c0 + 32;
      if (c0 < G.ncols) {
#pragma unroll
        for (int r = 0; r < 16; r++) top2_update(B0[r], c0, mx[r], sec[r], ix[r]);
#ifdef MT_COL_KEYS
        if constexpr (MT_COL_KEYS) colkey_tile(ck_keys + c0, B0, ck_row0, ck_last, half);
#endif
      }
      if (c1 < G.ncols) {
#pragma unroll
        for (int r = 0; r < 16; r++) top2_update(B1[r], c1, mx[r], sec[r], ix[r]);
#ifdef MT_COL_KEYS
        if constexpr (MT_COL_KEYS) colkey_tile(ck_keys + c1, B1, ck_row0, ck_last, half);
#endif
      }
    }
  }
#else
  for (int st = st0; st < st1; st++) {
    const int buf = (st - st0) & 1;
    gload(min(st + 1, st1 - 1));     // unconditional (the last iteration re-fetches its own tile): no phi copies of the 32 staging registers
    const float4 *b0 = reinterpret_cast<const float4 *>(&Bs[buf][col * MT_BSTRIDE + half * 64]);
    const float4 *b1 = reinterpret_cast<const float4 *>(&Bs[buf][(col + 32) * MT_BSTRIDE + half * 64]);
    floatx16 acc0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    floatx16 acc1 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // software pipeline: the ds_read_b128 pair of the next 4 k-pairs is in flight while 8 MFMAs run
    float4 p0 = b0[0], p1 = b1[0], q0, q1;
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      q0 = b0[i + 1]; q1 = b1[i + 1];
      __builtin_amdgcn_sched_barrier(0);        // keep the prefetch ahead of the MFMAs that hide it
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 0], p0.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 0], p1.x, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 1], p0.y, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 1], p1.y, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 2], p0.z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 2], p1.z, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 3], p0.w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 3], p1.w, acc1, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (i + 2 < 16) { p0 = b0[i + 2]; p1 = b1[i + 2]; }
      __builtin_amdgcn_sched_barrier(0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 4], q0.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 4], q1.x, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 5], q0.y, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 5], q1.y, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 6], q0.z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 6], q1.z, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 7], q0.w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * i + 7], q1.w, acc1, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // ascending column order within the residue class: columns 0-31 of the super-tile first
    const int c0 = tile_col0(G, st) + col, c1 = c0 + 32;
    if (c0 < G.ncols) {
#pragma unroll
      for (int r = 0; r < 16; r++) top2_update(acc0[r], c0, mx[r], sec[r], ix[r]);
    }
    if (c1 < G.ncols) {
#pragma unroll
      for (int r = 0; r < 16; r++) top2_update(acc1[r], c1, mx[r], sec[r], ix[r]);
    }
    lstore(buf ^ 1);
    MT_LDS_STORES_DONE();
    __syncthreads();
  }

#endif
  MT_STAMP_MAX(4);                 // sweep done
  // ---- reduce the 4 residues of a class (lanes 4c..4c+3 of the same half): exact merge
#pragma unroll
  for (int r = 0; r < 16; r++)
    top2_merge(mx[r], sec[r], ix[r], quad_xchg<0xB1>(mx[r]), quad_xchg<0xB1>(sec[r]), quad_xchg<0xB1>(ix[r]));
#pragma unroll
  for (int r = 0; r < 16; r++)
    top2_merge(mx[r], sec[r], ix[r], quad_xchg<0x4E>(mx[r]), quad_xchg<0x4E>(sec[r]), quad_xchg<0x4E>(ix[r]));

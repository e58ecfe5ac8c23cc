// pair_plan_body.inc — the body of the pair planner (pair_plan.hpp), included into pair_plan_kernel and
// pair_plan_capped_kernel in kernels_match.hip.  Textual, as match_sweep.inc: as an inline function the same body
// compiled into a different instruction stream of pair_plan_kernel, which misift_match_batch and misift_match_batch_i8 run.
//
// Expects in scope: pairs, npairs, set1, set2, S, hdr, plan; with PAIR_PLAN_CAPPED 1 also max_pts and num_matched: a pair
// with n1 or n2 above max_pts gets no work and pad = 1, and num_matched (when not NULL) starts at 0, or -1 for such a pair.
  __shared__ int s_scan[16][2];
  __shared__ long long s_sum[16];
  const int tid = threadIdx.x;
  long long rsum = 0;
  for (int p = tid; p < npairs; p += 1024) {
    const int f1 = pairs[2 * p], f2 = pairs[2 * p + 1];
    PairPlan P;
    P.n1 = max(set1.counts[f1], 0);
    P.n2 = max(set2.counts[f2], 0);
    P.off1 = (int)set1.base(f1);               // plan offsets are ints, as the API's offsets are
    P.off2 = (int)set2.base(f2);
#if PAIR_PLAN_CAPPED
    const bool over = P.n1 > max_pts || P.n2 > max_pts;
    pair_shape(S, over ? 0 : P.n1, over ? 0 : P.n2, P.ncols, P.ntiles, P.nrb);
    P.nchunks = 1; P.tpc = 1; P.item0 = 0; P.rb0 = 0; P.pad = over ? 1 : 0;
    if (num_matched) num_matched[p] = over ? -1 : 0;
#else
    pair_shape(S, P.n1, P.n2, P.ncols, P.ntiles, P.nrb);
    P.nchunks = 1; P.tpc = 1; P.item0 = 0; P.rb0 = 0; P.pad = 0;
#endif
    plan[p] = P;
    rsum += P.nrb;
  }
  for (int d = 32; d >= 1; d >>= 1) rsum += __shfl_down(rsum, d, 64);
  if ((tid & 63) == 0) s_sum[tid >> 6] = rsum;
  __syncthreads();
  long long R = 0;
  for (int w = 0; w < 16; w++) R += s_sum[w];
  const int C = pair_batch_chunks(S, R);
  int carry_items = 0, carry_rb = 0;
  for (int base = 0; base < npairs; base += 1024) {
    const int p = base + tid;                                  // the thread that wrote plan[p] above
    int v[2] = {0, 0}, nch = 1, tpc = 1;                       // v: items, row blocks
    if (p < npairs) {
      pair_chunks(plan[p].ntiles, C, nch, tpc);
      v[1] = plan[p].nrb;
      v[0] = v[1] * nch;
    }
    int tot[2];
    block_scan(v, tot, s_scan);
    if (p < npairs) {
      plan[p].nchunks = nch; plan[p].tpc = tpc;
      plan[p].item0 = carry_items + v[0]; plan[p].rb0 = carry_rb + v[1];
    }
    carry_items += tot[0]; carry_rb += tot[1];
  }
  if (tid == 0) {
    PairPlan E = {0, 0, 0, 0, 0, 0, 0, 1, 1, carry_items, carry_rb, 0};
    plan[npairs] = E;
    hdr[0] = carry_items; hdr[1] = C; hdr[2] = carry_rb; hdr[3] = 0;
  }

"""misift_match_pairs_batch_i8 against what a caller has without it, on one MI355X (matcher: pair-indexed
int8 batches).

Frames of the synthetic sequence of tools/bench_common.py (~2000 records each) in one packed device array, their 8-bit
descriptors quantised once outside the timed regions.
  (a) pairs (f, f + 1), 64 of them: match_pairs_batch_i8 mutual = 0 against one misift_match_batch_i8;
  (b) the same pairs with mutual = 1, against mutual = 0 and against the two-call cross-check (a forward
      misift_match_batch_i8, then a reversed one (f + 1, f); the record copies and the host comparison that alternative
      also needs are not timed);
  (c) a sequential window of 64 frames at W = 4 (246 pairs (f, f + k), k = 1..4) as one call, mutual 0 and 1, against
      four misift_match_batch_i8 calls (one per k);
  (d) cases (b) and (c) against misift_match_pairs_batch (fp32) with the same arguments;
  (e) one pair of --big x --big records, mutual 0 and 1, against misift_match_batch_i8 on that pair.
Reports the median over --reps timed repetitions (after --warmup) of ms per call sequence, each ended by a sync.  Prints
one JSON line per case; --out FILE also writes the list of results there as JSON."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cudasift_amd import capi  # noqa: E402
from bench_common import sequence, timed  # noqa: E402


class Batch:
    """A packed device batch with its 8-bit descriptors and the calls timed on it."""

    def __init__(self, ctx, frames):
        self.ctx, self.nfr = ctx, len(frames)
        sizes = np.array([len(p) for p in frames], np.int32)
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        self.d = ctx.upload(np.concatenate(frames))
        self.dc, self.do = ctx.upload(sizes), ctx.upload(offs)
        self.dq = ctx.zeros(128 * int(offs[-1]) + 16)
        ctx.quantize_batch(self.d, self.nfr, self.dc, self.do, 0, self.dq)
        ctx.sync()
        self.mp = int(sizes.max())

    def bufs(self, n):
        c = self.ctx
        return c.zeros(576 * n * self.mp), c.zeros(4 * n), c.zeros(4 * n)

    def i8(self, pairs):
        return lambda: self.ctx.match_batch_i8(pairs, self.d, self.dq, self.nfr, self.dc, self.do, 0)

    def pairs_i8(self, pairs, mutual, out):
        return lambda: self.ctx.match_pairs_batch_i8(pairs, self.d, self.dq, self.nfr, self.dc, self.do, 0,
                                                     max_pts=self.mp, mutual=mutual, out=out[0], out_counts=out[1],
                                                     num_matched=out[2])

    def pairs_f32(self, pairs, mutual, out):
        return lambda: self.ctx.match_pairs_batch(pairs, self.d, self.nfr, self.dc, self.do, 0, max_pts=self.mp,
                                                  mutual=mutual, out=out[0], out_counts=out[1], num_matched=out[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--big", type=int, default=100000, help="records per side of the one-pair case (0: skip)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0)
    b = Batch(ctx, sequence(65, a.records, 7 + 64))
    results = []

    def ms(fn, reps=a.reps):
        return round(timed(ctx, fn, a.warmup, reps, sync_after=True), 4)

    def ratio(t, x, y):
        return round(t[x] / t[y], 4)

    # (a) + (b) + (d): 64 pairs (f, f + 1)
    pairs = np.array([(f, f + 1) for f in range(64)], np.int32)
    rev = pairs[:, ::-1].copy()
    out = b.bufs(len(pairs))
    fwd, bwd = b.i8(pairs), b.i8(rev)

    def two_calls():
        fwd()
        bwd()

    t = {"match_batch_i8": ms(fwd),
         "pairs_i8_mutual0": ms(b.pairs_i8(pairs, 0, out)),
         "pairs_i8_mutual1": ms(b.pairs_i8(pairs, 1, out)),
         "two_call_crosscheck_i8": ms(two_calls),
         "pairs_fp32_mutual0": ms(b.pairs_f32(pairs, 0, out)),
         "pairs_fp32_mutual1": ms(b.pairs_f32(pairs, 1, out))}
    r = {"case": "64 pairs (f, f+1)", "pairs": 64, "mean_records": a.records, **t,
         "mutual0_vs_batch_i8": ratio(t, "pairs_i8_mutual0", "match_batch_i8"),
         "mutual1_vs_mutual0": ratio(t, "pairs_i8_mutual1", "pairs_i8_mutual0"),
         "mutual1_vs_two_calls": ratio(t, "pairs_i8_mutual1", "two_call_crosscheck_i8"),
         "mutual1_vs_fp32": ratio(t, "pairs_i8_mutual1", "pairs_fp32_mutual1")}
    print(json.dumps(r), flush=True)
    results.append(r)

    # (c) + (d): window W = 4 over 64 frames
    W = 4
    win = np.array([(f, f + k) for k in range(1, W + 1) for f in range(64 - k)], np.int32)
    out = b.bufs(len(win))
    per_k = [b.i8(np.array([(f, f + k) for f in range(64 - k)], np.int32)) for k in range(1, W + 1)]

    def four_calls():
        for call in per_k:
            call()

    t = {"pairs_i8_one_call": ms(b.pairs_i8(win, 0, out)),
         "pairs_i8_one_call_mutual1": ms(b.pairs_i8(win, 1, out)),
         "match_batch_i8_x4": ms(four_calls),
         "pairs_fp32_one_call": ms(b.pairs_f32(win, 0, out)),
         "pairs_fp32_one_call_mutual1": ms(b.pairs_f32(win, 1, out))}
    r = {"case": "window W=4 over 64 frames", "pairs": int(len(win)), "mean_records": a.records, **t,
         "one_call_vs_four": ratio(t, "pairs_i8_one_call", "match_batch_i8_x4"),
         "mutual1_vs_mutual0": ratio(t, "pairs_i8_one_call_mutual1", "pairs_i8_one_call"),
         "mutual0_vs_fp32": ratio(t, "pairs_i8_one_call", "pairs_fp32_one_call"),
         "mutual1_vs_fp32": ratio(t, "pairs_i8_one_call_mutual1", "pairs_fp32_one_call_mutual1")}
    print(json.dumps(r), flush=True)
    results.append(r)
    del out, b

    # (e): one big pair
    if a.big:
        b = Batch(ctx, sequence(2, a.big, 99))
        out = b.bufs(1)
        one = np.array([(0, 1)], np.int32)
        reps = max(3, a.reps // 4)
        t = {"match_batch_i8": ms(b.i8(one), reps),
             "pairs_i8_mutual0": ms(b.pairs_i8(one, 0, out), reps),
             "pairs_i8_mutual1": ms(b.pairs_i8(one, 1, out), reps)}
        r = {"case": "1 pair of %d x %d" % (a.big, a.big), "pairs": 1, **t,
             "mutual0_vs_batch_i8": ratio(t, "pairs_i8_mutual0", "match_batch_i8"),
             "mutual1_vs_mutual0": ratio(t, "pairs_i8_mutual1", "pairs_i8_mutual0")}
        print(json.dumps(r), flush=True)
        results.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

"""misift_match_pairs_batch against misift_match_batch on one MI355X (matcher: pair-indexed batches).

Frames of the synthetic sequence of tools/bench_common.py (~2000 records each) in one packed device array.
  (a) pairs (f, f + 1), 64 of them: match_pairs_batch mutual = 0 against one misift_match_batch;
  (b) the same pairs with mutual = 1, against mutual = 0 and against the two-call cross-check (a forward
      misift_match_batch, then a reversed one (f + 1, f) in match_full + match_exact_top2 mode; the record copies and the
      host comparison that alternative also needs are not timed);
  (c) a sequential window of 64 frames at W = 4 (246 pairs (f, f + k), k = 1..4) as one match_pairs_batch call, against
      four misift_match_batch calls (one per k).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0)
    nfr = 65
    frames = sequence(nfr, a.records, 7 + 64)
    sizes = np.array([len(p) for p in frames], np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    d = ctx.upload(np.concatenate(frames))
    dc, do = ctx.upload(sizes), ctx.upload(offs)
    mp = int(sizes.max())
    results = []

    def pairs_call(pairs, mutual, out):
        return lambda: ctx.match_pairs_batch(pairs, d, nfr, dc, do, 0, max_pts=mp, mutual=mutual, out=out[0],
                                             out_counts=out[1], num_matched=out[2])

    def bufs(n):
        return ctx.zeros(576 * n * mp), ctx.zeros(4 * n), ctx.zeros(4 * n)

    def ms(fn):
        return round(timed(ctx, fn, a.warmup, a.reps, sync_after=True), 4)

    # (a) + (b): 64 pairs (f, f + 1)
    pairs = np.array([(f, f + 1) for f in range(64)], np.int32)
    rev = pairs[:, ::-1].copy()
    out = bufs(len(pairs))

    def two_calls():
        ctx.match_batch(pairs, d, nfr, dc, do, 0)
        ctx.set_options(match_full=1, match_exact_top2=1)
        ctx.match_batch(rev, d, nfr, dc, do, 0)
        ctx.set_options(match_full=0, match_exact_top2=0)

    t = {"match_batch": ms(lambda: ctx.match_batch(pairs, d, nfr, dc, do, 0)),
         "pairs_mutual0": ms(pairs_call(pairs, 0, out)),
         "pairs_mutual1": ms(pairs_call(pairs, 1, out)),
         "two_call_crosscheck": ms(two_calls)}
    r = {"case": "64 pairs (f, f+1)", "pairs": 64, "mean_records": a.records, **t,
         "mutual0_vs_batch": round(t["pairs_mutual0"] / t["match_batch"], 4),
         "mutual1_vs_mutual0": round(t["pairs_mutual1"] / t["pairs_mutual0"], 4),
         "mutual1_vs_two_calls": round(t["pairs_mutual1"] / t["two_call_crosscheck"], 4)}
    print(json.dumps(r), flush=True)
    results.append(r)

    # (c) window W = 4 over 64 frames
    W = 4
    win = np.array([(f, f + k) for k in range(1, W + 1) for f in range(64 - k)], np.int32)
    out = bufs(len(win))
    per_k = [np.array([(f, f + k) for f in range(64 - k)], np.int32) for k in range(1, W + 1)]

    def four_calls():
        for p in per_k:
            ctx.match_batch(p, d, nfr, dc, do, 0)

    t = {"pairs_one_call": ms(pairs_call(win, 0, out)),
         "pairs_one_call_mutual1": ms(pairs_call(win, 1, out)),
         "match_batch_x4": ms(four_calls)}
    r = {"case": "window W=4 over 64 frames", "pairs": int(len(win)), "mean_records": a.records, **t,
         "one_call_vs_four": round(t["pairs_one_call"] / t["match_batch_x4"], 4)}
    print(json.dumps(r), flush=True)
    results.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

"""misift_find_fundamental_batch + misift_score_fundamental_batch against what they replace at the least, on one MI355X
(README: device batches, epipolar verification).

The README's windowed case: 64 frames of the synthetic sequence of tools/bench_common.py (~2000 records each) in one
packed device array, window W = 4 (246 pairs (f, f + k), k = 1..4), max_pts 2048, the rows produced by
misift_match_pairs_batch_i8 with the cross-check, outside the timed regions; 1000 hypotheses per pair.
  (a) the calls: HIP events on the context stream around find, around score, and around both (misift_timer_start /
      misift_timer_stop_ms), and a host clock around both + sync;
  (b) what a caller does without them before any verification can start: the device-to-host copy of the pairs' rows
      (npairs * max_pts * 576 bytes, into a buffer allocated beforehand), on the host clock.
Every figure is the median over --reps repetitions after --warmup.  The first --check pairs are compared with the numpy
restatement (tests/test_fundamental_cpu) at this size before anything is timed.  Prints one JSON line; --out FILE also
writes it there."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cudasift_amd import capi  # noqa: E402
from bench_common import sequence  # noqa: E402
from test_fundamental_cpu import expected_find, expected_score  # noqa: E402  (bench_common puts tests/ on the path)


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    return round(float(np.median([fn() for _ in range(reps)])), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--max-pts", type=int, default=2048)
    ap.add_argument("--loops", type=int, default=1000)
    ap.add_argument("--thresh", type=float, default=1.0)
    ap.add_argument("--check", type=int, default=3, help="pairs compared with the numpy restatement first")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--host-reps", type=int, default=5, help="repetitions of the read-back")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0)
    L = capi.lib()
    frames = [p[:a.max_pts] for p in sequence(a.frames, a.records, 7 + 64)]
    sizes = np.array([len(p) for p in frames], np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    total, nf, mp = int(offs[-1]), a.frames, a.max_pts
    d = ctx.upload(np.concatenate(frames))
    dc, do = ctx.upload(sizes), ctx.upload(offs)
    dq = ctx.zeros(128 * total + 16)
    ctx.quantize_batch(d, nf, dc, do, 0, dq)
    pairs = np.array([(f, f + k) for k in range(1, a.window + 1) for f in range(nf - k)], np.int32)
    npairs = len(pairs)
    rows, rc, _ = ctx.match_pairs_batch_i8(pairs, d, dq, nf, dc, do, 0, max_pts=mp, mutual=True)
    ctx.sync()
    sel, seeds = np.arange(npairs, dtype=np.int32), np.arange(npairs, dtype=np.uint32) + 1
    gates = (0.85, 0.95)
    dF, dn, dfit = ctx.zeros(36 * npairs), ctx.zeros(4 * npairs), ctx.zeros(4 * npairs)

    def find():
        ctx.find_fundamental_batch(sel, seeds, rows, npairs, rc, None, mp, max_pts=mp, num_loops=a.loops,
                                   min_score=gates[0], max_ambiguity=gates[1], thresh=a.thresh, fundamental=dF,
                                   num_inliers=dn)

    def score():
        ctx.score_fundamental_batch(sel, rows, npairs, rc, dF, None, mp, num_fit=dfit, min_score=gates[0],
                                    max_ambiguity=gates[1], thresh=a.thresh)

    def both():
        find()
        score()

    # the same answer as the restatement at this size, before anything is timed
    h_before = ctx.download(rows, (npairs * mp,), capi.POINT_DTYPE)
    h_rc = ctx.download(rc, (npairs,), np.int32)
    both()
    ctx.sync()
    h_rows = ctx.download(rows, (npairs * mp,), capi.POINT_DTYPE)
    F = ctx.download(dF, (npairs, 9), np.float32)
    num, fit = ctx.download(dn, (npairs,), np.int32), ctx.download(dfit, (npairs,), np.int32)
    for i in range(min(a.check, npairs)):
        sl = slice(i * mp, i * mp + max(int(h_rc[i]), 0))
        Fe, ne = expected_find(h_before[sl], int(h_rc[i]), int(seeds[i]), a.loops, *gates, a.thresh, mp)
        after, fe = expected_score(h_before[sl], int(h_rc[i]), Fe, *gates, a.thresh)
        assert ne == num[i] and Fe.tobytes() == F[i].tobytes() and fe == fit[i], (i, ne, num[i], fe, fit[i])
        assert after.tobytes() == h_rows[sl].tobytes(), i

    def events(fn):
        def run():
            ms = C.c_float()
            ctx.sync()
            capi.check(L.misift_timer_start(ctx.h), "misift_timer_start")
            fn()
            capi.check(L.misift_timer_stop_ms(ctx.h, C.byref(ms)), "misift_timer_stop_ms")
            return ms.value
        return run

    def host_ms(fn):
        def run():
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3
        return run

    def both_and_sync():
        both()
        ctx.sync()

    def copy_rows():
        capi.check(L.misift_copy_d2h(ctx.h, h_rows.ctypes.data, rows.ptr, h_rows.nbytes), "misift_copy_d2h")

    valid = [int(((h_before[i * mp:i * mp + max(int(h_rc[i]), 0)]["score"] > np.float32(gates[0])) &
                  (h_before[i * mp:i * mp + max(int(h_rc[i]), 0)]["ambiguity"] < np.float32(gates[1]))).sum())
             for i in range(npairs)]
    r = {"case": "window W=%d over %d frames, max_pts %d, %d loops" % (a.window, nf, mp, a.loops), "pairs": npairs,
         "records": total, "rows_bytes": int(h_rows.nbytes), "valid_rows_median": int(np.median(valid)),
         "inliers_median": int(np.median(num)), "num_fit_median": int(np.median(fit)),
         "find_events_ms": median_ms(events(find), a.warmup, a.reps),
         "score_events_ms": median_ms(events(score), a.warmup, a.reps),
         "find_score_events_ms": median_ms(events(both), a.warmup, a.reps),
         "find_score_call_and_sync_ms": median_ms(host_ms(both_and_sync), a.warmup, a.reps),
         "rows_d2h_ms": median_ms(host_ms(copy_rows), 1, a.host_reps)}
    r["calls_vs_d2h"] = round(r["find_score_events_ms"] / r["rows_d2h_ms"], 5)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

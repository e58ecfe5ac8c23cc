"""misift_improve_fundamental_batch against what it replaces at the least, on one MI355X (README: device batches,
epipolar verification).

The windowed case of tools/fundamental_time.py: 64 frames of the synthetic sequence of tools/bench_common.py (~2000
records each) in one packed device array, window W = 4 (246 pairs (f, f + k), k = 1..4), max_pts 2048, the rows produced
by misift_match_pairs_batch_i8 with the cross-check and the start F by misift_find_fundamental_batch at 1000 hypotheses,
both outside the timed regions.
  (a) the call at num_loops 0, 1 and 5, and misift_score_fundamental_batch for comparison with num_loops 0: HIP events on
      the context stream around the one call (misift_timer_start / misift_timer_stop_ms).  The start F is copied back
      into place before every timed call, outside the events.  The four variants take turns within every repetition, so
      a drift of the machine meets all of them alike.
  (b) what a host refinement needs before it can start: the device-to-host copy of the pairs' rows (npairs * max_pts *
      576 bytes, into a buffer allocated beforehand), on the host clock.
The synthetic sequence's matches are real but its positions are random, so few rows of a pair agree with any one F (a
median of 15 inliers): its rounds sum over a handful of records and the time is the 9x9 solve's.  A second case gives the
sums their full load: as many frames of tests/test_fundamental_cpu.planted_scene (2000 matches, 25 % outliers, 0.5 px
noise, about 1450 inliers), stride max_pts, the same calls.
Every figure is the median over --reps repetitions after --warmup.  The first --check pairs are compared with the numpy
restatement (tests/test_fundamental_refine_cpu) at this size before anything is timed.  Prints one JSON line; --out FILE
also writes it there."""
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
from test_fundamental_cpu import planted_scene  # noqa: E402  (bench_common puts tests/ on the path)
from test_fundamental_refine_cpu import expected_improve  # noqa: E402

LOOPS = (0, 1, 5)


def measure(ctx, a, rows, rc, npairs, mp):
    """The checks and the timings of one case: rows = npairs frames of stride mp with device counts rc."""
    L = capi.lib()
    sel, seeds = np.arange(npairs, dtype=np.int32), np.arange(npairs, dtype=np.uint32) + 1
    gates = (0.85, 0.95)
    dF, dn = ctx.find_fundamental_batch(sel, seeds, rows, npairs, rc, None, mp, max_pts=mp, num_loops=a.find_loops,
                                        min_score=gates[0], max_ambiguity=gates[1], thresh=a.thresh)
    ctx.sync()
    F0 = ctx.download(dF, (npairs, 9), np.float32)
    num0 = ctx.download(dn, (npairs,), np.int32)
    h_before = ctx.download(rows, (npairs * mp,), capi.POINT_DTYPE)
    h_rc = ctx.download(rc, (npairs,), np.int32)
    dfit, drounds = ctx.zeros(4 * npairs), ctx.zeros(4 * npairs)

    def reset():
        capi.check(L.misift_copy_h2d(ctx.h, dF.ptr, F0.ctypes.data, F0.nbytes), "misift_copy_h2d")

    def improve(loops):
        ctx.improve_fundamental_batch(sel, rows, npairs, rc, dF, None, mp, num_fit=dfit, num_rounds=drounds,
                                      num_loops=loops, min_score=gates[0], max_ambiguity=gates[1], thresh=a.thresh)

    def score():
        ctx.score_fundamental_batch(sel, rows, npairs, rc, dF, None, mp, num_fit=dfit, min_score=gates[0],
                                    max_ambiguity=gates[1], thresh=a.thresh)

    # the same answer as the restatement at this size, before anything is timed
    stats = {}
    for loops in LOOPS:
        reset()
        improve(loops)
        ctx.sync()
        F = ctx.download(dF, (npairs, 9), np.float32)
        fit, rounds = ctx.download(dfit, (npairs,), np.int32), ctx.download(drounds, (npairs,), np.int32)
        h_rows = ctx.download(rows, (npairs * mp,), capi.POINT_DTYPE)
        for i in range(min(a.check, npairs)):
            n = int(h_rc[i])
            sl = slice(i * mp, i * mp + max(n, 0))
            after, Fe, ce, re = expected_improve(h_before[sl], n, F0[i], loops, *gates, a.thresh)
            assert Fe.tobytes() == F[i].tobytes() and ce == fit[i] and re == rounds[i], (loops, i, ce, fit[i], re, rounds[i])
            assert after["match_error"].tobytes() == h_rows[sl]["match_error"].tobytes(), (loops, i)
        assert (fit >= num0).all()
        stats[loops] = (int(np.median(fit)), float(np.median(rounds)))

    def events(fn):
        ms = C.c_float()
        reset()
        ctx.sync()
        capi.check(L.misift_timer_start(ctx.h), "misift_timer_start")
        fn()
        capi.check(L.misift_timer_stop_ms(ctx.h, C.byref(ms)), "misift_timer_stop_ms")
        return ms.value

    variants = {"improve_0_events_ms": lambda: improve(0), "improve_1_events_ms": lambda: improve(1),
                "improve_5_events_ms": lambda: improve(5), "score_events_ms": score}
    times = {k: [] for k in variants}
    for rep in range(a.warmup + a.reps):                         # the variants take turns
        for k, fn in variants.items():
            t = events(fn)
            if rep >= a.warmup:
                times[k].append(t)

    def copy_rows():
        ctx.sync()
        t0 = time.perf_counter()
        capi.check(L.misift_copy_d2h(ctx.h, h_rows.ctypes.data, rows.ptr, h_rows.nbytes), "misift_copy_d2h")
        return (time.perf_counter() - t0) * 1e3

    copy_rows()
    d2h = [copy_rows() for _ in range(a.host_reps)]
    r = {"pairs": npairs, "rows_bytes": int(h_rows.nbytes), "row_count_median": int(np.median(h_rc)),
         "num_fit_median_start": stats[0][0], "num_fit_median_1": stats[1][0], "num_fit_median_5": stats[5][0],
         "rounds_median_1": stats[1][1], "rounds_median_5": stats[5][1]}
    for k, v in times.items():
        r[k] = round(float(np.median(v)), 4)
        r[k.replace("_ms", "_min_ms")] = round(float(np.min(v)), 4)
    r["rows_d2h_ms"] = round(float(np.median(d2h)), 4)
    r["improve_5_vs_d2h"] = round(r["improve_5_events_ms"] / r["rows_d2h_ms"], 5)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--max-pts", type=int, default=2048)
    ap.add_argument("--find-loops", type=int, default=1000)
    ap.add_argument("--thresh", type=float, default=1.0)
    ap.add_argument("--check", type=int, default=3, help="pairs compared with the numpy restatement first")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--host-reps", type=int, default=5, help="repetitions of the read-back")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0)
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
    r = {"windowed": measure(ctx, a, rows, rc, npairs, mp)}
    r["windowed"]["case"] = "window W=%d over %d frames, max_pts %d, start F from %d hypotheses" % (a.window, nf, mp,
                                                                                                  a.find_loops)
    scenes = np.zeros(npairs * mp, capi.POINT_DTYPE)
    for i in range(npairs):
        scenes[i * mp:i * mp + a.records] = planted_scene(i + 1, n=a.records, noise=0.5)[0]
    r["planted"] = measure(ctx, a, ctx.upload(scenes), ctx.upload(np.full(npairs, a.records, np.int32)), npairs, mp)
    r["planted"]["case"] = "%d planted scenes of %d matches, 25 %% outliers, 0.5 px noise, stride %d" % (npairs, a.records,
                                                                                                       mp)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

"""misift_align_points_batch against what it replaces at the least, on one MI355X (README: device batches, aligned
reconstructions).

Entries of 2000 planted correspondences each (align_cases.planted_pairs: b = s R a + t with 0.01 noise, a quarter
displaced by 2 units), pooled one after another, thresh 0.05, min_inliers 12, statuses given, d_inlier written.
  (a) the call at num_loops 256 and 1024 and refit_loops 0, 1 and 5, on 1 and on 16 entries: HIP events on the context
      stream around it (misift_timer_start / misift_timer_stop_ms).
  (b) what a host alignment needs before it can start: the device-to-host copy of the points of both sides (16 bytes
      each), their statuses and the map, into buffers allocated beforehand, on the host clock; for 1 and for 16 entries.
All variants take turns within every repetition, so a drift of the machine meets all alike.  Every figure is the median
over --reps repetitions after --warmup, with the minimum and the 10th and 90th percentiles beside it; kernels_ms is each
launch's mean over ten more calls (16 entries, num_loops 1024, refit_loops 5) with events around it.  All outputs are
compared with the numpy restatement (tests/align_cases.expected_align) at num_loops 256 before anything is timed.  Prints
one JSON line; --out FILE also writes it there."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cudasift_amd import capi  # noqa: E402
import bench_common  # noqa: E402,F401  (puts tests/ on the path)
import align_cases as AC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=2000)
    ap.add_argument("--entries", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--thresh", type=float, default=0.05)
    ap.add_argument("--min-inliers", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    ctx = capi.Context(0)
    sets = {}
    for ne in a.entries:
        case = AC.align_case([AC.pairs_of(a.candidates, 900 + e) for e in range(ne)], num_loops=256, thresh=a.thresh,
                             min_inliers=a.min_inliers, refit_loops=5, pad=(0, 0))
        dev = {k: ctx.upload(np.ascontiguousarray(case[k])) for k in ("src", "dst", "map", "src_status", "dst_status")}
        sizes = dict(sim=16 * ne, align_cand=ne, align_inliers=ne, align_status=ne, summary=8, inlier=len(case["map"]))
        outs = {k: ctx.upload(np.full(m, 0xA5A5A5A5, np.uint32)) for k, m in sizes.items()}
        host = {k: np.empty_like(np.ascontiguousarray(case[k])) for k in dev}
        sets[ne] = dict(case=case, dev=dev, outs=outs, sizes=sizes, host=host)

    def align(ne, num_loops, refit_loops):
        s = sets[ne]
        c, d = s["case"], s["dev"]
        ctx.align_points_batch(d["src"], d["dst"], d["map"], c["ranges"], c["seeds"], src_status=d["src_status"],
                               dst_status=d["dst_status"], num_loops=num_loops, thresh=a.thresh,
                               min_inliers=a.min_inliers, refit_loops=refit_loops, **s["outs"])

    # the same answer as the restatement at this size, before anything is timed
    expected = {}
    for ne in a.entries:
        align(ne, 256, 5)
        ctx.sync()
        e = expected[ne] = AC.expected_align(sets[ne]["case"])
        for k, m in sets[ne]["sizes"].items():
            assert ctx.download(sets[ne]["outs"][k], (m,), np.uint32).tobytes() == e[k].tobytes(), (ne, k)

    def events(fn):
        ms = C.c_float()
        ctx.sync()
        capi.check(L.misift_timer_start(ctx.h), "misift_timer_start")
        fn()
        capi.check(L.misift_timer_stop_ms(ctx.h, C.byref(ms)), "misift_timer_stop_ms")
        return ms.value

    def copy_back(ne):
        s = sets[ne]
        ctx.sync()
        t0 = time.perf_counter()
        for k, h in s["host"].items():
            capi.check(L.misift_copy_d2h(ctx.h, h.ctypes.data, s["dev"][k].ptr, h.nbytes), "misift_copy_d2h")
        return (time.perf_counter() - t0) * 1e3

    variants = {}
    for ne in a.entries:
        for loops in (256, 1024):
            for refits in (0, 1, 5):
                variants["align_entries%d_loops%d_refit%d_events_ms" % (ne, loops, refits)] = (
                    lambda ne=ne, loops=loops, refits=refits: events(lambda: align(ne, loops, refits)))
        variants["inputs_d2h_entries%d_ms" % ne] = lambda ne=ne: copy_back(ne)
    times = {k: [] for k in variants}
    for rep in range(a.warmup + a.reps):                         # the variants take turns
        for k, fn in variants.items():
            t = fn()
            if rep >= a.warmup:
                times[k].append(t)
    ne = max(a.entries)
    ctx.profile_enable(True)                                     # the launches alone: events around each, a run of its own
    ctx.profile_reset()                                          # behind the timed ones
    for _ in range(10):
        align(ne, 1024, 5)
    ctx.sync()
    kernels = {k: round(v["total_ms"] / max(v["calls"], 1), 4) for k, v in ctx.profile_read().items()}
    ctx.profile_enable(False)
    r = {"case": "%d planted correspondences per entry, a quarter displaced by 2 units, 0.01 noise, thresh %g" % (
        a.candidates, a.thresh), "entries": a.entries, "min_inliers": a.min_inliers, "reps": a.reps,
        "d2h_bytes": {str(n): int(sum(h.nbytes for h in sets[n]["host"].values())) for n in a.entries},
        "summary_loops256_refit5": {str(n): expected[n]["summary"].view(np.int32).tolist() for n in a.entries},
        "refits_kept_loops256_refit5": {str(n): [x["kept"] for x in expected[n]["entries"]] for n in a.entries}}
    for k, v in times.items():
        r[k] = round(float(np.median(v)), 4)
        r[k.replace("_ms", "_min_ms")] = round(float(np.min(v)), 4)
        r[k.replace("_ms", "_p10_p90_ms")] = [round(float(x), 4) for x in np.percentile(v, [10, 90])]
    r["kernels_ms_entries%d_loops1024_refit5" % ne] = kernels
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

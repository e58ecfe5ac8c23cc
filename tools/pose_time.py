"""misift_recover_pose_batch against what it replaces at the least, on one MI355X (README: device batches, relative
pose).

The shape of tools/fundamental_refine_time.py's planted case: 246 pairs (window W = 4 over 64 frames) of
tests/pose_cases.planted scenes, 2000 matches each with a quarter of them wrong and 0.5 px noise, K1 != K2, stride
max_pts 2048, each pair's F the exact one of its planted pose.
  (a) the call with d_votes and d_xyz, the call with both NULL, and misift_score_fundamental_batch at the same shape: HIP
      events on the context stream around the one call (misift_timer_start / misift_timer_stop_ms).  The three take
      turns within every repetition, so a drift of the machine meets all of them alike.
  (b) what a host pose recovery needs before it can start: the device-to-host copy of the pairs' rows (npairs * max_pts *
      576 bytes, into a buffer allocated beforehand), on the host clock.
Every figure is the median over --reps repetitions after --warmup.  The first --check pairs are compared with the numpy
restatement (tests/pose_cases.expected_pose) at this size before anything is timed.  Prints one JSON line; --out FILE
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
import bench_common  # noqa: E402,F401  (puts tests/ on the path)
import pose_cases as PC  # noqa: E402

GATES = (0.85, 0.95)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=246)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--max-pts", type=int, default=2048)
    ap.add_argument("--thresh", type=float, default=1.0)
    ap.add_argument("--check", type=int, default=3, help="pairs compared with the numpy restatement first")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--host-reps", type=int, default=5, help="repetitions of the read-back")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    ctx = capi.Context(0)
    npairs, mp, n = a.pairs, a.max_pts, a.records
    rows = np.zeros(npairs * mp, capi.POINT_DTYPE)
    F, K = np.zeros((npairs, 9), np.float32), np.zeros((npairs, 8), np.float32)
    for i in range(npairs):
        s = PC.planted(seed=i + 1, n=n, k2=PC.K_B, angle=0.05, tscale=0.3, outliers=0.25)
        rows[i * mp:i * mp + n], F[i], K[i] = s["recs"], s["F"], s["K8"]
    d_rows, rc, dF = ctx.upload(rows), ctx.upload(np.full(npairs, n, np.int32)), ctx.upload(F)
    sel = np.arange(npairs, dtype=np.int32)
    dpose, dfront, dvotes = ctx.zeros(48 * npairs), ctx.zeros(4 * npairs), ctx.zeros(16 * npairs)
    dxyz, dfit = ctx.zeros(16 * npairs * mp), ctx.zeros(4 * npairs)
    gates = dict(min_score=GATES[0], max_ambiguity=GATES[1], thresh=a.thresh)

    def pose(full):
        ctx.recover_pose_batch(sel, K, d_rows, npairs, rc, dF, None, mp, pose=dpose, num_front=dfront,
                               votes=dvotes if full else None, xyz=dxyz if full else None, **gates)

    def score():
        ctx.score_fundamental_batch(sel, d_rows, npairs, rc, dF, None, mp, num_fit=dfit, **gates)

    # the same answer as the restatement at this size, before anything is timed
    pose(True)
    ctx.sync()
    got = (ctx.download(dpose, (npairs, 12), np.float32), ctx.download(dfront, (npairs,), np.int32),
           ctx.download(dvotes, (npairs, 4), np.int32), ctx.download(dxyz, (npairs * mp, 4), np.uint32))
    for i in range(min(a.check, npairs)):
        with np.errstate(all="ignore"):
            e = PC.expected_pose(rows[i * mp:i * mp + n], n, F[i], K[i], *GATES, a.thresh)
        assert got[0][i].tobytes() == e["pose"].tobytes() and got[1][i] == e["num_front"], (i, got[1][i], e["num_front"])
        assert got[2][i].tolist() == e["votes"].tolist(), (i, got[2][i], e["votes"])
        assert got[3][i * mp:i * mp + n].tobytes() == e["xyz"].view(np.uint32).tobytes(), i

    def events(fn):
        ms = C.c_float()
        ctx.sync()
        capi.check(L.misift_timer_start(ctx.h), "misift_timer_start")
        fn()
        capi.check(L.misift_timer_stop_ms(ctx.h, C.byref(ms)), "misift_timer_stop_ms")
        return ms.value

    variants = {"pose_xyz_events_ms": lambda: pose(True), "pose_events_ms": lambda: pose(False),
                "score_events_ms": score}
    times = {k: [] for k in variants}
    for rep in range(a.warmup + a.reps):                         # the variants take turns
        for k, fn in variants.items():
            t = events(fn)
            if rep >= a.warmup:
                times[k].append(t)

    h_rows = np.empty_like(rows)

    def copy_rows():
        ctx.sync()
        t0 = time.perf_counter()
        capi.check(L.misift_copy_d2h(ctx.h, h_rows.ctypes.data, d_rows.ptr, h_rows.nbytes), "misift_copy_d2h")
        return (time.perf_counter() - t0) * 1e3

    copy_rows()
    d2h = [copy_rows() for _ in range(a.host_reps)]
    r = {"case": "%d planted scenes of %d matches, 25 %% wrong, 0.5 px noise, stride %d" % (npairs, n, mp),
         "pairs": npairs, "rows_bytes": int(rows.nbytes), "num_front_median": int(np.median(got[1])),
         "reps": a.reps}
    for k, v in times.items():
        r[k] = round(float(np.median(v)), 4)
        r[k.replace("_ms", "_min_ms")] = round(float(np.min(v)), 4)
    r["rows_d2h_ms"] = round(float(np.median(d2h)), 4)
    r["pose_xyz_vs_d2h"] = round(r["pose_xyz_events_ms"] / r["rows_d2h_ms"], 5)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

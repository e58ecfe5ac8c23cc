"""misift_recover_pose_planar_batch beside misift_recover_pose_batch, on one MI355X (README: device batches, pose of
planar pairs).

The shape of tools/pose_time.py: 246 pairs (window W = 4 over 64 frames) of tests/pose_planar_cases.planar_scene scenes,
2000 matches each on one plane but for a tenth of them, 0.5 px noise, K1 != K2, stride max_pts 2048, each pair's H a
least-squares fit of its on-plane matches and its F the exact one of its planted pose.  Every entry is planar, so every
entry runs the decomposition, the vote and the depth walk: the call's most expensive case.
  The new call with every optional output, the new call with the four of them NULL, and misift_recover_pose_batch with
  d_votes and d_xyz at the same shape: HIP events on the context stream around the one call (misift_timer_start /
  misift_timer_stop_ms).  The three take turns within every repetition, so a drift of the machine meets all of them
  alike.
Every figure is the median over --reps repetitions after --warmup, with the 10th and 90th percentiles.  The first --check
pairs are compared with the numpy restatement (tests/pose_planar_cases.expected_planar) at this size before anything is
timed.  Prints one JSON line; --out FILE also writes it there."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cudasift_amd import capi  # noqa: E402
import bench_common  # noqa: E402,F401  (puts tests/ on the path)
import pose_cases as PC  # noqa: E402
import pose_planar_cases as PP  # noqa: E402

GATES = (0.85, 0.95)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=246)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--max-pts", type=int, default=2048)
    ap.add_argument("--check", type=int, default=3, help="pairs compared with the numpy restatement first")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    ctx = capi.Context(0)
    npairs, mp, n = a.pairs, a.max_pts, a.records
    rows = np.zeros(npairs * mp, capi.POINT_DTYPE)
    H, F, K = (np.zeros((npairs, k), np.float32) for k in (9, 9, 8))
    for i in range(npairs):
        s = PP.planar_scene(seed=i + 1, n=n, baseline=0.3, off=0.1)
        Fx = np.linalg.inv(PC.kmat(PC.K_B)).T @ PC.skew(s["t"]) @ s["R"] @ np.linalg.inv(PC.kmat(PC.K_A))
        rows[i * mp:i * mp + n], H[i], K[i] = s["recs"], s["H"], s["K8"]
        F[i] = (Fx / np.abs(Fx).max()).astype(np.float32).reshape(9)
    d_rows, rc, dH, dF = ctx.upload(rows), ctx.upload(np.full(npairs, n, np.int32)), ctx.upload(H), ctx.upload(F)
    sel = np.arange(npairs, dtype=np.int32)
    dpose, dfront, dvotes = ctx.zeros(48 * npairs), ctx.zeros(4 * npairs), ctx.zeros(16 * npairs)
    dxyz, dmodel, dhf = ctx.zeros(16 * npairs * mp), ctx.zeros(4 * npairs), ctx.zeros(8 * npairs)
    dalt, dplane = ctx.zeros(48 * npairs), ctx.zeros(16 * npairs)
    gates = dict(min_score=GATES[0], max_ambiguity=GATES[1])

    def planar(full):
        ctx.recover_pose_planar_batch(sel, K, d_rows, npairs, rc, dH, dF, None, mp, model=dmodel, hf_counts=dhf,
                                      pose=dpose, num_front=dfront, votes=dvotes if full else None,
                                      xyz=dxyz if full else None, pose_alt=dalt if full else None,
                                      plane=dplane if full else None, **gates, **PP.PARAMS)

    def pose():
        ctx.recover_pose_batch(sel, K, d_rows, npairs, rc, dF, None, mp, pose=dpose, num_front=dfront, votes=dvotes,
                               xyz=dxyz, thresh=PP.THRESH_F, **gates)

    # the same answer as the restatement at this size, before anything is timed
    planar(True)
    ctx.sync()
    got = dict(model=ctx.download(dmodel, (npairs,), np.int32), hf=ctx.download(dhf, (npairs, 2), np.int32),
               pose=ctx.download(dpose, (npairs, 12), np.float32), front=ctx.download(dfront, (npairs,), np.int32),
               votes=ctx.download(dvotes, (npairs, 4), np.int32), xyz=ctx.download(dxyz, (npairs * mp, 4), np.uint32),
               alt=ctx.download(dalt, (npairs, 12), np.float32), plane=ctx.download(dplane, (npairs, 4), np.float32))
    for i in range(min(a.check, npairs)):
        with np.errstate(all="ignore"):
            e = PP.expected_planar(rows[i * mp:i * mp + n], n, H[i], F[i], K[i])
        assert got["model"][i] == e["model"] == PP.PLANE and got["hf"][i].tolist() == e["hf"].tolist(), (i, e["hf"])
        assert got["pose"][i].tobytes() == e["pose"].tobytes() and got["front"][i] == e["num_front"], i
        assert got["alt"][i].tobytes() == e["pose_alt"].tobytes() and got["plane"][i].tobytes() == e["plane"].tobytes()
        assert got["votes"][i].tolist() == e["votes"].tolist(), (i, got["votes"][i], e["votes"])
        assert got["xyz"][i * mp:i * mp + n].tobytes() == e["xyz"].view(np.uint32).tobytes(), i

    def events(fn):
        ms = C.c_float()
        ctx.sync()
        capi.check(L.misift_timer_start(ctx.h), "misift_timer_start")
        fn()
        capi.check(L.misift_timer_stop_ms(ctx.h, C.byref(ms)), "misift_timer_stop_ms")
        return ms.value

    variants = {"planar_full_events_ms": lambda: planar(True), "planar_events_ms": lambda: planar(False),
                "pose_xyz_events_ms": pose}
    times = {k: [] for k in variants}
    for rep in range(a.warmup + a.reps):                         # the variants take turns
        for k, fn in variants.items():
            t = events(fn)
            if rep >= a.warmup:
                times[k].append(t)
    r = {"case": "%d planar scenes of %d matches, 10 %% off the plane, 0.5 px noise, stride %d" % (npairs, n, mp),
         "pairs": npairs, "planar_entries": int((got["model"] == PP.PLANE).sum()),
         "num_front_median": int(np.median(got["front"])), "reps": a.reps}
    for k, v in times.items():
        r[k] = round(float(np.median(v)), 4)
        r[k.replace("_ms", "_p10_ms")] = round(float(np.percentile(v, 10)), 4)
        r[k.replace("_ms", "_p90_ms")] = round(float(np.percentile(v, 90)), 4)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

"""misift_link_poses_batch against what it replaces at the least, on one MI355X (README: device batches, linked poses).

The README's window: W = 4 over 64 frames, 246 pairs (i, i + k) at max_pts 2048, and every link that window implies: a
CHAIN link (i, i + k) -> (i + k, i + k + m) and a FAN link (i, i + k), (i, i + m) with k < m, the spanning ones first in
outward order from pair (0, 1), then the redundant ones, which the propagation passes over but whose ratios are computed
all the same.  The rows are those of tests/posegraph_cases.scene_rows on a planted path of 64 cameras (2000 points, a
quarter of the matches wrong, 0.5 px noise); each pair's F is the exact one of its planted pose, and d_pose, d_num_front
and d_xyz come from misift_recover_pose_batch on the device.
  (a) the call: HIP events on the context stream around it (misift_timer_start / misift_timer_stop_ms).
  (b) what a host join needs before it can start: the device-to-host copy of the pairs' rows (npairs * max_pts * 576
      bytes) and of d_xyz (16 bytes per row), into buffers allocated beforehand, on the host clock.
The two take turns within every repetition, so a drift of the machine meets both alike.  Every figure is the median over
--reps repetitions after --warmup; kernels_ms is each launch's mean over ten more calls with events around every launch.  All six outputs are compared with the numpy restatement
(tests/posegraph_cases.expected_link_poses) at this size before anything is timed.  Prints one JSON line; --out FILE also
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
import bench_common  # noqa: E402,F401  (puts tests/ on the path)
import pose_cases as PC  # noqa: E402
import posegraph_cases as G  # noqa: E402

GATES = (0.85, 0.95)


def window(nframes, w):
    """(pairs, links, walk) of the window: pairs in order of their first frame, then of their step."""
    pairs = [(i, i + k) for i in range(nframes) for k in range(1, w + 1) if i + k < nframes]
    at = {p: n for n, p in enumerate(pairs)}
    first, rest = [], []
    for i in range(nframes):
        for k in range(1, w + 1):
            if (i, i + k) not in at:
                continue
            for m in range(1, w + 1):
                if (i + k, i + k + m) in at:
                    (first if k == 1 and m == 1 else rest).append((at[(i, i + k)], at[(i + k, i + k + m)], G.CHAIN))
                if m > k and (i, i + m) in at:
                    (first if k == 1 else rest).append((at[(i, i + k)], at[(i, i + m)], G.FAN))
    return pairs, first + rest, [at[(i, i + 1)] for i in range(nframes - 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--max-pts", type=int, default=2048)
    ap.add_argument("--min-common", type=int, default=8)
    ap.add_argument("--max-error", type=float, default=2.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    ctx = capi.Context(0)
    mp, n = a.max_pts, a.records
    pairs, links, walk = window(a.frames, a.window)
    npairs = len(pairs)
    rng = np.random.default_rng(64)
    cams = G.camera_path(a.frames, rng, steps=rng.uniform(0.12, 0.6, a.frames - 1),
                         turn=lambda i: 0.25 * np.sin(0.3 * i))
    centre = np.mean([-r.T @ t for r, t in cams], 0)
    X = centre + rng.uniform([-6, -3, 9], [6, 3, 18], (n, 3))
    raw, _ = G.scene_rows(cams, X, rng, 0.5, 0.25, pairs)
    rows = np.zeros(npairs * mp, capi.POINT_DTYPE)
    F, K = np.zeros((npairs, 9), np.float32), np.tile(np.array(PC.K_A + PC.K_A, np.float32), (npairs, 1))
    Km = PC.kmat(PC.K_A)
    for p, (i, j) in enumerate(pairs):
        (Ra, ta), (Rb, tb) = cams[i], cams[j]
        R, t = Rb @ Ra.T, tb - Rb @ Ra.T @ ta
        f = np.linalg.inv(Km).T @ PC.skew(t) @ R @ np.linalg.inv(Km)
        F[p] = (f / np.abs(f).max()).reshape(9)
        rows[p * mp:p * mp + n] = raw[p]
    d_rows, rc, dF = ctx.upload(rows), ctx.upload(np.full(npairs, n, np.int32)), ctx.upload(F)
    sel = np.arange(npairs, dtype=np.int32)
    gates = dict(min_score=GATES[0], max_ambiguity=GATES[1])
    # match_error under F, then the poses and the depths: what the chain leaves on the device for this call
    ctx.improve_fundamental_batch(sel, d_rows, npairs, rc, dF, None, mp, num_loops=0, thresh=1.0, **gates)
    dxyz = ctx.zeros(16 * npairs * mp)
    dpose, dfront = ctx.recover_pose_batch(sel, K, d_rows, npairs, rc, dF, None, mp, thresh=1.0, xyz=dxyz, **gates)
    outs = dict(link_ratio=ctx.zeros(4 * len(links)), link_common=ctx.zeros(4 * len(links)),
                pair_scale=ctx.zeros(4 * npairs), cam=ctx.zeros(48 * a.frames), cam_pair=ctx.zeros(4 * a.frames),
                summary=ctx.zeros(32))

    def link():
        ctx.link_poses_batch(pairs, a.frames, d_rows, rc, mp, dpose, dfront, dxyz, links, 0, 0, walk,
                             min_common=a.min_common, max_error=a.max_error, **gates, **outs)

    # the same answer as the restatement at this size, before anything is timed
    link()
    ctx.sync()
    case = dict(pairs=np.array(pairs, np.int32), nimages=a.frames,
                rows=ctx.download(d_rows, (npairs * mp,), capi.POINT_DTYPE), row_counts=np.full(npairs, n, np.int32),
                max_pts=mp, max_error=a.max_error, pose=ctx.download(dpose, (npairs, 12), np.float32),
                num_front=ctx.download(dfront, (npairs,), np.int32),
                xyz=ctx.download(dxyz, (npairs * mp, 4), np.float32), links=np.array(links, np.int32), seed_pair=0,
                root_image=0, min_common=a.min_common, walk=np.array(walk, np.int32))
    with np.errstate(all="ignore"):
        e = G.expected_link_poses(case, GATES)
    for k, v in e.items():
        got = ctx.download(outs[k], (v.size,), np.uint32)
        assert got.tobytes() == np.ascontiguousarray(v).view(np.uint32).tobytes(), k
    summary = e["summary"].tolist()

    def events(fn):
        ms = C.c_float()
        ctx.sync()
        capi.check(L.misift_timer_start(ctx.h), "misift_timer_start")
        fn()
        capi.check(L.misift_timer_stop_ms(ctx.h, C.byref(ms)), "misift_timer_stop_ms")
        return ms.value

    h_rows, h_xyz = np.empty_like(rows), np.empty((npairs * mp, 4), np.float32)

    def copy_back():
        ctx.sync()
        t0 = time.perf_counter()
        capi.check(L.misift_copy_d2h(ctx.h, h_rows.ctypes.data, d_rows.ptr, h_rows.nbytes), "misift_copy_d2h")
        capi.check(L.misift_copy_d2h(ctx.h, h_xyz.ctypes.data, dxyz.ptr, h_xyz.nbytes), "misift_copy_d2h")
        return (time.perf_counter() - t0) * 1e3

    times = {"link_poses_events_ms": [], "rows_xyz_d2h_ms": []}
    for rep in range(a.warmup + a.reps):                         # the two take turns
        t = events(link), copy_back()
        if rep >= a.warmup:
            times["link_poses_events_ms"].append(t[0])
            times["rows_xyz_d2h_ms"].append(t[1])
    ctx.profile_enable(True)                                     # the two launches apart: events around each, a run of
    ctx.profile_reset()                                          # its own behind the timed ones
    for _ in range(10):
        link()
    ctx.sync()
    kernels = {k: round(v["total_ms"] / max(v["calls"], 1), 4) for k, v in ctx.profile_read().items()}
    ctx.profile_enable(False)
    gt = G.planted_cameras(cams, 0, pairs[0])
    cam = e["cam"].astype(np.float64)
    r = {"case": "window %d over %d frames, %d matches per pair, 25 %% wrong, 0.5 px noise, stride %d" % (
        a.window, a.frames, n, mp), "pairs": npairs, "links": len(links), "walk": len(walk),
        "d2h_bytes": int(rows.nbytes + h_xyz.nbytes), "summary": summary, "reps": a.reps,
        "camera_position_error_max": round(float(np.linalg.norm(cam[:, 9:] - gt[:, 9:], axis=1).max()), 5)}
    for k, v in times.items():
        r[k] = round(float(np.median(v)), 4)
        r[k.replace("_ms", "_min_ms")] = round(float(np.min(v)), 4)
        r[k.replace("_ms", "_p10_p90_ms")] = [round(float(x), 4) for x in np.percentile(v, [10, 90])]
    r["kernels_ms"] = kernels
    r["link_poses_vs_d2h"] = round(r["link_poses_events_ms"] / r["rows_xyz_d2h_ms"], 5)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

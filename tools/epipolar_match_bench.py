"""misift_match_epipolar_batch against misift_match_batch on the same frame pairs, on one MI355X (matcher:
epipolar-guided pairs).

A planted two-view scene per pair (~2000 records per frame): set-1 frame f holds random positions on a 1920 x 1080 frame,
random depths and random L2-normalised descriptors; set-2 frame f holds 85 % of them seen from a second camera (a small
rotation and a translation, the same K; F = K^-T [t]x R K^-1) plus 0.5 px noise, with perturbed descriptors and shuffled,
and 15 % decoys: copies of other records' descriptors at random positions (repeated texture).  Pairs (f, f) of two packed
device arrays; counts and offsets on the device.  The two calls are timed in the same process, alternating, --reps
repetitions each after --warmup (each followed by a sync, started on an idle device); the medians, the 10th and 90th
percentiles of each (the run-to-run spread the comparison is judged against) and the ratio of the medians are reported,
with the mean candidates per row (the call's own gate, from the library's host hook) and the mean entries gate-tested
per row (the records in the cells the walk visits, from the gather hook, which runs the kernel's span functions on the
grid the bin launch builds).  Prints one JSON line; --out FILE also writes it there."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cudasift_amd import capi  # noqa: E402

W, H = 1920.0, 1080.0
K = np.array([[1.1 * W, 0, W / 2], [0, 1.1 * W, H / 2], [0, 0, 1]])


def motion(i):
    """(R, t) of pair i: a few degrees about each axis and a mostly sideways translation."""
    ax, ay, az = 0.02 + 0.004 * (i % 5), -0.03 + 0.005 * (i % 7), 0.03 * ((i % 4) - 1.5)
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx, np.array([0.5, 0.1 * ((i % 3) - 1), 0.05 * ((i % 2) - 0.5)])


def fundamental(R, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return (F / np.abs(F).max()).astype(np.float32)


def pairs_of_frames(npairs, mean, seed):
    rng = np.random.default_rng(seed)
    set1, set2, Fs = [], [], []
    for i in range(npairs):
        n = int(rng.integers(int(mean * 0.9), int(mean * 1.1)))
        d = rng.random((n, 128), dtype=np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        p1 = np.zeros(n, capi.POINT_DTYPE)
        p1["data"] = d
        p1["xpos"] = rng.random(n) * W
        p1["ypos"] = rng.random(n) * H
        R, t = motion(i)
        keep = rng.permutation(n)[:int(0.85 * n)]
        rays = np.linalg.inv(K) @ np.stack([p1["xpos"][keep], p1["ypos"][keep], np.ones(len(keep))]).astype(np.float64)
        q = K @ (R @ (rays * rng.uniform(4.0, 20.0, len(keep))) + t[:, None])
        x = np.abs(d[keep] + rng.normal(0, 0.01, (len(keep), 128)).astype(np.float32))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        p2 = np.zeros(n, capi.POINT_DTYPE)
        p2["data"][:len(keep)] = x
        p2["xpos"][:len(keep)] = q[0] / q[2] + rng.normal(0, 0.5, len(keep))
        p2["ypos"][:len(keep)] = q[1] / q[2] + rng.normal(0, 0.5, len(keep))
        nd = n - len(keep)
        p2["data"][len(keep):] = d[rng.integers(0, n, nd)]
        p2["xpos"][len(keep):] = rng.random(nd) * W
        p2["ypos"][len(keep):] = rng.random(nd) * H
        set1.append(p1)
        set2.append(p2[rng.permutation(n)])
        Fs.append(fundamental(R, t))
    return set1, set2, Fs


def gate_and_walk(F, p1, p2, radius):
    """(candidates, entries gate-tested) of a pair, summed over its rows, from the library's host hooks."""
    L = capi.lib()
    xy1 = np.ascontiguousarray(np.stack([p1["xpos"], p1["ypos"]], 1), np.float32)
    xy2 = np.ascontiguousarray(np.stack([p2["xpos"], p2["ypos"]], 1), np.float32)
    F = np.ascontiguousarray(F, np.float32).reshape(9)
    out = np.zeros((len(xy1), len(xy2)), np.uint8)
    g = np.zeros(2, np.int32)
    capi.check(L.misift_test_epipolar_gate(F.ctypes.data, xy1.ctypes.data, len(xy1), xy2.ctypes.data, len(xy2), radius,
                                           out.ctypes.data), "misift_test_epipolar_gate")
    cand = int(out.sum())
    capi.check(L.misift_test_epipolar_gather(F.ctypes.data, xy1.ctypes.data, len(xy1), xy2.ctypes.data, len(xy2), radius,
                                             out.ctypes.data, g.ctypes.data), "misift_test_epipolar_gather")
    return cand, int(out.sum())


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(ts)), 4), "p10_ms": round(float(np.percentile(ts, 10)), 4),
            "p90_ms": round(float(np.percentile(ts, 90)), 4)}


def run(ctx, npairs, mean, radius, warmup, reps):
    set1, set2, Fs = pairs_of_frames(npairs, mean, 11 + npairs)
    sizes1 = np.array([len(p) for p in set1], np.int32)
    sizes2 = np.array([len(p) for p in set2], np.int32)
    offs1 = np.concatenate([[0], np.cumsum(sizes1)]).astype(np.int32)
    offs2 = np.concatenate([[0], np.cumsum(sizes2)]).astype(np.int32)
    d1, d2 = ctx.upload(np.concatenate(set1)), ctx.upload(np.concatenate(set2))
    c1, o1, c2, o2 = ctx.upload(sizes1), ctx.upload(offs1), ctx.upload(sizes2), ctx.upload(offs2)
    dF = ctx.upload(np.concatenate([F.reshape(9) for F in Fs]))
    nf = ctx.zeros(4 * npairs)
    pairs = np.array([(f, f) for f in range(npairs)], np.int32)
    rows = int(sizes1.sum())

    def batch():
        ctx.match_batch(pairs, d1, npairs, c1, o1, 0, d2, npairs, c2, o2, 0)
        ctx.sync()

    def epipolar():
        ctx.match_epipolar_batch(pairs, d1, npairs, c1, dF, radius, o1, 0, d2, npairs, c2, o2, 0, max_pts=4096,
                                 num_found=nf)
        ctx.sync()

    for _ in range(warmup):
        batch()
        epipolar()
    tb, te = [], []
    for _ in range(reps):                               # alternating, each started on an idle device
        for fn, ts in ((batch, tb), (epipolar, te)):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
    found = int(ctx.download(nf, (npairs,), np.int32).sum())
    cand = walked = 0
    for F, a, b in zip(Fs, set1, set2):
        c, w = gate_and_walk(F, a, b, radius)
        cand += c
        walked += w
    sb, se = stats(tb), stats(te)
    return {"measured_on": "MI355X", "pairs": npairs, "mean_records": mean, "radius": radius, "reps": reps,
            "match_epipolar_batch": se, "match_batch": sb,
            "ratio_match_batch_over_epipolar": round(sb["median_ms"] / se["median_ms"], 2),
            "epipolar_faster_beyond_spread": bool(se["p90_ms"] < sb["p10_ms"]),
            "candidates_per_row": round(cand / rows, 3), "entries_gate_tested_per_row": round(walked / rows, 2),
            "rows": rows, "rows_matched": found}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if capi.device_count() < 1:
        sys.exit("epipolar_match_bench: no GPU visible; times are measured on the device or not at all")
    ctx = capi.Context(0)
    r = run(ctx, a.pairs, a.records, a.radius, a.warmup, a.reps)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

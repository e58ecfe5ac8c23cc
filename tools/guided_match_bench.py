"""misift_match_guided_batch against misift_match_batch on the same frame pairs, on one MI355X (matcher:
homography-guided pairs).

Synthetic pairs (~2000 records per frame): set-1 frame f holds random positions on a 1920 x 1080 frame and random
L2-normalised descriptors; set-2 frame f holds 85 % of them moved by a fixed H (rotation, scale, translation and a small
perspective term) plus 0.5 px noise, with perturbed descriptors and shuffled, and 15 % decoys: copies of other records'
descriptors at random positions (repeated texture).  Pairs (f, f) of two packed device arrays; counts and offsets on the
device.  For each number of pairs (--pairs) and radius (--radii) it reports the median over --reps timed repetitions
(after --warmup) of one misift_match_guided_batch and of one misift_match_batch (both followed by a sync), the mean
candidates per row (counted on the host with the call's own gate), the rows of set 1 per second of the guided call and
the rows it matched.  Prints one JSON line per case; --out FILE also writes the list of results there as JSON."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cudasift_amd import capi  # noqa: E402
from bench_common import timed  # noqa: E402

H = np.array([[1.01 * np.cos(0.035), -1.01 * np.sin(0.035), 15.0],
              [1.01 * np.sin(0.035), 1.01 * np.cos(0.035), -8.0],
              [1e-6, -2e-6, 1.0]], np.float32)


def pairs_of_frames(npairs, mean, seed):
    rng = np.random.default_rng(seed)
    set1, set2 = [], []
    for _ in range(npairs):
        n = int(rng.integers(int(mean * 0.9), int(mean * 1.1)))
        d = rng.random((n, 128), dtype=np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        p1 = np.zeros(n, capi.POINT_DTYPE)
        p1["data"] = d
        p1["xpos"] = rng.random(n) * 1920
        p1["ypos"] = rng.random(n) * 1080
        keep = rng.permutation(n)[:int(0.85 * n)]
        q = H.astype(np.float64) @ np.stack([p1["xpos"][keep], p1["ypos"][keep], np.ones(len(keep))]).astype(np.float64)
        x = np.abs(d[keep] + rng.normal(0, 0.01, (len(keep), 128)).astype(np.float32))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        p2 = np.zeros(n, capi.POINT_DTYPE)
        p2["data"][:len(keep)] = x
        p2["xpos"][:len(keep)] = q[0] / q[2] + rng.normal(0, 0.5, len(keep))
        p2["ypos"][:len(keep)] = q[1] / q[2] + rng.normal(0, 0.5, len(keep))
        nd = n - len(keep)
        p2["data"][len(keep):] = d[rng.integers(0, n, nd)]
        p2["xpos"][len(keep):] = rng.random(nd) * 1920
        p2["ypos"][len(keep):] = rng.random(nd) * 1080
        set1.append(p1)
        set2.append(p2[rng.permutation(n)])
    return set1, set2


def candidates(p1, p2, radius):
    """Candidates of every row, with the call's gate (numpy float32, C's order)."""
    h = H.reshape(9)
    x, y = p1["xpos"], p1["ypos"]
    den = h[6] * x + h[7] * y + h[8]
    px = (h[0] * x + h[1] * y + h[2]) / den
    py = (h[3] * x + h[4] * y + h[5]) / den
    dx = px[:, None] - p2["xpos"][None, :]
    dy = py[:, None] - p2["ypos"][None, :]
    return int(((dx * dx + dy * dy) < np.float32(radius) * np.float32(radius)).sum())


def run(ctx, npairs, mean, radii, warmup, reps):
    set1, set2 = pairs_of_frames(npairs, mean, 11 + npairs)
    sizes1 = np.array([len(p) for p in set1], np.int32)
    sizes2 = np.array([len(p) for p in set2], np.int32)
    offs1 = np.concatenate([[0], np.cumsum(sizes1)]).astype(np.int32)
    offs2 = np.concatenate([[0], np.cumsum(sizes2)]).astype(np.int32)
    d1, d2 = ctx.upload(np.concatenate(set1)), ctx.upload(np.concatenate(set2))
    c1, o1, c2, o2 = ctx.upload(sizes1), ctx.upload(offs1), ctx.upload(sizes2), ctx.upload(offs2)
    dH = ctx.upload(np.tile(H.reshape(9), npairs))
    nf = ctx.zeros(4 * npairs)
    pairs = np.array([(f, f) for f in range(npairs)], np.int32)
    rows = int(sizes1.sum())

    def batch():
        ctx.match_batch(pairs, d1, npairs, c1, o1, 0, d2, npairs, c2, o2, 0)
        ctx.sync()

    batch_ms = timed(ctx, batch, warmup, reps, sync_after=False)
    out = []
    for radius in radii:
        def guided():
            ctx.match_guided_batch(pairs, d1, npairs, c1, dH, radius, o1, 0, d2, npairs, c2, o2, 0, max_pts=4096,
                                   num_found=nf)
            ctx.sync()

        guided_ms = timed(ctx, guided, warmup, reps, sync_after=False)
        found = int(ctx.download(nf, (npairs,), np.int32).sum())
        cand = sum(candidates(a, b, radius) for a, b in zip(set1, set2))
        out.append({"pairs": npairs, "mean_records": mean, "radius": radius, "guided_ms": round(guided_ms, 4),
                    "match_batch_ms": round(batch_ms, 4), "speedup": round(batch_ms / guided_ms, 2),
                    "candidates_per_row": round(cand / rows, 3), "guided_mrows_s": round(rows / guided_ms / 1e3, 2),
                    "rows": rows, "rows_matched": found})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="8,64,256")
    ap.add_argument("--radii", default="4,10,32")
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    radii = [float(v) for v in a.radii.split(",")]
    ctx = capi.Context(0)
    results = []
    for n in (int(v) for v in a.pairs.split(",")):
        for r in run(ctx, n, a.records, radii, a.warmup, a.reps):
            print(json.dumps(r), flush=True)
            results.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

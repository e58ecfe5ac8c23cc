"""misift_find_homography_batch + misift_improve_homography_batch against a per-pair loop of misift_find_homography +
misift_improve_homography on one MI355X (homography: batched frames).

Frames of ~--records matched records each (tests/synth.py synth_matches: 60 % inliers of a known homography) in one packed
device array.  (a) per frame: srand-seeded misift_find_homography (host rand() draws, three host round trips) then
misift_improve_homography, counts known on the host; (b) the two batch calls with the counts on the device, one
synchronisation at the end.  Reports the median over --reps timed repetitions (after --warmup) of ms per batch, the
speed-up, and the inlier tests per second (entries x loops rounded up to 16 x records).  Also the median latency of one
misift_find_homography on one frame.  Prints one JSON line per case; --out FILE also writes the list of results there."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cudasift_amd import capi  # noqa: E402
from bench_common import timed  # noqa: E402
from synth import synth_matches  # noqa: E402

FIND = (0.85, 0.95, 5.0)          # min_score, max_ambiguity, thresh (API defaults)
IMPROVE = (5, 0.0, 0.80, 3.0)     # loops, min_score, max_ambiguity, thresh (mainSift.cpp:78)
LIBC = C.CDLL(None)


def frames(n, mean, seed):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(int(mean * 0.9), int(mean * 1.1), n)
    return [synth_matches(int(s), seed=seed * 1000 + f)[0] for f, s in enumerate(sizes)]


def run(ctx, nsel, mean, loops, warmup, reps):
    fr = frames(nsel, mean, 5 + nsel)
    sizes = np.array([len(p) for p in fr], np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    d = ctx.upload(np.concatenate(fr))
    dc, do = ctx.upload(sizes), ctx.upload(offs)
    sel = np.arange(nsel, dtype=np.int32)
    seeds = np.arange(1, nsel + 1, dtype=np.uint32)
    dH, dn, dnf = ctx.zeros(36 * nsel), ctx.zeros(4 * nsel), ctx.zeros(4 * nsel)
    L = capi.lib()
    H = (C.c_float * 9)()
    nm, nf = C.c_int(), C.c_int()

    def loop():
        for f in range(nsel):
            LIBC.srand(C.c_uint(int(seeds[f])))
            p = d.ptr + 576 * int(offs[f])
            capi.check(L.misift_find_homography(ctx.h, p, int(sizes[f]), H, C.byref(nm), loops, *FIND),
                       "misift_find_homography")
            capi.check(L.misift_improve_homography(ctx.h, p, int(sizes[f]), H, IMPROVE[0], *IMPROVE[1:], C.byref(nf)),
                       "misift_improve_homography")

    def batch():
        ctx.find_homography_batch(sel, seeds, d, nsel, dc, do, 0, max_pts=int(sizes.max()), num_loops=loops,
                                  min_score=FIND[0], max_ambiguity=FIND[1], thresh=FIND[2], homography=dH,
                                  num_matches=dn)
        ctx.improve_homography_batch(sel, d, nsel, dc, dH, do, 0, num_fit=dnf, num_loops=IMPROVE[0],
                                     min_score=IMPROVE[1], max_ambiguity=IMPROVE[2], thresh=IMPROVE[3])
        ctx.sync()

    def single():
        LIBC.srand(C.c_uint(1))
        capi.check(L.misift_find_homography(ctx.h, d.ptr, int(sizes[0]), H, C.byref(nm), loops, *FIND),
                   "misift_find_homography")

    t_loop = timed(ctx, loop, warmup, reps, sync_after=False)
    t_batch = timed(ctx, batch, warmup, reps, sync_after=False)
    t_single = timed(ctx, single, warmup, max(reps, 20), sync_after=False)
    tests = float(nsel) * ((loops + 15) // 16 * 16) * float(sizes.sum()) / nsel
    return {"entries": nsel, "mean_records": mean, "loops": loops, "loop_ms": round(t_loop, 4),
            "batch_ms": round(t_batch, 4), "speedup": round(t_loop / t_batch, 2),
            "loop_gtests_s": round(tests / (t_loop * 1e-3) / 1e9, 3),
            "batch_gtests_s": round(tests / (t_batch * 1e-3) / 1e9, 3),
            "single_find_ms": round(t_single, 4), "single_find_records": int(sizes[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", default="8,64,256")
    ap.add_argument("--loops", default="1000,10000")
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0)
    results = []
    for loops in (int(v) for v in a.loops.split(",")):
        for n in (int(v) for v in a.entries.split(",")):
            r = run(ctx, n, a.records, loops, a.warmup, a.reps)
            print(json.dumps(r), flush=True)
            results.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

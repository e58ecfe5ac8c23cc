"""misift_match_batch against a loop of misift_match on one MI355X (matcher: batched pairs).

Frames of a synthetic sequence (~2000 records each: frame f + 1 = frame f's descriptors, perturbed and shuffled, so the
matches are real) in one packed device array; pairs (f, f + 1).  (a) one misift_match per pair, counts known on the host;
(b) one misift_match_batch with the counts on the device.  Reports the median over --reps timed repetitions (after
--warmup) of ms per batch, Mpairs/s and the fraction of the 157.3 TFLOP/s fp32 matrix peak (256 flop per row x column).
Prints one JSON line per batch size; --out FILE also writes the list of results there as JSON."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cudasift_amd import capi  # noqa: E402
from bench_common import sequence, timed  # noqa: E402

PEAK = 157.3e12


def run(ctx, npairs, mean, warmup, reps):
    frames = sequence(npairs + 1, mean, 7 + npairs)
    sizes = np.array([len(p) for p in frames], np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    d = ctx.upload(np.concatenate(frames))
    dc, do = ctx.upload(sizes), ctx.upload(offs)
    pairs = np.array([(f, f + 1) for f in range(npairs)], np.int32)
    L = capi.lib()

    def loop():
        for f in range(npairs):
            capi.check(L.misift_match(ctx.h, d.ptr + 576 * int(offs[f]), int(sizes[f]), d.ptr + 576 * int(offs[f + 1]),
                                      int(sizes[f + 1])), "misift_match")

    def batch():
        ctx.match_batch(pairs, d, npairs + 1, dc, do, 0)
        ctx.sync()

    # the timed region ends when fn returns: batch() ends with its own sync, loop() with the last misift_match
    out = {name: timed(ctx, fn, warmup, reps, sync_after=False) for name, fn in (("loop", loop), ("batch", batch))}
    flop = 256.0 * float((sizes[:-1].astype(np.float64) * sizes[1:]).sum())
    res = {"pairs": npairs, "mean_records": mean, "loop_ms": round(out["loop"], 4), "batch_ms": round(out["batch"], 4),
           "speedup": round(out["loop"] / out["batch"], 2),
           "loop_mpairs_s": round(npairs / out["loop"] / 1e3, 4), "batch_mpairs_s": round(npairs / out["batch"] / 1e3, 4),
           "loop_peak_frac": round(flop / (out["loop"] * 1e-3) / PEAK, 4),
           "batch_peak_frac": round(flop / (out["batch"] * 1e-3) / PEAK, 4), "gflop": round(flop / 1e9, 2)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="8,64,256")
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0)
    results = []
    for n in (int(v) for v in a.pairs.split(",")):
        r = run(ctx, n, a.records, a.warmup, a.reps)
        print(json.dumps(r), flush=True)
        results.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

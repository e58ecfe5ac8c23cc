"""misift_match_batch_i8 (int8 matrix cores) against misift_match_batch (fp32 matrix cores) on one MI355X (DESIGN.md,
matcher: 8-bit descriptors).

(a) frames of a synthetic sequence (~2000 records each: frame f + 1 = frame f's descriptors, perturbed and shuffled, so
the matches are real) in one packed device array, pairs (f, f + 1), for 8 / 64 / 256 pairs; (b) one pair of 100 000 x
100 000.  misift_quantize_batch is timed on its own (it runs once per frame, not per pair).  Reports the median over
--reps timed repetitions (after --warmup) of ms per call (host clock around the call and a synchronise), Mpairs/s, and
the fraction of peak: fp32 against 157.3 TFLOP/s, int8 against 5.0 POP/s (256 operations per row x column; spec peaks,
MI355X_MICROARCH.md).  Prints one JSON line per case; --out FILE also writes the list of results there as JSON."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cudasift_amd import capi  # noqa: E402
from bench_common import sequence, timed  # noqa: E402

PEAK_F32 = 157.3e12
PEAK_I8 = 5.0e15


def run(ctx, frames, pairs, warmup, reps, label):
    sizes = np.array([len(p) for p in frames], np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    nf = len(frames)
    d = ctx.upload(np.concatenate(frames))
    dc, do = ctx.upload(sizes), ctx.upload(offs)
    dq = ctx.zeros(128 * int(offs[-1]) + 16)
    pairs = np.asarray(pairs, np.int32)
    t_q = timed(ctx, lambda: ctx.quantize_batch(d, nf, dc, do, 0, dq), warmup, reps, sync_after=True)
    t_f = timed(ctx, lambda: ctx.match_batch(pairs, d, nf, dc, do, 0), warmup, reps, sync_after=True)
    t_i = timed(ctx, lambda: ctx.match_batch_i8(pairs, d, dq, nf, dc, do, 0), warmup, reps, sync_after=True)
    ops = 256.0 * float(sum(float(sizes[a]) * float(sizes[b]) for a, b in pairs))
    n = len(pairs)
    return {"case": label, "pairs": n, "quantize_ms": round(t_q, 4), "fp32_ms": round(t_f, 4), "i8_ms": round(t_i, 4),
            "speedup": round(t_f / t_i, 2), "fp32_mpairs_s": round(n / t_f / 1e3, 4),
            "i8_mpairs_s": round(n / t_i / 1e3, 4), "fp32_peak_frac": round(ops / (t_f * 1e-3) / PEAK_F32, 4),
            "i8_peak_frac": round(ops / (t_i * 1e-3) / PEAK_I8, 4), "gops": round(ops / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="8,64,256")
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--big", type=int, default=100000, help="records per side of the one-pair case (0: skip)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0)
    results = []
    for n in (int(v) for v in a.pairs.split(",") if v):
        frames = sequence(n + 1, a.records, 7 + n)
        r = run(ctx, frames, [(f, f + 1) for f in range(n)], a.warmup, a.reps, "%d pairs of ~%d" % (n, a.records))
        print(json.dumps(r), flush=True)
        results.append(r)
    if a.big:
        frames = sequence(2, a.big, 99)
        r = run(ctx, frames, [(0, 1)], a.warmup, max(3, a.reps // 4), "1 pair of %d x %d" % (a.big, a.big))
        print(json.dumps(r), flush=True)
        results.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

"""What the batch bench tools share: the synthetic frame sequence and the timing loop."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cudasift_amd import capi  # noqa: E402
from synth import synth_descriptors  # noqa: E402


def sequence(nframes, mean, seed):
    """Frames of about `mean` records (exactly `mean` for one frame): frame f + 1 = frame f's descriptors, perturbed and
    shuffled, so the matches are real."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(int(mean * 0.9), int(mean * 1.1), nframes) if nframes > 1 else np.array([mean])
    d = synth_descriptors(int(sizes.max()) * 2, seed)
    frames, cur = [], d[:sizes[0]]
    for f in range(nframes):
        n = int(sizes[f])
        base = cur[rng.permutation(len(cur))[:n]] if len(cur) >= n else np.concatenate([cur, d[:n - len(cur)]])
        x = np.abs(base + rng.normal(0, 0.003, base.shape).astype(np.float32))
        x /= np.sqrt((x * x).sum(1, keepdims=True))
        p = np.zeros(n, capi.POINT_DTYPE)
        p["data"] = x
        p["xpos"] = rng.random(n) * 1920
        p["ypos"] = rng.random(n) * 1080
        frames.append(p)
        cur = x
    return frames


def timed(ctx, fn, warmup, reps, *, sync_after):
    """Median ms of fn() over reps repetitions after warmup, each started on an idle device.  sync_after: the timed
    region ends with a ctx.sync() of its own (fn only enqueues) rather than when fn returns (fn waits for its work)."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        if sync_after:
            ctx.sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3

"""misift_select_pairs_batch (preemptive matching) on one MI355X, beside what a caller has without it (README: device
batches, choosing the pairs).

The workload: N frames of about 2000 records (the synthetic descriptors of tools/bench_common.py, scales drawn per
record) in one packed device array, quantised once outside the timed regions.  Variants, taking turns in one process so
that each sees the same machine:
  select N=64 / N=512, top=256 / top=100   one misift_select_pairs_batch call, k = 8, min_votes = 4
  exhaustive N=64                          misift_match_pairs_batch_i8 (mutual) over all 2016 pairs at max_pts 2048:
                                           what the parent offered an unordered set
Every figure is HIP events on the context stream around the call (misift_timer_start / misift_timer_stop_ms): the
median, the 10th and the 90th percentile over --reps rounds after --warmup.  The split over the launches comes from a
pass of its own with the library's per-launch events on (misift_profile_enable), which serialise the launches and are
therefore not part of the call figures.  Before anything is timed the N=64 outputs are compared with the numpy
restatement (tests/select_cases.py).  Without a GPU the tool fails: it has no number to give.  Prints one JSON line;
--out FILE also writes it there."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cudasift_amd import capi  # noqa: E402
from bench_common import sequence  # noqa: E402
import select_cases as SC  # noqa: E402  (bench_common puts tests/ on the path)


def batch(ctx, nframes, records, seed):
    frames = sequence(nframes, records, seed)
    rng = np.random.default_rng(seed + 1)
    for p in frames:
        p["scale"] = np.exp(rng.normal(1.0, 0.8, len(p))).astype(np.float32)
    sizes = np.array([len(p) for p in frames], np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    recs = np.concatenate(frames)
    d, dc, do = ctx.upload(recs), ctx.upload(sizes), ctx.upload(offs[:nframes])
    dq = ctx.zeros(128 * len(recs) + 16)
    ctx.quantize_batch(d, nframes, dc, do, 0, dq)
    ctx.sync()
    return dict(n=nframes, recs=recs, sizes=sizes, offs=offs[:nframes], d=d, dc=dc, do=do, dq=dq)


def stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "p10_ms": round(float(np.percentile(ms, 10)), 4),
            "p90_ms": round(float(np.percentile(ms, 90)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--tops", type=int, nargs="+", default=[256, 100])
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--min-votes", type=int, default=4)
    ap.add_argument("--exhaustive-frames", type=int, default=64)
    ap.add_argument("--max-pts", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--split-reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert capi.device_count() >= 1, "select_pairs_time needs an MI355X: there is no number without one"
    ctx = capi.Context(0)
    L = capi.lib()
    gates = dict(min_score=0.85, max_ambiguity=0.95, min_votes=a.min_votes, k=a.k)
    batches = {n: batch(ctx, n, a.records, 7 + n) for n in sorted(set(a.frames + [a.exhaustive_frames]))}

    variants, info = {}, {}
    for n in a.frames:
        B = batches[n]
        for top in a.tops:
            out = ctx.select_pairs_batch(B["d"], B["dq"], n, B["dc"], B["do"], 0, top=top, **gates)
            ctx.sync()

            def call(B=B, n=n, top=top, out=out):
                ctx.select_pairs_batch(B["d"], B["dq"], n, B["dc"], B["do"], 0, top=top, **gates,
                                       **dict(zip(SC.OUTPUTS, out)))
            name = "select_n%d_top%d" % (n, top)
            variants[name] = call
            s = ctx.download(out[5], (8,), np.int32)
            info[name] = {"frames": n, "top": top, "all_pairs": n * (n - 1) // 2, "pairs_selected": int(s[0]),
                          "frames_without_neighbour": int(s[2]), "max_votes": int(s[4])}
            if n == min(a.frames):                               # the restatement's bytes, before anything is timed
                case = dict(recs=B["recs"], q=SC.quantize_np(B["recs"]["data"]).reshape(-1, 128), counts=B["sizes"],
                            offs=B["offs"], stride=0, memo={}, top=top, max_pairs=n * (n - 1) // 2, **gates)
                exp = SC.expected(case, poison=0)
                for key, buf in zip(SC.OUTPUTS, out):
                    got = ctx.download(buf, exp[key].shape, np.int32)
                    assert got.tobytes() == exp[key].tobytes(), (name, key)
                info[name]["checked_against_restatement"] = True

    E = batches[a.exhaustive_frames]
    ne = a.exhaustive_frames
    all_pairs = np.array([(x, y) for x in range(ne) for y in range(x + 1, ne)], np.int32)
    eout = ctx.match_pairs_batch_i8(all_pairs, E["d"], E["dq"], ne, E["dc"], E["do"], 0, max_pts=a.max_pts, mutual=True)
    ctx.sync()

    def exhaustive():
        ctx.match_pairs_batch_i8(all_pairs, E["d"], E["dq"], ne, E["dc"], E["do"], 0, max_pts=a.max_pts, mutual=True,
                                 out=eout[0], out_counts=eout[1], num_matched=eout[2])
    ename = "exhaustive_match_pairs_i8_n%d" % ne
    variants[ename] = exhaustive
    info[ename] = {"frames": ne, "pairs": len(all_pairs), "max_pts": a.max_pts,
                   "output_bytes": int(len(all_pairs)) * a.max_pts * 576}

    def events(fn):
        ms = C.c_float()
        ctx.sync()
        capi.check(L.misift_timer_start(ctx.h), "misift_timer_start")
        fn()
        capi.check(L.misift_timer_stop_ms(ctx.h, C.byref(ms)), "misift_timer_stop_ms")
        return ms.value

    times = {k: [] for k in variants}
    for r in range(a.warmup + a.reps):
        for k, fn in variants.items():                           # the variants take turns
            t = events(fn)
            if r >= a.warmup:
                times[k].append(t)
    result = {"device": "MI355X", "records_per_frame": a.records, "reps": a.reps, "k": a.k, "min_votes": a.min_votes,
              "variants": {k: dict(info[k], **stats(times[k])) for k in variants}}

    # the split over the launches, in a pass of its own
    ctx.profile_enable(True)
    for k, fn in variants.items():
        fn()
        ctx.sync()
        ctx.profile_reset()
        for _ in range(a.split_reps):
            fn()
        ctx.sync()
        split = ctx.profile_read()
        result["variants"][k]["launch_ms_mean"] = {nm: round(v["total_ms"] / max(v["calls"], 1), 4)
                                                   for nm, v in sorted(split.items())}
    ctx.profile_enable(False)
    sel = result["variants"].get("select_n%d_top256" % ne)
    if sel:
        result["select_top256_vs_exhaustive_n%d" % ne] = round(sel["median_ms"] / result["variants"][ename]["median_ms"], 5)
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

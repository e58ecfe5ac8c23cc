"""misift_merge_scenes_batch beside what it replaces, the read-back of everything a host merge would need before it can
start, on one MI355X (README: device batches, merging two reconstructions).

The shape is two of the README's windows that overlap by half: 64 images each, image i of A is image i of the merged
scene and image i of B is image i + 32, 96 images in all; 863 tracks and 55 232 observations per scene.  431 world
tracks run through all 96 images, so both scenes hold them (64 observations each, the 32 of the shared images twice);
432 tracks per scene are its own.  The exports are fabricated directly (tests/merge_cases.scene_from_tracks), each
scene's tracks in an order of its own; the map is the one misift_correspond_tracks_batch gives for them, and every tie is
accepted.  All four optional arrays are given.
  (a) the call, HIP events on the context stream around it (misift_timer_start / misift_timer_stop_ms);
  (b) the device-to-host copy of what a host merge needs before it can start: per scene the T + 1 offsets, the O
      observations, the summary, the T points, view counts and statuses, the cameras and d_cam_pair and the record index,
      and the map and the accept flags, into pinned memory, events around the copies.  The copy is given T and O for
      nothing (a real caller reads the summaries first), and misift_copy_d2h waits for the end of each copy.
The two take turns within every repetition, so a drift of the machine meets both alike.  Every figure is the median over
--reps repetitions after --warmup, with the 10th and 90th percentiles beside it.  kernels_ms is the time per call of each
launch group, the mean over ten more calls with events around every group; shares are of their sum.  All thirteen outputs
are compared with the numpy restatement (tests/merge_cases.expected_merge) at this size before anything is timed.  Prints
one JSON line; --out FILE also writes it there."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cudasift_amd import capi  # noqa: E402
import bench_common  # noqa: E402,F401  (puts tests/ on the path)
import merge_cases as MC  # noqa: E402


def two_windows(nimages, shift, shared, own, per_frame, seed):
    """The case of the docstring: (case, T, O per scene)."""
    rng = np.random.default_rng(seed)
    world = [("ab", 0, nimages + shift)] * shared + [("a", 0, nimages)] * own + [("b", shift, nimages + shift)] * own
    scenes, index = {}, {}
    for which, fs in (("a", 0), ("b", shift)):
        mine = [k for k, w in enumerate(world) if which in w[0]]
        mine = [mine[i] for i in rng.permutation(len(mine))]
        index[which] = {k: t for t, k in enumerate(mine)}
        tracks = [[(f - fs, k) for f in range(max(world[k][1], fs), min(world[k][2], fs + nimages))] for k in mine]
        scenes[which] = MC.scene_from_tracks(tracks, nimages, seed + (which == "b"), per_frame=per_frame)
    point_map = np.full(len(index["a"]), -1, np.int32)
    for k, t in index["a"].items():
        if k in index["b"]:
            point_map[t] = index["b"][k]
    case = MC.merge_case(scenes["a"], scenes["b"], point_map, accept=np.ones(len(point_map), np.int32), fshift_a=0,
                         fshift_b=shift, slack_images=0, per_frame=per_frame)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--shift", type=int, default=32)
    ap.add_argument("--shared", type=int, default=431)
    ap.add_argument("--own", type=int, default=432)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    ctx = capi.Context(0)
    case = two_windows(a.images, a.shift, a.shared, a.own, a.records, 64)
    ins = MC.inputs(case)
    dev = {}
    for s in "ab":
        S = case[s]
        dev[s] = dict({k: ctx.upload(v) for k, v in ins[s].items()}, max_tracks=S["max_tracks"], max_obs=S["max_obs"],
                      nimages=S["nimages"], max_records=S["max_records"])
    dmap, dacc = ctx.upload(ins["map"]), ctx.upload(ins["accept"])
    sizes = MC.sizes(case)
    outs = {k: ctx.upload(np.full(m, MC.POISON_WORD, np.uint32)) for k, m in sizes.items()}

    def merge():
        ctx.merge_scenes_batch(dev["a"], dev["b"], dmap, case["nimages_out"], case["max_tracks_out"], case["max_obs_out"],
                               accept=dacc, fshift_a=case["fshift_a"], fshift_b=case["fshift_b"],
                               rshift_a=case["rshift_a"], rshift_b=case["rshift_b"],
                               max_records_out=case["max_records_out"], **outs)

    # the same answer as the restatement at this size, before anything is timed
    merge()
    ctx.sync()
    e = MC.expected_merge(case)
    for k in MC.OUTPUTS:
        assert ctx.download(outs[k], (sizes[k],), np.uint32).tobytes() == e[k].tobytes(), k

    def events(fn):
        ms = C.c_float()
        ctx.sync()
        capi.check(L.misift_timer_start(ctx.h), "misift_timer_start")
        fn()
        capi.check(L.misift_timer_stop_ms(ctx.h, C.byref(ms)), "misift_timer_stop_ms")
        return ms.value

    # what a host merge reads back first
    reads = [(dmap, 4 * MC.counts(case["a"])[0]), (dacc, 4 * MC.counts(case["a"])[0])]
    for s in "ab":
        S, d = case[s], dev[s]
        T, O = MC.counts(S)
        reads += [(d["track_offsets"], 4 * (T + 1)), (d["obs"], 16 * O), (d["export_summary"], 32), (d["points"], 16 * T),
                  (d["point_views"], 4 * T), (d["point_status"], 4 * T), (d["cam"], 48 * S["nimages"]),
                  (d["cam_pair"], 4 * S["nimages"]), (d["record_obs"], 4 * S["max_records"])]
    pinned = [capi.PinnedArray((max(b, 4),), np.uint8) for _, b in reads]

    def read_back():
        for (buf, b), dst in zip(reads, pinned):
            capi.check(L.misift_copy_d2h(ctx.h, dst.array.ctypes.data, buf.ptr, b), "misift_copy_d2h")

    times = {"merge_events_ms": [], "read_back_events_ms": []}
    for rep in range(a.warmup + a.reps):                         # the two take turns
        t = (events(merge), events(read_back))
        if rep >= a.warmup:
            for k, v in zip(times, t):
                times[k].append(v)
    ctx.profile_enable(True)                                     # the launch groups alone: events around each, a run of
    ctx.profile_reset()                                          # its own behind the timed ones
    for _ in range(10):
        merge()
    ctx.sync()
    kernels = {k: round(v["total_ms"] / 10, 4) for k, v in ctx.profile_read().items() if k.startswith("merge_")}
    ctx.profile_enable(False)
    total_k = sum(kernels.values())
    s = e["summary"].view(np.int32)
    unions = [len(m["union"]) for m in e["res"]["merged"]]
    r = {"case": "two windows of %d images overlapping by %d, %d tracks through both and %d of its own per scene" % (
        a.images, a.images - a.shift, a.shared, a.own),
        "tracks_a": MC.counts(case["a"])[0], "observations_a": MC.counts(case["a"])[1],
        "tracks_b": MC.counts(case["b"])[0], "observations_b": MC.counts(case["b"])[1], "images_out": case["nimages_out"],
        "records_out": case["max_records_out"], "summary": s.tolist(), "tracks_merged": int(s[0]),
        "observations_merged": int(s[1]), "duplicates_removed": int(s[5]), "largest_union": max(unions),
        "staged_on_chip": MC.capacity(), "reps": a.reps, "read_back_bytes": int(sum(b for _, b in reads))}
    for k, v in times.items():
        r[k] = round(float(np.median(v)), 4)
        r[k.replace("_ms", "_min_ms")] = round(float(np.min(v)), 4)
        r[k.replace("_ms", "_p10_p90_ms")] = [round(float(x), 4) for x in np.percentile(v, [10, 90])]
    r["kernels_ms"] = kernels
    r["kernel_shares"] = {k: round(v / total_k, 4) for k, v in kernels.items()} if total_k else {}
    r["merge_vs_read_back"] = round(r["merge_events_ms"] / r["read_back_events_ms"], 4)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

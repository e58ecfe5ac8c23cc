"""misift_export_tracks_batch against what it replaces, on one MI355X (README: device batches, feature tracks).

The workload of tools/tracks_time.py: 64 frames of the synthetic sequence of tools/bench_common.py (~2000 records each)
in one packed device array, window W = 4 (246 pairs (f, f + k), k = 1..4), max_pts 2048, the rows produced by
misift_match_pairs_batch_i8 with the cross-check and the labels by one misift_link_tracks_batch call, both outside the
timed regions.  The export runs with min_len = 2 and consistent_only = 1.
  (a) the call: HIP events on the context stream around one misift_export_tracks_batch (misift_timer_start /
      misift_timer_stop_ms), and a host clock around call + sync;
  (b) what a caller does without it: the device-to-host copy of the three label arrays, the device-to-host copy of the
      records' xpos / ypos (misift_download_fields) and the numpy restatement of the call on the copies
      (tests/test_tracks_export_cpu.expected_export), each on the host clock.  The upload of the result, which a next
      stage on the GPU would need as well, is not counted.
Every figure is the median over --reps repetitions after --warmup.  The call's five outputs are compared with the
restatement's at this size before anything is timed.  Prints one JSON line; --out FILE also writes it there."""
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
from bench_common import sequence  # noqa: E402
from test_tracks_export_cpu import NAMES, expected_export  # noqa: E402  (bench_common puts tests/ on the path)


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    return round(float(np.median([fn() for _ in range(reps)])), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--max-pts", type=int, default=2048)
    ap.add_argument("--min-len", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--host-reps", type=int, default=5, help="repetitions of the read-back and the numpy restatement")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0)
    L = capi.lib()
    frames = [p[:a.max_pts] for p in sequence(a.frames, a.records, 7 + 64)]
    sizes = np.array([len(p) for p in frames], np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    total, nf, mp = int(offs[-1]), a.frames, a.max_pts
    d = ctx.upload(np.concatenate(frames))
    dc, do = ctx.upload(sizes), ctx.upload(offs)
    dq = ctx.zeros(128 * total + 16)
    ctx.quantize_batch(d, nf, dc, do, 0, dq)
    pairs = np.array([(f, f + k) for k in range(1, a.window + 1) for f in range(nf - k)], np.int32)
    rows, rc, _ = ctx.match_pairs_batch_i8(pairs, d, dq, nf, dc, do, 0, max_pts=mp, mutual=True)
    lab = ctx.link_tracks_batch(pairs, rows, rc, mp, nf, dc, do, 0, max_records=total)
    ctx.sync()
    max_tracks, max_obs = total // a.min_len + 1, total
    shapes = ((max_tracks + 1,), np.int32), ((max_tracks,), np.int32), ((max_obs,), capi.TRACK_OBS_DTYPE), \
        ((total,), np.int32), ((8,), np.int32)
    out = [ctx.zeros(4 * (max_tracks + 1)), ctx.zeros(4 * max_tracks), ctx.zeros(16 * max_obs), ctx.zeros(4 * total),
           ctx.zeros(32)]

    def call():
        ctx.export_tracks_batch(d, nf, dc, do, 0, max_records=total, track=lab[0], track_len=lab[1],
                                track_frames=lab[2], min_len=a.min_len, consistent_only=1, max_tracks=max_tracks,
                                max_obs=max_obs, track_offsets=out[0], track_root=out[1], obs=out[2], record_obs=out[3],
                                summary=out[4])

    h_lab = [np.empty(total, np.int32) for _ in range(3)]
    h_recs = np.zeros(total, capi.POINT_DTYPE)

    def copy_labels():
        for h, b in zip(h_lab, lab[:3]):
            capi.check(L.misift_copy_d2h(ctx.h, h.ctypes.data, b.ptr, h.nbytes), "misift_copy_d2h")

    def copy_positions():
        capi.check(L.misift_download_fields(ctx.h, h_recs.ctypes.data, d.ptr, total, 0, 2), "misift_download_fields")

    def restate():
        xy = np.stack([np.ascontiguousarray(h_recs[k]).view(np.uint32) for k in ("xpos", "ypos")], 1)
        return expected_export(xy, sizes, offs, 0, total, *h_lab, a.min_len, 1, max_tracks, max_obs, 0)

    # the same answer as the restatement at this size, before anything is timed
    call()
    ctx.sync()
    copy_labels()
    copy_positions()
    got = [ctx.download(b, *s) for b, s in zip(out, shapes)]
    for g, e, name in zip(got, restate(), NAMES):
        assert g.tobytes() == e.tobytes(), name

    def call_events():
        ms = C.c_float()
        ctx.sync()
        capi.check(L.misift_timer_start(ctx.h), "misift_timer_start")
        call()
        capi.check(L.misift_timer_stop_ms(ctx.h, C.byref(ms)), "misift_timer_stop_ms")
        return ms.value

    def host_ms(fn):
        def run():
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3
        return run

    def call_and_sync():
        call()
        ctx.sync()

    s = got[4]
    r = {"case": "window W=%d over %d frames, max_pts %d, min_len %d, consistent only" % (a.window, nf, mp, a.min_len),
         "pairs": len(pairs), "records": total, "selected_tracks": int(s[0]), "selected_observations": int(s[1]),
         "tracks_written": int(s[2]), "observations_written": int(s[3]), "longest_written": int(s[4]),
         "export_tracks_events_ms": median_ms(call_events, a.warmup, a.reps),
         "export_tracks_call_and_sync_ms": median_ms(host_ms(call_and_sync), a.warmup, a.reps),
         "labels_d2h_ms": median_ms(host_ms(copy_labels), 1, a.host_reps),
         "positions_d2h_ms": median_ms(host_ms(copy_positions), 1, a.host_reps),
         "numpy_restatement_ms": median_ms(host_ms(restate), 1, a.host_reps)}
    r["readback_total_ms"] = round(r["labels_d2h_ms"] + r["positions_d2h_ms"] + r["numpy_restatement_ms"], 4)
    r["call_vs_d2h"] = round(r["export_tracks_events_ms"] / (r["labels_d2h_ms"] + r["positions_d2h_ms"]), 5)
    r["call_vs_readback_total"] = round(r["export_tracks_events_ms"] / r["readback_total_ms"], 5)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

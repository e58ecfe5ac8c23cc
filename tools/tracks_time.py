"""misift_link_tracks_batch against what it replaces at the least, on one MI355X (README: device batches, feature tracks).

The README's windowed case: 64 frames of the synthetic sequence of tools/bench_common.py (~2000 records each) in one
packed device array, window W = 4 (246 pairs (f, f + k), k = 1..4), max_pts 2048, the rows produced by
misift_match_pairs_batch_i8 with the cross-check, outside the timed regions.
  (a) the call: HIP events on the context stream around one misift_link_tracks_batch (misift_timer_start /
      misift_timer_stop_ms), and a host clock around call + sync;
  (b) what a caller does without it: the device-to-host copy of the pairs' rows (npairs * max_pts * 576 bytes, into a
      buffer allocated beforehand) and the numpy restatement of the call on them (tests/test_tracks_cpu.expected_tracks),
      each on the host clock.
Every figure is the median over --reps repetitions after --warmup.  The call's four outputs are compared with the
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
from test_tracks_cpu import expected_tracks  # noqa: E402  (bench_common puts tests/ on the path)


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
    npairs = len(pairs)
    rows, rc, _ = ctx.match_pairs_batch_i8(pairs, d, dq, nf, dc, do, 0, max_pts=mp, mutual=True)
    ctx.sync()
    gates = (0.85, 0.95, float("inf"))
    out = [ctx.zeros(4 * total) for _ in range(3)] + [ctx.zeros(32)]

    def call():
        ctx.link_tracks_batch(pairs, rows, rc, mp, nf, dc, do, 0, max_records=total, min_score=gates[0],
                              max_ambiguity=gates[1], max_error=gates[2], track=out[0], track_len=out[1],
                              track_frames=out[2], summary=out[3])

    # the same answer as the restatement at this size, before anything is timed
    call()
    ctx.sync()
    h_rows = ctx.download(rows, (npairs * mp,), capi.POINT_DTYPE)
    h_rc = ctx.download(rc, (npairs,), np.int32)
    exp = expected_tracks(pairs, h_rows, h_rc, mp, sizes, offs, 0, total, gates)
    got = [ctx.download(b, (n,), np.int32) for b, n in zip(out, (total,) * 3 + (8,))]
    for g, e, name in zip(got, exp, ("track", "track_len", "track_frames", "summary")):
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

    def copy_rows():
        capi.check(L.misift_copy_d2h(ctx.h, h_rows.ctypes.data, rows.ptr, h_rows.nbytes), "misift_copy_d2h")

    s = got[3]
    r = {"case": "window W=%d over %d frames, max_pts %d" % (a.window, nf, mp), "pairs": npairs, "records": total,
         "rows_bytes": int(h_rows.nbytes), "accepted_edges": int(s[0]), "tracks": int(s[1]),
         "records_in_tracks": int(s[2]), "inconsistent": int(s[3]), "longest": int(s[4]),
         "link_tracks_events_ms": median_ms(call_events, a.warmup, a.reps),
         "link_tracks_call_and_sync_ms": median_ms(host_ms(call_and_sync), a.warmup, a.reps),
         "rows_d2h_ms": median_ms(host_ms(copy_rows), 1, a.host_reps),
         "numpy_restatement_ms": median_ms(
             host_ms(lambda: expected_tracks(pairs, h_rows, h_rc, mp, sizes, offs, 0, total, gates)), 1, a.host_reps)}
    r["readback_total_ms"] = round(r["rows_d2h_ms"] + r["numpy_restatement_ms"], 4)
    r["call_vs_d2h"] = round(r["link_tracks_events_ms"] / r["rows_d2h_ms"], 5)
    r["call_vs_readback_total"] = round(r["link_tracks_events_ms"] / r["readback_total_ms"], 5)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

"""misift_resect_cameras_batch against what it replaces at the least, on one MI355X (README: device batches, resected
cameras).

The README's window: W = 4 over 64 frames, 246 pairs (i, i + k) at max_pts 2048, on the planted path of 64 cameras of
tools/link_poses_time.py (2000 points, a quarter of the matches wrong, 0.5 px noise; each pair's F is the exact one of its
planted pose).  Both chains and misift_triangulate_tracks_batch run on the device first, as in
tools/refine_cameras_time.py: the offsets, d_obs and the export summary, d_points and d_point_status.  All 64 images are
resected (only_unset = 0, install = 0), max_cand 2048, thresh 4 px.
  (a) the call at num_loops 256 and 1024: HIP events on the context stream around it (misift_timer_start /
      misift_timer_stop_ms).
  (b) what a host resection needs before it can start: the device-to-host copy of the O observations written (16 bytes
      each), the T + 1 offsets, the T points (16 bytes each) and their status, into buffers allocated beforehand, on the
      host clock.
The three take turns within every repetition, so a drift of the machine meets all alike.  Every figure is the median over
--reps repetitions after --warmup; kernels_ms is each launch's mean over ten more calls at num_loops 1024 with events
around it, and solve_share / count_share their part of the four.  All outputs are compared with the numpy restatement
(tests/resect_cases.expected_resect) at this size before anything is timed.  Prints one JSON line; --out FILE also writes
it there."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cudasift_amd import capi  # noqa: E402
import bench_common  # noqa: E402,F401  (puts tests/ on the path)
import pose_cases as PC  # noqa: E402
import posegraph_cases as G  # noqa: E402
import refine_cases as RC  # noqa: E402
import resect_cases as C6  # noqa: E402
import triangulate_cases as TC  # noqa: E402
from link_poses_time import GATES, window  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--max-pts", type=int, default=2048)
    ap.add_argument("--min-common", type=int, default=8)
    ap.add_argument("--max-error", type=float, default=2.0)
    ap.add_argument("--min-len", type=int, default=3)
    ap.add_argument("--num-loops", type=int, default=5, help="Gauss-Newton steps of the triangulation")
    ap.add_argument("--max-cand", type=int, default=2048)
    ap.add_argument("--thresh", type=float, default=4.0)
    ap.add_argument("--min-inliers", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = capi.lib()
    ctx = capi.Context(0)
    mp, n, nf = a.max_pts, a.records, a.frames
    pairs, links, walk = window(nf, a.window)
    npairs = len(pairs)
    rng = np.random.default_rng(64)
    cams = G.camera_path(nf, rng, steps=rng.uniform(0.12, 0.6, nf - 1), turn=lambda i: 0.25 * np.sin(0.3 * i))
    centre = np.mean([-r.T @ t for r, t in cams], 0)
    X = centre + rng.uniform([-6, -3, 9], [6, 3, 18], (n, 3))
    raw, _ = G.scene_rows(cams, X, rng, 0.5, 0.25, pairs)
    rows = np.zeros(npairs * mp, capi.POINT_DTYPE)
    F, K8 = np.zeros((npairs, 9), np.float32), np.tile(np.array(PC.K_A + PC.K_A, np.float32), (npairs, 1))
    Km = PC.kmat(PC.K_A)
    recs = np.zeros(nf * n, capi.POINT_DTYPE)                    # the record batch the rows index: n records per image
    for p, (i, j) in enumerate(pairs):
        (Ra, ta), (Rb, tb) = cams[i], cams[j]
        R, t = Rb @ Ra.T, tb - Rb @ Ra.T @ ta
        f = np.linalg.inv(Km).T @ PC.skew(t) @ R @ np.linalg.inv(Km)
        F[p] = (f / np.abs(f).max()).reshape(9)
        rows[p * mp:p * mp + n] = raw[p]
        for k, mk in (("xpos", "match_xpos"), ("ypos", "match_ypos")):
            recs[k][i * n:(i + 1) * n] = raw[p][k]
            recs[k][j * n + raw[p]["match"]] = raw[p][mk]
    d_rows, rc, dF = ctx.upload(rows), ctx.upload(np.full(npairs, n, np.int32)), ctx.upload(F)
    sel = np.arange(npairs, dtype=np.int32)
    gates = dict(min_score=GATES[0], max_ambiguity=GATES[1])
    # the pose chain: match_error under F, the poses and the depths, the cameras
    ctx.improve_fundamental_batch(sel, d_rows, npairs, rc, dF, None, mp, num_loops=0, thresh=1.0, **gates)
    dxyz = ctx.zeros(16 * npairs * mp)
    dpose, dfront = ctx.recover_pose_batch(sel, K8, d_rows, npairs, rc, dF, None, mp, thresh=1.0, xyz=dxyz, **gates)
    _, _, _, dcam, dcam_pair, _ = ctx.link_poses_batch(pairs, nf, d_rows, rc, mp, dpose, dfront, dxyz, links, 0, 0, walk,
                                                       min_common=a.min_common, max_error=a.max_error, **gates)
    # the track chain
    total = nf * n
    d_recs, d_cnt = ctx.upload(recs), ctx.upload(np.full(nf, n, np.int32))
    lab = ctx.link_tracks_batch(pairs, d_rows, rc, mp, nf, d_cnt, None, n, max_records=total,
                                max_error=a.max_error, **gates)
    max_tracks, max_obs = total // a.min_len + 1, total
    doff, _, dobs, _, dsum = ctx.export_tracks_batch(d_recs, nf, d_cnt, None, n, max_records=total, track=lab[0],
                                                     track_len=lab[1], track_frames=lab[2], min_len=a.min_len,
                                                     consistent_only=1, max_tracks=max_tracks, max_obs=max_obs,
                                                     record_obs=None)
    K = np.tile(np.array(PC.K_A, np.float32), (nf, 1))
    tri = ctx.triangulate_tracks_batch(max_tracks, max_obs, doff, dobs, dsum, nf, dcam, dcam_pair, K, min_views=2,
                                       num_loops=a.num_loops)
    dpts, dstatus = tri[0], tri[2]
    images, seeds = np.arange(nf, dtype=np.int32), np.arange(nf, dtype=np.uint32) + 1
    sizes = dict(res_cam=12 * nf, res_cand=nf, res_inliers=nf, res_status=nf, summary=8)
    outs = {k: ctx.upload(np.full(m, TC.POISON_WORD, np.uint32)) for k, m in sizes.items()}

    def resect(num_loops):
        ctx.resect_cameras_batch(max_tracks, max_obs, doff, dobs, dsum, dpts, dstatus, nf, K, images, seeds, a.max_cand,
                                 num_loops=num_loops, thresh=a.thresh, min_inliers=a.min_inliers, only_unset=0, install=0,
                                 cam=dcam, cam_pair=dcam_pair, **outs)

    # the same answer as the restatement at this size, before anything is timed
    base = dict(max_tracks=max_tracks, max_obs=max_obs, track_offsets=ctx.download(doff, (max_tracks + 1,), np.int32),
                obs=ctx.download(dobs, (max_obs,), TC.OBS_DTYPE), export_summary=ctx.download(dsum, (8,), np.int32),
                nimages=nf, cam=ctx.download(dcam, (nf, 12), np.float32),
                cam_pair=ctx.download(dcam_pair, (nf,), np.int32), intrinsics=K,
                points=ctx.download(dpts, (max_tracks, 4), np.float32),
                point_status=ctx.download(dstatus, (max_tracks,), np.int32))
    expected = {}
    for loops in (256, 1024):
        resect(loops)
        ctx.sync()
        case = C6.resect_case(base, images, seeds=seeds, max_cand=a.max_cand, num_loops=loops, thresh=a.thresh,
                              min_inliers=a.min_inliers)
        e = expected[loops] = C6.expected_resect(case)
        for k in C6.OUTPUTS:
            assert ctx.download(outs[k], (sizes[k],), np.uint32).tobytes() == e[k].tobytes(), (loops, k)
    T, O = RC.counts(base)

    def events(fn):
        ms = C.c_float()
        ctx.sync()
        capi.check(L.misift_timer_start(ctx.h), "misift_timer_start")
        fn()
        capi.check(L.misift_timer_stop_ms(ctx.h, C.byref(ms)), "misift_timer_stop_ms")
        return ms.value

    h_obs, h_off = np.empty(max(O, 1), TC.OBS_DTYPE), np.empty(T + 1, np.int32)
    h_pts, h_status = np.empty((max(T, 1), 4), np.float32), np.empty(max(T, 1), np.int32)

    def copy_back():
        ctx.sync()
        t0 = time.perf_counter()
        for h, d, nbytes in ((h_obs, dobs, 16 * O), (h_off, doff, h_off.nbytes), (h_pts, dpts, 16 * T),
                             (h_status, dstatus, 4 * T)):
            capi.check(L.misift_copy_d2h(ctx.h, h.ctypes.data, d.ptr, nbytes), "misift_copy_d2h")
        return (time.perf_counter() - t0) * 1e3

    times = {"resect_loops256_events_ms": [], "resect_loops1024_events_ms": [], "inputs_d2h_ms": []}
    for rep in range(a.warmup + a.reps):                         # the three take turns
        t = (events(lambda: resect(256)), events(lambda: resect(1024)), copy_back())
        if rep >= a.warmup:
            for k, v in zip(times, t):
                times[k].append(v)
    ctx.profile_enable(True)                                     # the launches alone: events around each, a run of its own
    ctx.profile_reset()                                          # behind the timed ones
    for _ in range(10):
        resect(1024)
    ctx.sync()
    kernels = {k: round(v["total_ms"] / max(v["calls"], 1), 4) for k, v in ctx.profile_read().items()}
    ctx.profile_enable(False)
    e = expected[1024]
    ents = e["entries"]
    ok = np.array([x["status"] == C6.OK for x in ents])
    r = {"case": "window %d over %d frames, %d matches per pair, 25 %% wrong, 0.5 px noise, tracks of %d and more" % (
        a.window, nf, n, a.min_len), "pairs": npairs, "tracks": T, "observations": O, "images": nf,
        "max_cand": a.max_cand, "thresh_px": a.thresh, "min_inliers": a.min_inliers,
        "d2h_bytes": int(16 * O + h_off.nbytes + 20 * T), "reps": a.reps,
        "summary_loops256": expected[256]["summary"].view(np.int32).tolist(),
        "summary_loops1024": e["summary"].view(np.int32).tolist(),
        "candidates_per_image_median": int(np.median([x["cand"] for x in ents])),
        "inlier_share_median": round(float(np.median([x["inliers"] / max(x["cand"], 1) for x in ents])), 4),
        "resected_of_images": [int(ok.sum()), nf]}
    for k, v in times.items():
        r[k] = round(float(np.median(v)), 4)
        r[k.replace("_ms", "_min_ms")] = round(float(np.min(v)), 4)
        r[k.replace("_ms", "_p10_p90_ms")] = [round(float(x), 4) for x in np.percentile(v, [10, 90])]
    r["kernels_ms"] = kernels
    total = sum(kernels.get(k, 0.0) for k in ("resect_gather", "resect_solve", "resect_count", "resect_pick"))
    if total > 0:
        r["solve_share"] = round(kernels.get("resect_solve", 0.0) / total, 4)
        r["count_share"] = round(kernels.get("resect_count", 0.0) / total, 4)
    for loops in (256, 1024):
        r["resect_loops%d_vs_d2h" % loops] = round(r["resect_loops%d_events_ms" % loops] / r["inputs_d2h_ms"], 5)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

"""misift_filter_tracks_batch beside what it replaces, the read-back of the lists a host filter would need, and the loop
it is for, on one MI355X (README: device batches, filtering the observations).

The README's window: W = 4 over 64 frames, 246 pairs (i, i + k) at max_pts 2048, on the planted path of 64 cameras of
tools/link_poses_time.py (2000 points, a quarter of the matches wrong, 0.5 px noise; each pair's F is the exact one of its
planted pose).  Both chains, misift_triangulate_tracks_batch and one misift_adjust_bundle_batch run on the device first, as
in tools/bundle_time.py; the filter reads the adjusted cameras and points.
  (a) the call, HIP events on the context stream around it (misift_timer_start / misift_timer_stop_ms), against the
      device-to-host copy of what a host filter needs before it can start: the T + 1 offsets, the O observations, the T
      points and their status, the cameras and d_cam_pair, into pinned memory, events around the seven copies.  The copy
      is given T and O for nothing (a real caller reads the export summary first), and misift_copy_d2h waits for the end
      of each copy.
  (b) the loop: adjust -> filter -> adjust on the filter's outputs against adjust -> adjust, the same num_loops each.
The four take turns within every repetition, so a drift of the machine meets all alike.  Every figure is the median over
--reps repetitions after --warmup.  kernels_ms is the time per call of each launch, the mean over ten more calls with
events around every launch; shares are of their sum.  All nine outputs are compared with the numpy restatement
(tests/filter_cases.expected_filter) at this size before anything is timed.  Prints one JSON line; --out FILE also writes
it there."""
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
import filter_cases as FC  # noqa: E402
import pose_cases as PC  # noqa: E402
import posegraph_cases as G  # noqa: E402
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
    ap.add_argument("--num-loops", type=int, default=5)
    ap.add_argument("--min-obs", type=int, default=6)
    ap.add_argument("--cg-iters", type=int, default=10)
    ap.add_argument("--lambda0", type=float, default=1e-3)
    ap.add_argument("--filter-error", type=float, default=1.5)
    ap.add_argument("--filter-angle-deg", type=float, default=1.0)
    ap.add_argument("--filter-min-views", type=int, default=3)
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
    hold = [pairs[0][1]]                                         # the seed pair is pair 0, the root its first image
    tri = ctx.triangulate_tracks_batch(max_tracks, max_obs, doff, dobs, dsum, nf, dcam, dcam_pair, K, min_views=2,
                                       num_loops=a.num_loops)
    dpts, dstatus = tri[0], tri[2]
    mt, mo = max_tracks, max_obs
    args = dict(min_views=2, min_obs=a.min_obs, max_error=np.inf, lambda0=a.lambda0, orthonormalise=1, hold=hold,
                num_loops=a.num_loops, cg_iters=a.cg_iters)
    adj1 = ctx.adjust_bundle_batch(mt, mo, doff, dobs, dsum, dpts, dstatus, nf, dcam, dcam_pair, K, **args)
    dcam1, dpts1 = adj1[0], adj1[1]
    fargs = dict(max_error=a.filter_error, max_cos=float(np.float32(np.cos(np.deg2rad(a.filter_angle_deg)))),
                 min_views=a.filter_min_views, unique_frames=1)
    sizes = FC.sizes(dict(max_tracks=mt, max_obs=mo))
    outs = {k: ctx.upload(np.full(m, TC.POISON_WORD, np.uint32)) for k, m in sizes.items()}

    def filt():
        ctx.filter_tracks_batch(mt, mo, doff, dobs, dsum, dpts1, dstatus, nf, dcam1, dcam_pair, K, **fargs, **outs)

    # the same answer as the restatement at this size, before anything is timed
    filt()
    ctx.sync()
    case = dict(max_tracks=mt, max_obs=mo, track_offsets=ctx.download(doff, (mt + 1,), np.int32),
                obs=ctx.download(dobs, (mo,), TC.OBS_DTYPE), export_summary=ctx.download(dsum, (8,), np.int32),
                nimages=nf, cam=ctx.download(dcam1, (nf, 12), np.float32),
                cam_pair=ctx.download(dcam_pair, (nf,), np.int32), intrinsics=K,
                points=ctx.download(dpts1, (mt, 4), np.float32), point_status=ctx.download(dstatus, (mt,), np.int32),
                **fargs)
    e = FC.expected_filter(case)
    for k in FC.OUTPUTS:
        assert ctx.download(outs[k], (sizes[k],), np.uint32).tobytes() == e[k].tobytes(), k
    T, O = int(case["export_summary"][2]), int(case["export_summary"][3])

    def events(fn):
        ms = C.c_float()
        ctx.sync()
        capi.check(L.misift_timer_start(ctx.h), "misift_timer_start")
        fn()
        capi.check(L.misift_timer_stop_ms(ctx.h, C.byref(ms)), "misift_timer_stop_ms")
        return ms.value

    # what a host filter reads back first
    reads = ((doff, 4 * (T + 1)), (dobs, 16 * O), (dpts1, 16 * T), (dstatus, 4 * T), (dcam1, 48 * nf), (dcam_pair, 4 * nf),
             (dsum, 32))
    pinned = [capi.PinnedArray((max(b, 4),), np.uint8) for _, b in reads]

    def read_back():
        for (buf, b), dst in zip(reads, pinned):
            capi.check(L.misift_copy_d2h(ctx.h, dst.array.ctypes.data, buf.ptr, b), "misift_copy_d2h")

    adj2 = ctx.adjust_bundle_batch(mt, mo, doff, dobs, dsum, dpts, dstatus, nf, dcam, dcam_pair, K, **args)
    keep = dict(zip(("cam_out", "points_out", "cam_obs", "cam_status", "cam_rms", "point_obs", "history", "cost",
                     "summary"), adj2))

    def adjust_adjust():
        ctx.adjust_bundle_batch(mt, mo, doff, dobs, dsum, dpts, dstatus, nf, dcam, dcam_pair, K, **args, **keep)
        ctx.adjust_bundle_batch(mt, mo, doff, dobs, dsum, keep["points_out"], dstatus, nf, keep["cam_out"], dcam_pair, K,
                                **args, **keep)

    final = dict(keep, cam_out=ctx.zeros(48 * nf), points_out=ctx.zeros(16 * mt))

    def adjust_filter_adjust():
        ctx.adjust_bundle_batch(mt, mo, doff, dobs, dsum, dpts, dstatus, nf, dcam, dcam_pair, K, **args, **keep)
        ctx.filter_tracks_batch(mt, mo, doff, dobs, dsum, keep["points_out"], dstatus, nf, keep["cam_out"], dcam_pair, K,
                                **fargs, **outs)
        ctx.adjust_bundle_batch(mt, mo, outs["track_offsets_out"], outs["obs_out"], outs["export_summary_out"],
                                outs["points_out"], outs["point_status_out"], nf, keep["cam_out"], dcam_pair, K, **args,
                                **final)

    times = {"filter_events_ms": [], "read_back_events_ms": [], "adjust_adjust_events_ms": [],
             "adjust_filter_adjust_events_ms": []}
    for rep in range(a.warmup + a.reps):                         # the four take turns
        t = (events(filt), events(read_back), events(adjust_adjust), events(adjust_filter_adjust))
        if rep >= a.warmup:
            for k, v in zip(times, t):
                times[k].append(v)
    adjust_adjust()                                              # the two loops write the same cost and summary
    ctx.sync()
    cost_aa = ctx.download(keep["cost"], (2,), np.float32)
    members_aa = int(ctx.download(keep["summary"], (8,), np.int32)[2])
    adjust_filter_adjust()
    ctx.sync()
    cost_afa = ctx.download(final["cost"], (2,), np.float32)
    members_afa = int(ctx.download(final["summary"], (8,), np.int32)[2])
    ctx.profile_enable(True)                                     # the launches alone: events around each, a run of its own
    ctx.profile_reset()                                          # behind the timed ones
    for _ in range(10):
        filt()
    ctx.sync()
    kernels = {k: round(v["total_ms"] / 10, 4) for k, v in ctx.profile_read().items() if k.startswith("filter_")}
    ctx.profile_enable(False)
    total_k = sum(kernels.values())
    s = e["summary"].view(np.int32)
    r = {"case": "window %d over %d frames, %d matches per pair, 25 %% wrong, 0.5 px noise, tracks of %d and more" % (
        a.window, nf, n, a.min_len), "pairs": npairs, "tracks": T, "observations": O, "images": nf,
        "filter": dict(fargs, min_angle_deg=a.filter_angle_deg), "summary": s.tolist(),
        "tracks_kept": int(s[0]), "observations_kept": int(s[1]), "reps": a.reps,
        "read_back_bytes": int(sum(b for _, b in reads)), "adjust_num_loops": a.num_loops, "adjust_cg_iters": a.cg_iters,
        "adjust_adjust_rms_px": round(float(np.sqrt(cost_aa[1] / max(members_aa, 1))), 4),
        "adjust_filter_adjust_rms_px": round(float(np.sqrt(cost_afa[1] / max(members_afa, 1))), 4)}
    for k, v in times.items():
        r[k] = round(float(np.median(v)), 4)
        r[k.replace("_ms", "_min_ms")] = round(float(np.min(v)), 4)
        r[k.replace("_ms", "_p10_p90_ms")] = [round(float(x), 4) for x in np.percentile(v, [10, 90])]
    r["kernels_ms"] = kernels
    r["kernel_shares"] = {k: round(v / total_k, 4) for k, v in kernels.items()} if total_k else {}
    r["filter_vs_read_back"] = round(r["filter_events_ms"] / r["read_back_events_ms"], 4)
    r["loop_with_filter_vs_without"] = round(r["adjust_filter_adjust_events_ms"] / r["adjust_adjust_events_ms"], 4)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

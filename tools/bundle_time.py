"""misift_adjust_bundle_batch beside what it replaces, one round of triangulate + refine, on one MI355X (README: device
batches, bundle adjustment).

The README's window: W = 4 over 64 frames, 246 pairs (i, i + k) at max_pts 2048, on the planted path of 64 cameras of
tools/link_poses_time.py (2000 points, a quarter of the matches wrong, 0.5 px noise; each pair's F is the exact one of its
planted pose).  Both chains and misift_triangulate_tracks_batch run on the device first, as in
tools/refine_cameras_time.py: d_cam and d_cam_pair, the offsets, d_obs and the export summary, d_points and
d_point_status.  The root and the other image of the seed pair are held.
  (a) one LM step (num_loops 1) at cg_iters 0, 5 and 10, and num_loops 5 at cg_iters 10: HIP events on the context stream
      around the call (misift_timer_start / misift_timer_stop_ms).
  (b) one round of the parent's method: triangulate, then refine at num_loops 5 in place, events around the two.
The five take turns within every repetition, so a drift of the machine meets all alike.  Every figure is the median over
--reps repetitions after --warmup.  kernels_ms is the time per call of each kind of launch (per-track, per-image, the
scalar workgroup, the trial state, setup and outputs), the mean over ten more calls at num_loops 5 and cg_iters 10 with
events around every launch; shares are of their sum.  All nine outputs are compared with the numpy restatement
(tests/bundle_cases.expected_bundle) at this size before anything is timed.  Prints one JSON line; --out FILE also writes
it there.

--focal times misift_adjust_bundle_focal_batch instead: the plain call, the new call with ngroups 0 (which must give the
plain call's bytes), with all images in one group and with the images dealt to eight groups, the focal given 10 % long
(both compared with their restatement, tests/bundle_focal_cases.expected_focal), taking turns, for one step and for --num-loops.
--radial times misift_adjust_bundle_radial_batch instead: the plain call, the focal call with all images in one group, the
new call on the same input with nothing radial (which must give the focal call's bytes and launches its kernels), with the
one group's coefficient an unknown and with the images dealt to eight groups, all unknown, the observations displaced by a
planted lens (one group compared with its restatement, tests/bundle_radial_cases.expected_radial), taking turns, for one
step and for --num-loops; then misift_undistort_obs_batch beside the device-to-host copy of the observation list it saves.
--parent-json FILE (with --radial) takes the JSON that `bundle_time.py --focal --out FILE` of the parent commit wrote in a
process of its own and puts its one-group figures beside these under "parent_focal_call_in_its_own_process".
--losses times misift_adjust_bundle_robust_batch instead of (a) and (b): the plain call, loss 0 through the new call,
Huber at --huber px and Geman-McClure at --geman-mcclure px without d_obs_weight, and Huber with it (one launch more),
each at num_loops 1 and --num-loops, cg_iters --cg-iters.  The ten take turns within every repetition in one process.  The
two losses are compared with their restatement (tests/bundle_robust_cases.expected_bundle), all ten outputs, and loss 0
with the plain call's, before anything is timed; kernels_ms is then given for the plain call and for each loss."""
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
import bundle_cases as BC  # noqa: E402
import bundle_focal_cases as BF  # noqa: E402
import bundle_radial_cases as BD  # noqa: E402
import bundle_robust_cases as BR  # noqa: E402
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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--losses", action="store_true")
    ap.add_argument("--focal", action="store_true")
    ap.add_argument("--radial", action="store_true")
    ap.add_argument("--parent-json", default="")
    ap.add_argument("--huber", type=float, default=2.0)
    ap.add_argument("--geman-mcclure", type=float, default=4.0)
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
    sizes = BC.sizes(dict(nimages=nf, max_tracks=max_tracks, num_loops=a.num_loops))
    outs = {k: ctx.upload(np.full(m, TC.POISON_WORD, np.uint32)) for k, m in sizes.items()}
    args = dict(min_views=2, min_obs=a.min_obs, max_error=np.inf, lambda0=a.lambda0, orthonormalise=1)

    dweight = ctx.upload(np.full(max_obs, TC.POISON_WORD, np.uint32))

    def adjust(num_loops, cg_iters, loss=None, scale=0.0, weights=False):
        if loss is None:
            ctx.adjust_bundle_batch(max_tracks, max_obs, doff, dobs, dsum, dpts, dstatus, nf, dcam, dcam_pair, K,
                                    hold=hold, num_loops=num_loops, cg_iters=cg_iters, **args, **outs)
        else:
            ctx.adjust_bundle_robust_batch(max_tracks, max_obs, doff, dobs, dsum, dpts, dstatus, nf, dcam, dcam_pair, K,
                                           hold=hold, num_loops=num_loops, cg_iters=cg_iters, loss=loss, loss_scale=scale,
                                           obs_weight=dweight if weights else None, **args, **outs)

    # the same answer as the restatement at this size, before anything is timed
    adjust(a.num_loops, a.cg_iters)
    ctx.sync()
    case = dict(max_tracks=max_tracks, max_obs=max_obs, track_offsets=ctx.download(doff, (max_tracks + 1,), np.int32),
                obs=ctx.download(dobs, (max_obs,), TC.OBS_DTYPE), export_summary=ctx.download(dsum, (8,), np.int32),
                nimages=nf, cam=ctx.download(dcam, (nf, 12), np.float32),
                cam_pair=ctx.download(dcam_pair, (nf,), np.int32), intrinsics=K,
                points=ctx.download(dpts, (max_tracks, 4), np.float32),
                point_status=ctx.download(dstatus, (max_tracks,), np.int32), hold=tuple(hold), num_loops=a.num_loops,
                cg_iters=a.cg_iters, **args)
    e = BC.expected_bundle(case)
    for k in BC.OUTPUTS:
        assert ctx.download(outs[k], (sizes[k],), np.uint32).tobytes() == e[k].tobytes(), k
    P = e["res"]["problem"]

    def events(fn):
        ms = C.c_float()
        ctx.sync()
        capi.check(L.misift_timer_start(ctx.h), "misift_timer_start")
        fn()
        capi.check(L.misift_timer_stop_ms(ctx.h, C.byref(ms)), "misift_timer_stop_ms")
        return ms.value

    def percentiles(r, times):
        for k, v in times.items():
            r[k] = round(float(np.median(v)), 4)
            r[k.replace("_ms", "_min_ms")] = round(float(np.min(v)), 4)
            r[k.replace("_ms", "_p10_p90_ms")] = [round(float(x), 4) for x in np.percentile(v, [10, 90])]

    def launches_of(fn):
        ctx.profile_enable(True)                                 # the launches alone: events around each, a run of its own
        ctx.profile_reset()                                      # behind the timed ones
        for _ in range(10):
            fn()
        ctx.sync()
        read = {k: v for k, v in ctx.profile_read().items() if k.startswith("bundle_")}
        ctx.profile_enable(False)
        return {k: round(v["total_ms"] / 10, 4) for k, v in read.items()}, {k: v["calls"] // 10 for k, v in read.items()}

    r = {"case": "window %d over %d frames, %d matches per pair, 25 %% wrong, 0.5 px noise, tracks of %d and more" % (
        a.window, nf, n, a.min_len), "pairs": npairs, "tracks": int(P.T), "observations": int(P.O), "images": nf,
        "held": hold, "min_obs": a.min_obs, "lambda0": a.lambda0, "summary": e["summary"].view(np.int32).tolist(),
        "reps": a.reps}
    if a.focal:
        # misift_adjust_bundle_focal_batch: the plain call, the new call without a group (the plain call's kernels) and
        # with all images in one group, the given fx, fy 10 % long; the three take turns
        Kf = K.copy()
        Kf[:, :2] *= np.float32(1.1)
        dk, dfocal = ctx.zeros(16 * nf), ctx.zeros(12 * BF.MAX_GROUPS)
        groups = {0: np.zeros(nf, np.int32), 1: np.zeros(nf, np.int32),
                  BF.MAX_GROUPS: (np.arange(nf) % BF.MAX_GROUPS).astype(np.int32)}

        def focal_adjust(num_loops, ngroups):
            ctx.adjust_bundle_focal_batch(max_tracks, max_obs, doff, dobs, dsum, dpts, dstatus, nf, dcam, dcam_pair,
                                          Kf if ngroups else K, groups[ngroups], ngroups=ngroups, hold=hold,
                                          num_loops=num_loops,
                                          cg_iters=a.cg_iters, loss=BR.NONE, intrinsics_out=dk, focal=dfocal, **args, **outs)

        plain = {k: ctx.download(outs[k], (sizes[k],), np.uint32).tobytes() for k in BC.OUTPUTS}
        focal_adjust(a.num_loops, 0)
        ctx.sync()
        assert all(ctx.download(outs[k], (sizes[k],), np.uint32).tobytes() == plain[k] for k in BC.OUTPUTS)
        assert ctx.download(dk, (nf, 4), np.float32).tobytes() == K.tobytes()
        r["focal"] = {"given_focal_factor": 1.1, "cg_iters": a.cg_iters}
        for ng in (1, BF.MAX_GROUPS):
            focal_adjust(a.num_loops, ng)
            ctx.sync()
            x = BF.expected_focal(BF.focal(dict(case, intrinsics=Kf), groups[ng], ng))
            for k in BC.OUTPUTS:
                assert ctx.download(outs[k], (sizes[k],), np.uint32).tobytes() == x[k].tobytes(), (ng, k)
            assert ctx.download(dk, (4 * nf,), np.uint32).tobytes() == x["intrinsics_out"].tobytes()
            assert ctx.download(dfocal, (3 * ng,), np.uint32).tobytes() == x["focal"].tobytes()
            r["focal"]["groups%d" % ng] = {"scale": [round(float(v), 6) for v in x["res"]["scale"][:ng]],
                                          "steps": x["res"]["trace"], "rms_px_after": round(BF.pooled_rms(x["res"]), 4)}
        variants = (("plain", lambda loops: adjust(loops, a.cg_iters)), ("groups0", lambda loops: focal_adjust(loops, 0)),
                    ("group1", lambda loops: focal_adjust(loops, 1)),
                    ("groups8", lambda loops: focal_adjust(loops, BF.MAX_GROUPS)))
        names = ["adjust_%s_loops%d_cg%d_events_ms" % (v[0], loops, a.cg_iters) for loops in (1, a.num_loops)
                 for v in variants]
        times = {k: [] for k in names}
        for rep in range(a.warmup + a.reps):
            t = [events(lambda: v[1](loops)) for loops in (1, a.num_loops) for v in variants]
            if rep >= a.warmup:
                for k, v in zip(names, t):
                    times[k].append(v)
        percentiles(r, times)
        r["kernels_ms"], r["launches_per_call"] = {}, {}
        for v in variants:
            r["kernels_ms"][v[0]], r["launches_per_call"][v[0]] = launches_of(lambda: v[1](a.num_loops))
        for loops in (1, a.num_loops):
            key = "adjust_%%s_loops%d_cg%d_events_ms" % (loops, a.cg_iters)
            r["ratios_loops%d" % loops] = {"groups0_vs_plain": round(r[key % "groups0"] / r[key % "plain"], 4),
                                           "group1_vs_plain": round(r[key % "group1"] / r[key % "plain"], 4),
                                           "groups8_vs_plain": round(r[key % "groups8"] / r[key % "plain"], 4)}
        print(json.dumps(r), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(r, f, indent=1)
        ctx.close()
        return
    if a.radial:
        # misift_adjust_bundle_radial_batch: the given fx, fy 10 % long as under --focal, the observations displaced by a
        # lens of 5 % at the image corner; the five variants take turns
        Kf = K.copy()
        Kf[:, :2] *= np.float32(1.1)
        groups = {1: np.zeros(nf, np.int32), BD.MAX_GROUPS: (np.arange(nf) % BD.MAX_GROUPS).astype(np.int32)}
        kplant = BD.corner_k(dict(intrinsics=K), -0.05)
        lens = BD.distort_obs(dict(case, group=groups[1]), [kplant])["obs"]
        dlens = ctx.upload(lens)
        dk, dfocal, dradial = ctx.zeros(16 * nf), ctx.zeros(12 * BD.MAX_GROUPS), ctx.zeros(12 * BD.MAX_GROUPS)

        def focal_adjust(num_loops):
            ctx.adjust_bundle_focal_batch(max_tracks, max_obs, doff, dlens, dsum, dpts, dstatus, nf, dcam, dcam_pair, Kf,
                                          groups[1], ngroups=1, hold=hold, num_loops=num_loops, cg_iters=a.cg_iters,
                                          loss=BR.NONE, intrinsics_out=dk, focal=dfocal, **args, **outs)

        def radial_adjust(num_loops, ngroups, on):
            ctx.adjust_bundle_radial_batch(max_tracks, max_obs, doff, dlens, dsum, dpts, dstatus, nf, dcam, dcam_pair, Kf,
                                           groups[ngroups], ngroups=ngroups, radial=[on] * ngroups, k0=[0.0] * ngroups,
                                           hold=hold, num_loops=num_loops, cg_iters=a.cg_iters, loss=BR.NONE,
                                           intrinsics_out=dk, focal=dfocal, radial_out=dradial, **args, **outs)

        def words():
            got = {k: ctx.download(outs[k], (sizes[k],), np.uint32).tobytes() for k in BC.OUTPUTS}
            got["intrinsics_out"] = ctx.download(dk, (4 * nf,), np.uint32).tobytes()
            got["focal"] = ctx.download(dfocal, (3,), np.uint32).tobytes()
            return got

        focal_adjust(a.num_loops)
        ctx.sync()
        foc = words()
        radial_adjust(a.num_loops, 1, 0)
        ctx.sync()
        assert words() == foc, "nothing radial: not the focal call's bytes"
        radial_adjust(a.num_loops, 1, 1)
        ctx.sync()
        x = BD.expected_radial(BD.radial(BF.focal(dict(case, obs=lens, intrinsics=Kf), groups[1], 1), [1], [0.0]))
        for k in BC.OUTPUTS:
            assert ctx.download(outs[k], (sizes[k],), np.uint32).tobytes() == x[k].tobytes(), k
        assert ctx.download(dk, (4 * nf,), np.uint32).tobytes() == x["intrinsics_out"].tobytes()
        assert ctx.download(dradial, (3,), np.uint32).tobytes() == x["radial_out"].tobytes()
        r["radial"] = {"given_focal_factor": 1.1, "planted_k": round(float(kplant), 6), "cg_iters": a.cg_iters,
                       "group1": {"k": round(float(x["res"]["coef"][0]), 6), "scale": round(float(x["res"]["scale"][0]), 6),
                                  "steps": x["res"]["trace"], "rms_px_after": round(BD.pooled_rms(x["res"]), 4)}}
        variants = (("plain", lambda loops: adjust(loops, a.cg_iters)), ("focal", focal_adjust),
                    ("radial_none", lambda loops: radial_adjust(loops, 1, 0)),
                    ("radial_group1", lambda loops: radial_adjust(loops, 1, 1)),
                    ("radial_groups8", lambda loops: radial_adjust(loops, BD.MAX_GROUPS, 1)))
        names = ["adjust_%s_loops%d_cg%d_events_ms" % (v[0], loops, a.cg_iters) for loops in (1, a.num_loops)
                 for v in variants]
        times = {k: [] for k in names}
        dund = ctx.zeros(16 * max_obs)
        und, d2h = [], []
        for rep in range(a.warmup + a.reps):
            t = [events(lambda: v[1](loops)) for loops in (1, a.num_loops) for v in variants]
            u = events(lambda: ctx.undistort_obs_batch(max_obs, dlens, dsum, nf, Kf, groups[1], dradial, ngroups=1,
                                                       obs_out=dund))
            ctx.sync()
            t0 = time.perf_counter()                             # a synchronous copy: the host's clock around it
            ctx.download(dlens, (max_obs,), TC.OBS_DTYPE)
            c = 1e3 * (time.perf_counter() - t0)
            if rep >= a.warmup:
                for k, v in zip(names, t):
                    times[k].append(v)
                und.append(u)
                d2h.append(c)
        times["undistort_obs_events_ms"], times["obs_list_to_host_wall_ms"] = und, d2h
        percentiles(r, times)
        r["kernels_ms"], r["launches_per_call"] = {}, {}
        for v in variants:
            r["kernels_ms"][v[0]], r["launches_per_call"][v[0]] = launches_of(lambda: v[1](a.num_loops))
        for loops in (1, a.num_loops):
            key = "adjust_%%s_loops%d_cg%d_events_ms" % (loops, a.cg_iters)
            r["ratios_loops%d" % loops] = {"radial_none_vs_focal": round(r[key % "radial_none"] / r[key % "focal"], 4),
                                           "radial_group1_vs_focal": round(r[key % "radial_group1"] / r[key % "focal"], 4),
                                           "radial_groups8_vs_focal": round(r[key % "radial_groups8"] / r[key % "focal"], 4)}
        if a.parent_json:
            with open(a.parent_json) as f:
                parent = json.load(f)
            own = {k: v for k, v in parent.items() if k.startswith("adjust_group1_")}
            own["kernels_ms"] = parent["kernels_ms"]["group1"]
            r["parent_focal_call_in_its_own_process"] = own
            for loops in (1, a.num_loops):
                lo, hi = own["adjust_group1_loops%d_cg%d_events_p10_p90_ms" % (loops, a.cg_iters)]
                mine = r["adjust_radial_none_loops%d_cg%d_events_ms" % (loops, a.cg_iters)]
                r["ratios_loops%d" % loops]["radial_none_within_parent_p10_p90"] = bool(lo <= mine <= hi)
        print(json.dumps(r), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(r, f, indent=1)
        ctx.close()
        return
    if a.losses:
        variants = (("plain", None, 0.0, False), ("loss0", BR.NONE, 0.0, False), ("huber", BR.HUBER, a.huber, False),
                    ("geman_mcclure", BR.GEMAN_MCCLURE, a.geman_mcclure, False),
                    ("huber_weights", BR.HUBER, a.huber, True))
        r["losses"] = {"huber_px": a.huber, "geman_mcclure_px": a.geman_mcclure, "cg_iters": a.cg_iters}
        # the same answers as the restatements at this size, before anything is timed
        plain = {k: ctx.download(outs[k], (sizes[k],), np.uint32).tobytes() for k in BC.OUTPUTS}
        for name, loss, scale, _ in variants[1:4]:
            adjust(a.num_loops, a.cg_iters, loss, scale, True)
            ctx.sync()
            got = {k: ctx.download(outs[k], (sizes[k],), np.uint32) for k in BC.OUTPUTS}
            got["obs_weight"] = ctx.download(dweight, (max_obs,), np.uint32)
            if loss == BR.NONE:
                assert all(got[k].tobytes() == plain[k] for k in BC.OUTPUTS), name
                continue
            x = BR.expected_bundle(BR.robust(case, loss, scale))
            BR.compare_all(got, x, name)
            w = x["res"]["w"]
            r["losses"][name] = {"steps": x["res"]["trace"], "cg_iterations": [h[3] for h in x["res"]["history"]],
                                 "members_with_w_below_half": int((w < 0.5).sum()),
                                 "rms_px_after": round(BR.pooled_rms(x["res"]), 4)}
        names = ["adjust_%s_loops%d_cg%d_events_ms" % (v[0], loops, a.cg_iters) for loops in (1, a.num_loops)
                 for v in variants]
        times = {k: [] for k in names}
        for rep in range(a.warmup + a.reps):                     # the ten take turns
            t = [events(lambda: adjust(loops, a.cg_iters, v[1], v[2], v[3])) for loops in (1, a.num_loops)
                 for v in variants]
            if rep >= a.warmup:
                for k, v in zip(names, t):
                    times[k].append(v)
        percentiles(r, times)
        r["kernels_ms"], r["launches_per_call"] = {}, {}
        for v in variants:
            r["kernels_ms"][v[0]], r["launches_per_call"][v[0]] = launches_of(
                lambda: adjust(a.num_loops, a.cg_iters, v[1], v[2], v[3]))
        for loops in (1, a.num_loops):
            key = "adjust_%%s_loops%d_cg%d_events_ms" % (loops, a.cg_iters)
            r["ratios_loops%d" % loops] = {
                "loss0_vs_plain": round(r[key % "loss0"] / r[key % "plain"], 4),
                "huber_vs_loss0": round(r[key % "huber"] / r[key % "loss0"], 4),
                "geman_mcclure_vs_loss0": round(r[key % "geman_mcclure"] / r[key % "loss0"], 4),
                "huber_weights_vs_huber": round(r[key % "huber_weights"] / r[key % "huber"], 4)}
        print(json.dumps(r), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(r, f, indent=1)
        ctx.close()
        return

    dround = ctx.upload(case["cam"])                             # the round works in place on a copy of the cameras
    tri_outs = dict(points=ctx.zeros(16 * max_tracks), point_views=ctx.zeros(4 * max_tracks),
                    point_status=ctx.zeros(4 * max_tracks), obs_error=None, summary=ctx.zeros(32))
    ref_outs = dict(cam_obs=ctx.zeros(4 * nf), cam_rms=ctx.zeros(8 * nf), cam_steps=ctx.zeros(4 * nf),
                    cam_status=ctx.zeros(4 * nf), summary=ctx.zeros(32))

    def full_round():
        ctx.triangulate_tracks_batch(max_tracks, max_obs, doff, dobs, dsum, nf, dround, dcam_pair, K, min_views=2,
                                     num_loops=5, **tri_outs)
        ctx.refine_cameras_batch(max_tracks, max_obs, doff, dobs, dsum, tri_outs["points"], tri_outs["point_status"], nf,
                                 dround, dcam_pair, K, hold=hold, min_obs=a.min_obs, num_loops=5, max_error=np.inf,
                                 orthonormalise=1, cam_out=dround, **ref_outs)

    times = {"adjust_loops1_cg0_events_ms": [], "adjust_loops1_cg5_events_ms": [], "adjust_loops1_cg10_events_ms": [],
             "adjust_loops5_cg10_events_ms": [], "round_events_ms": []}
    for rep in range(a.warmup + a.reps):                         # the five take turns
        t = (events(lambda: adjust(1, 0)), events(lambda: adjust(1, 5)), events(lambda: adjust(1, 10)),
             events(lambda: adjust(5, 10)), events(full_round))
        if rep >= a.warmup:
            for k, v in zip(times, t):
                times[k].append(v)
    kernels, launches = launches_of(lambda: adjust(5, 10))
    total_k = sum(kernels.values())
    cost = e["cost"].view(np.float32)
    r.update({"steps": e["res"]["trace"], "cg_iterations": [h[3] for h in e["res"]["history"]],
              "rms_px_before_after": [round(float(np.sqrt(c / max(len(P.slot), 1))), 4) for c in cost]})
    percentiles(r, times)
    r["kernels_ms"] = kernels
    r["launches_per_call"] = launches
    r["kernel_shares"] = {k: round(v / total_k, 4) for k, v in kernels.items()} if total_k else {}
    r["adjust_loops1_cg10_vs_round"] = round(r["adjust_loops1_cg10_events_ms"] / r["round_events_ms"], 4)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

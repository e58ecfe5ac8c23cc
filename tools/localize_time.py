"""misift_describe_points_batch, the int8 match against the scene frame and misift_localize_frames_batch on one MI355X
(README: device batches, localised frames).

Two planted scenes: 863 points (the number of tracks the README's window exports) seen by 7 images each, and 100 000 points
seen by 4 each.  16 query frames of 2000 records: record r of a query shows a random point of the scene (a quarter of the
positions anywhere in the frame, 0.5 px noise on the others) and carries that point's descriptor under its own noise.
  (a) describe, the match (misift_match_pairs_batch_i8, 16 pairs against the one scene frame), localise at num_loops 256
      and 1024, and the three one after another: HIP events on the context stream around each (misift_timer_start /
      misift_timer_stop_ms).
  (b) what a host PnP needs before it can start: the device-to-host copy of the 16 x 2000 rows (576 bytes each), the T
      points (16 bytes each) and their status, into buffers allocated beforehand, on the host clock.
  (c) misift_resect_cameras_batch on 16 images of as many candidates as the queries have (a planted scene of its own, the
      candidates one observation each), at the same num_loops, in the same process.
All take turns within every repetition, so a drift of the machine meets all alike.  Every figure is the median over --reps
repetitions after --warmup, with the 10th and 90th percentiles; kernels_ms is each launch's mean over ten more calls at
num_loops 1024 with events around it.  describe and localise are compared with the numpy restatements
(tests/localize_cases) at the smaller size before anything is timed.  Prints one JSON line per scene; --out FILE also
writes both there."""
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
import batch_util as BU  # noqa: E402
import localize_cases as LC  # noqa: E402
import resect_cases as C6  # noqa: E402
import triangulate_cases as TC  # noqa: E402

f32 = np.float32
NQ, NREC = 16, 2000


def project(cam, K, X):
    R, t = cam
    Xc = X @ R.T + t
    return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], 1)


def scene(npts, views, seed):
    """The describe case of npts points seen by `views` images each, and NQ query frames with their planted cameras."""
    rng = np.random.default_rng(seed)
    ncams = views + NQ
    cams = TC.cameras(ncams, 0.1, rng)
    K = np.array([TC.INTRINSICS[i % 2] for i in range(ncams)], f32)
    R0, t0 = cams[ncams // 2]
    z = rng.uniform(4, 12, npts)
    Xc = np.stack([rng.uniform(-0.2, 0.2, npts) * z, rng.uniform(-0.15, 0.15, npts) * z, z], 1)
    X = ((Xc - t0) @ R0).astype(f32)
    d = np.abs(rng.normal(0, 1, (npts, 128))).astype(f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)

    def rows_of(idx):
        v = d[idx] + rng.normal(0, 0.004, (len(idx), 128)).astype(f32)
        return BU.quantize_np(v / np.linalg.norm(v, axis=1, keepdims=True))

    q = np.concatenate([rows_of(np.arange(npts)) for _ in range(views)])   # frame f, record r: point r
    obs = np.zeros(npts * views, TC.OBS_DTYPE)
    obs["frame"], obs["record"] = np.tile(np.arange(views), npts), np.repeat(np.arange(npts), views)
    pts = np.zeros((npts, 4), f32)
    pts[:, :3] = X
    describe = dict(max_tracks=npts, max_obs=npts * views, track_offsets=(np.arange(npts + 1) * views).astype(np.int32),
                    obs=obs, export_summary=np.array([npts, npts * views, npts, npts * views, views, 0, 0, 0], np.int32),
                    points=pts, point_status=np.zeros(npts, np.int32), q=q, nframes=views,
                    counts=np.full(views, npts, np.int32), offsets=None, stride=npts, max_records=npts * views)
    query, query_q = np.zeros(NQ * NREC, capi.POINT_DTYPE), np.zeros((NQ * NREC, 128), np.int8)
    for i in range(NQ):
        idx = rng.integers(0, npts, NREC)
        px = project(cams[views + i], K[views + i], X[idx].astype(np.float64)) + rng.normal(0, 0.5, (NREC, 2))
        bad = rng.choice(NREC, NREC // 4, replace=False)
        px[bad] = rng.uniform([0, 0], [1920, 1080], (len(bad), 2))
        query["xpos"][i * NREC:(i + 1) * NREC], query["ypos"][i * NREC:(i + 1) * NREC] = px.T.astype(f32)
        query_q[i * NREC:(i + 1) * NREC] = rows_of(idx)
    cam = np.zeros((ncams, 12), f32)
    pair = np.full(ncams, C6.UNSET, np.int32)
    return dict(describe=describe, K=K, query=query, query_q=query_q, cam=cam, cam_pair=pair, ncams=ncams, views=views,
                true=np.array([np.concatenate([R.reshape(9), t]) for R, t in cams]))


def stats(r, times):
    for k, v in times.items():
        r[k] = round(float(np.median(v)), 4)
        r[k.replace("_ms", "_min_ms")] = round(float(np.min(v)), 4)
        r[k.replace("_ms", "_p10_p90_ms")] = [round(float(x), 4) for x in np.percentile(v, [10, 90])]


def run(ctx, a, npts, views, check):
    L = capi.lib()
    sc = scene(npts, views, 300 + views)
    d, K, ncams = sc["describe"], sc["K"], sc["ncams"]
    mt, mo = d["max_tracks"], d["max_obs"]
    ins = LC.describe_inputs(d)
    dev = {k: ctx.upload(v) for k, v in ins.items()}
    douts = {k: ctx.upload(np.full(m, LC.POISON_WORD, np.uint32)) for k, m in LC.describe_sizes(d).items()}
    d_qrecs, d_qq = ctx.upload(sc["query"]), ctx.upload(sc["query_q"])
    d_qcnt = ctx.upload(np.full(NQ, NREC, np.int32))
    rstride = max(NREC, mt)                                      # the pair matcher turns away a pair with n2 > max_pts
    rows, row_counts, matched = ctx.zeros(576 * NQ * rstride), ctx.zeros(4 * NQ), ctx.zeros(4 * NQ)
    pairs = [(i, 0) for i in range(NQ)]
    frames, images = np.arange(NQ, dtype=np.int32), np.arange(views, ncams, dtype=np.int32)
    seeds = np.arange(NQ, dtype=np.uint32) + 1
    mf = NQ * NREC
    proto = dict(frames=frames, max_found=mf)
    louts = {k: ctx.upload(np.full(max(m, 1), LC.POISON_WORD, np.uint32)) for k, m in LC.localize_sizes(proto).items()}
    d_cam, d_pair = ctx.upload(sc["cam"]), ctx.upload(sc["cam_pair"])
    largs = dict(min_score=0.5, max_ambiguity=0.95, thresh=a.thresh, min_inliers=a.min_inliers, only_unset=0, install=0)

    def describe():
        ctx.describe_points_batch(mt, mo, dev["track_offsets"], dev["obs"], dev["export_summary"], dev["points"],
                                  dev["point_status"], dev["q"], d["nframes"], dev["counts"], None, d["stride"],
                                  d["max_records"], **douts)

    def match():
        ctx.match_pairs_batch_i8(pairs, d_qrecs, d_qq, NQ, d_qcnt, None, NREC, recs2=douts["scene_recs"],
                                 q2=douts["scene_q"], nframes2=1, counts2=douts["scene_count"], offsets2=None,
                                 stride2=mt, max_pts=rstride, out=rows, out_counts=row_counts, num_matched=matched)

    def localize(num_loops):
        ctx.localize_frames_batch(rows, NQ, row_counts, None, rstride, mt, dev["export_summary"], dev["points"],
                                  dev["point_status"], ncams, K, frames, images, seeds, NREC, mf, num_loops=num_loops,
                                  cam=d_cam, cam_pair=d_pair, **largs, **louts)

    describe()
    match()
    localize(1024)
    ctx.sync()
    got_rows = ctx.download(rows, (NQ * rstride,), capi.POINT_DTYPE) if check else None
    lcase = dict(rows=got_rows, nframes_rows=NQ, counts=np.full(NQ, NREC, np.int32), offsets=None, stride=rstride,
                 max_tracks=mt, export_summary=d["export_summary"], points=d["points"], point_status=d["point_status"],
                 nimages=ncams, intrinsics=K, frames=frames, images=images, seeds=seeds, max_pts=NREC, num_loops=1024,
                 cam=sc["cam"], cam_pair=sc["cam_pair"], max_found=mf, **largs)
    if check:                                                    # the same answers as the restatements, before timing
        ed = LC.expected_describe(d)
        for k, m in LC.describe_sizes(d).items():
            assert ctx.download(douts[k], (m,), np.uint32).tobytes() == ed[k].tobytes(), k
        el = LC.expected_localize(lcase)
        for k, m in LC.localize_sizes(lcase).items():
            assert ctx.download(louts[k], (m,), np.uint32).tobytes() == el[k].tobytes(), k
    status = ctx.download(louts["res_status"], (NQ,), np.int32)
    cand = ctx.download(louts["res_cand"], (NQ,), np.int32)
    inl = ctx.download(louts["res_inliers"], (NQ,), np.int32)
    cams = ctx.download(louts["res_cam"], (NQ, 12), f32)
    errs = [C6.pose_error(cams[i], sc["true"][views + i]) for i in range(NQ) if status[i] == 0]

    # resect on as many candidates per image, in the same process
    rs = C6.planted(tuple(int(c) for c in cand), 400 + views)
    rcase = rs["case"]
    rdev = {k: ctx.upload(np.ascontiguousarray(rcase[k])) for k in ("track_offsets", "obs", "export_summary", "points",
                                                                    "point_status", "cam", "cam_pair")}
    routs = [ctx.zeros(4 * m) for m in (12 * NQ, NQ, NQ, NQ, 8)]
    rimages = np.arange(NQ, dtype=np.int32)

    def resect(num_loops):
        ctx.resect_cameras_batch(rcase["max_tracks"], rcase["max_obs"], rdev["track_offsets"], rdev["obs"],
                                 rdev["export_summary"], rdev["points"], rdev["point_status"], NQ, rcase["intrinsics"],
                                 rimages, seeds, 4096, num_loops=num_loops, thresh=a.thresh, min_inliers=a.min_inliers,
                                 only_unset=0, install=0, cam=rdev["cam"], cam_pair=rdev["cam_pair"], res_cam=routs[0],
                                 res_cand=routs[1], res_inliers=routs[2], res_status=routs[3], summary=routs[4])

    resect(1024)
    ctx.sync()
    assert ctx.download(routs[1], (NQ,), np.int32).tolist() == cand.tolist()

    def events(fn):
        ms = C.c_float()
        ctx.sync()
        capi.check(L.misift_timer_start(ctx.h), "misift_timer_start")
        fn()
        capi.check(L.misift_timer_stop_ms(ctx.h, C.byref(ms)), "misift_timer_stop_ms")
        return ms.value

    h_rows = np.empty(NQ * NREC, capi.POINT_DTYPE)
    h_pts, h_status = np.empty((mt, 4), f32), np.empty(mt, np.int32)

    def copy_back():
        ctx.sync()
        t0 = time.perf_counter()
        for i in range(NQ):                                      # the rows of a pair lie rstride records apart
            capi.check(L.misift_copy_d2h(ctx.h, h_rows.ctypes.data + 576 * NREC * i, rows.ptr + 576 * rstride * i,
                                         576 * NREC), "misift_copy_d2h")
        for h, dv, nbytes in ((h_pts, dev["points"], 16 * mt), (h_status, dev["point_status"], 4 * mt)):
            capi.check(L.misift_copy_d2h(ctx.h, h.ctypes.data, dv.ptr, nbytes), "misift_copy_d2h")
        return (time.perf_counter() - t0) * 1e3

    def three():
        describe()
        match()
        localize(1024)

    turns = (("describe_events_ms", lambda: events(describe)), ("match_i8_events_ms", lambda: events(match)),
             ("localize_loops256_events_ms", lambda: events(lambda: localize(256))),
             ("localize_loops1024_events_ms", lambda: events(lambda: localize(1024))),
             ("describe_match_localize1024_events_ms", lambda: events(three)),
             ("resect_loops256_events_ms", lambda: events(lambda: resect(256))),
             ("resect_loops1024_events_ms", lambda: events(lambda: resect(1024))), ("inputs_d2h_ms", copy_back))
    times = {k: [] for k, _ in turns}
    for rep in range(a.warmup + a.reps):                         # all take turns
        for k, fn in turns:
            v = fn()
            if rep >= a.warmup:
                times[k].append(v)
    ctx.profile_enable(True)                                     # the launches alone: events around each, a run of its own
    ctx.profile_reset()
    for _ in range(10):
        describe()
        localize(1024)
        resect(1024)
    ctx.sync()
    kernels = {k: round(v["total_ms"] / max(v["calls"], 1), 4) for k, v in ctx.profile_read().items()}
    ctx.profile_enable(False)
    O = mo
    moved = 128 * O + 16 * O + 704 * mt                          # rows read, slots read, per point: 128 + 576 written
    r = {"case": "%d points seen by %d images each, %d query frames of %d records, 25 %% wrong, 0.5 px noise" % (
        npts, views, NQ, NREC), "points": mt, "observations": O, "queries": NQ, "records_per_query": NREC,
        "thresh_px": a.thresh, "min_inliers": a.min_inliers, "reps": a.reps, "checked_against_restatement": bool(check),
        "describe_summary": ctx.download(douts["summary"], (8,), np.int32).tolist(),
        "localize_summary": ctx.download(louts["summary"], (8,), np.int32).tolist(),
        "candidates_per_query_median": int(np.median(cand)),
        "inlier_share_median": round(float(np.median(inl / np.maximum(cand, 1))), 4),
        "localised_of_queries": [int((status == 0).sum()), NQ],
        "rotation_error_rad_max": round(float(max(e[0] for e in errs)), 6) if errs else None,
        "centre_error_max": round(float(max(e[1] for e in errs)), 6) if errs else None,
        "d2h_bytes": int(h_rows.nbytes + 20 * mt), "describe_bytes_moved": int(moved)}
    stats(r, times)
    r["kernels_ms"] = kernels
    r["describe_gb_per_s"] = round(moved / (r["describe_events_ms"] * 1e-3) / 1e9, 2)
    lk = sum(kernels.get(k, 0.0) for k in ("localize_gather", "localize_solve", "localize_count", "localize_pick",
                                           "localize_emit"))
    rk = sum(kernels.get(k, 0.0) for k in ("resect_gather", "resect_solve", "resect_count", "resect_pick"))
    r["localize_kernels_sum_ms"], r["resect_kernels_sum_ms"] = round(lk, 4), round(rk, 4)
    r["gather_plus_emit_minus_resect_gather_ms"] = round(kernels.get("localize_gather", 0.0) +
                                                         kernels.get("localize_emit", 0.0) -
                                                         kernels.get("resect_gather", 0.0), 4)
    for loops in (256, 1024):
        r["localize_loops%d_vs_d2h" % loops] = round(r["localize_loops%d_events_ms" % loops] / r["inputs_d2h_ms"], 5)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--thresh", type=float, default=4.0)
    ap.add_argument("--min-inliers", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0)
    out = {"window": run(ctx, a, 863, 7, True), "large": run(ctx, a, 100000, 4, False)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

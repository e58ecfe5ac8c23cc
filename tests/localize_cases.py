"""misift_describe_points_batch and misift_localize_frames_batch: expected_describe and expected_localize, the numpy
restatements of the definitions in include/misift.h, the wrappers of the library's host hooks, and the cases of their
tests (test_localize_cpu.py pins the restatements to the hooks and asserts the premises of the cases,
test_gpu_localize.py holds the device to them byte for byte).  The draw, the solve, the count and the pick are
resect_cases', the member test refine_cases'.  A localise case is mostly a resect case turned into match rows
(from_resect): row r of the frame of image i is the r-th candidate resect gathers for i, so both calls must give the same
camera.  No GPU in here, and cudasift_amd.capi is imported inside functions only."""
import numpy as np

import refine_cases as RC
import resect_cases as C
import triangulate_cases as TC
from test_fundamental_cpu import f32

POISON_WORD = TC.POISON_WORD
POISON_BYTE = POISON_WORD & 0xff
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
OBS_DTYPE = TC.OBS_DTYPE
GATES = (0.85, 0.95)
DESCRIBE_OUTPUTS = ("scene_q", "scene_recs", "scene_count", "point_members", "summary")
LOCALIZE_OUTPUTS = C.OUTPUTS + ("found_offsets", "found_obs", "found_summary", "found_points", "found_views",
                                "found_status", "found_map")


def point_dtype():
    from cudasift_amd import capi
    return capi.POINT_DTYPE


# ---- describe: the definition restated

def frame_layout(case):
    """Per frame (n, base, takes part)."""
    out = []
    for f in range(case["nframes"]):
        n = max(int(case["counts"][f]), 0)
        base = int(case["offsets"][f]) if case["offsets"] is not None else f * case["stride"]
        out.append((n, base, n == 0 or (base >= 0 and base + n <= case["max_records"])))
    return out


def describe_sizes(case):
    mt = case["max_tracks"]
    return dict(scene_q=32 * mt, scene_recs=144 * mt, scene_count=1, point_members=mt, summary=8)


def expected_describe(case):
    """The five outputs as uint32 arrays of exactly the stated sizes; what the call leaves untouched is POISON_WORD."""
    mt = case["max_tracks"]
    T, O = RC.counts(case)
    lay = frame_layout(case)
    q = np.asarray(case["q"], np.int8).reshape(-1, 128)
    offs = np.asarray(case["track_offsets"], np.int64)
    obs = case["obs"]
    pts = np.asarray(case["points"], f32).reshape(-1, 4)
    out = {k: np.full(n, POISON_WORD, np.uint32) for k, n in describe_sizes(case).items()}
    scene_q = out["scene_q"].view(np.int8).reshape(mt, 128)
    recs = out["scene_recs"].reshape(mt, 144)
    members = out["point_members"].view(np.int32)
    summary = np.zeros(8, np.int64)
    for t in range(T):
        off, end = int(offs[t]), int(offs[t + 1])
        valid = 0 <= off <= end <= O
        rows = []
        if valid:
            for o in range(off, end):
                f, r = int(obs["frame"][o]), int(obs["record"][o])
                if 0 <= f < case["nframes"] and lay[f][2] and 0 <= r < lay[f][0]:
                    rows.append(lay[f][1] + r)
                else:
                    summary[3] += 1
        m = len(rows)
        desc = valid and m > 0 and int(case["point_status"][t]) == 0 and bool(np.isfinite(pts[t, :3]).all())
        scene_q[t] = 0
        recs[t] = 0
        if desc:
            s = q[rows].astype(np.int64).sum(0)
            scene_q[t] = ((2 * s + m) // (2 * m)).astype(np.int8)          # bytes in [0, 127]: floor == C's division
            recs[t, :3] = pts[t, :3].view(np.uint32)
            summary[1] += 1
            summary[2] += m
        members[t] = m
    summary[0] = T
    out["scene_count"][0] = T
    out["summary"] = summary.astype(np.int32).view(np.uint32)
    return out


def hook_describe(case):
    """The library's host hook on poisoned outputs of exactly the stated sizes."""
    from cudasift_amd import capi
    ins = describe_inputs(case)
    outs = {k: np.full(n, POISON_WORD, np.uint32) for k, n in describe_sizes(case).items()}
    rc = capi.lib().misift_test_describe_points(
        case["max_tracks"], case["max_obs"], ins["track_offsets"].ctypes.data, ins["obs"].ctypes.data,
        ins["export_summary"].ctypes.data, ins["points"].ctypes.data, ins["point_status"].ctypes.data,
        ins["q"].ctypes.data, case["nframes"], ins["counts"].ctypes.data,
        ins["offsets"].ctypes.data if case["offsets"] is not None else None, case["stride"], case["max_records"],
        *[outs[k].ctypes.data for k in DESCRIBE_OUTPUTS])
    assert rc == 0, capi.lib().misift_last_error()
    return outs


def describe_inputs(case):
    """The inputs at exactly the sizes the call states (numpy's allocations of this size are 16-byte aligned)."""
    mt, mo = case["max_tracks"], case["max_obs"]
    ins = dict(track_offsets=np.ascontiguousarray(case["track_offsets"][:mt + 1], np.int32),
               obs=np.ascontiguousarray(case["obs"][:mo]), export_summary=np.ascontiguousarray(case["export_summary"]),
               points=np.ascontiguousarray(case["points"], f32).reshape(-1, 4),
               point_status=np.ascontiguousarray(case["point_status"], np.int32),
               q=np.ascontiguousarray(case["q"], np.int8).reshape(-1, 128),
               counts=np.ascontiguousarray(case["counts"], np.int32),
               offsets=np.ascontiguousarray(case["offsets"] if case["offsets"] is not None else [0], np.int32))
    assert len(ins["track_offsets"]) == mt + 1 and len(ins["obs"]) == mo and len(ins["points"]) == mt
    assert len(ins["q"]) == case["max_records"] and len(ins["counts"]) == max(case["nframes"], 1)
    return ins


# ---- describe: cases

def describe_case(lengths, seed=1, packed=False, slack_tracks=2, slack_obs=5, frame_sizes=(37, 0, 64, 21, 50), q=None):
    """Tracks of the given numbers of observations over a batch of len(frame_sizes) frames; every observation names a
    random record of a random non-empty frame, so records repeat within a track (their rows count once each)."""
    rng = np.random.default_rng(seed)
    sizes = np.array(frame_sizes, np.int32)
    nf = len(sizes)
    if packed:
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32)
        stride, max_records = -1, int(sizes.sum()) + 3
    else:
        offsets, stride = None, int(sizes.max()) + 1
        max_records = stride * nf
    T, O = len(lengths), int(sum(lengths))
    mt, mo = max(T + slack_tracks, 1), max(O + slack_obs, 1)
    offs = np.full(mt + 1, POISON_WORD, np.uint32).view(np.int32)
    offs[:T + 1] = np.concatenate([[0], np.cumsum(lengths)])
    obs = np.zeros(mo, OBS_DTYPE)
    usable = np.nonzero(sizes > 0)[0]
    obs["frame"] = rng.choice(usable, mo)
    obs["record"] = (rng.random(mo) * sizes[obs["frame"]]).astype(np.int32)
    obs["xpos"], obs["ypos"] = rng.uniform(0, 1000, (2, mo)).astype(f32)
    pts = rng.normal(0, 3, (mt, 4)).astype(f32)
    q = rng.integers(0, 128, (max_records, 128)).astype(np.int8) if q is None else q
    return dict(max_tracks=mt, max_obs=mo, track_offsets=offs, obs=obs,
                export_summary=np.array([T, O, T, O, max(list(lengths) + [0]), 0, 0, 0], np.int32), points=pts,
                point_status=np.zeros(mt, np.int32), q=q, nframes=nf, counts=sizes, offsets=offsets, stride=stride,
                max_records=max_records)


LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 301)   # either side of a turn of 8 and of the lane groups


def hostile_describe_case(packed):
    case = describe_case(LENGTHS + (6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6), seed=5, packed=packed)
    T, O = RC.counts(case)
    offs, obs = case["track_offsets"].copy(), case["obs"].copy()
    st, pts, counts = case["point_status"].copy(), case["points"].copy(), case["counts"].copy()
    first = int(offs[len(LENGTHS)])                              # the tracks of six
    fr, rec = obs["frame"], obs["record"]
    fr[first], fr[first + 1], fr[first + 2], fr[first + 3] = -1, case["nframes"], INT_MAX, INT_MIN
    rec[first + 6], rec[first + 7], rec[first + 8] = -1, counts[fr[first + 7]], INT_MAX
    rec[first + 9] = INT_MIN
    st[len(LENGTHS) + 2], st[len(LENGTHS) + 3] = 1, 4
    pts[len(LENGTHS) + 4, 0], pts[len(LENGTHS) + 5, 2], pts[len(LENGTHS) + 6, 1] = np.nan, np.inf, -np.inf
    pts[len(LENGTHS) + 7, 3] = np.nan                            # the fourth word is not looked at
    offs[len(LENGTHS) + 9] = offs[len(LENGTHS) + 8] - 3          # overlaps the track before it and makes it descend
    offs[T] = O + 4                                              # the last track passes O
    case.update(track_offsets=offs, obs=obs, point_status=st, points=pts)
    return case


def bad_frames_case(packed):
    """A count of -1, and a frame pushed outside max_records: their observations do not contribute."""
    case = describe_case((3, 5, 8, 13, 21, 34), seed=6, packed=packed)
    counts = case["counts"].copy()
    counts[3] = -1
    if packed:
        offsets = case["offsets"].copy()
        offsets[4] = case["max_records"] - int(counts[4]) + 1
        case.update(offsets=offsets)
    else:
        counts[4] = case["stride"] + 1                           # the last frame reaches past max_records
    case.update(counts=counts)
    return case


def ties_case():
    """Every byte a tie: tracks of two rows whose bytes differ by one (the mean rounds up), and 301 rows of all 127."""
    lengths = (2, 2, 301, 3)
    case = describe_case(lengths, seed=7, frame_sizes=(2, 2, 301, 3))
    q = np.zeros((case["max_records"], 128), np.int8)
    s = case["stride"]
    q[0], q[1] = 1, 2                                            # frame 0
    q[s], q[s + 1] = np.arange(128) % 127, np.arange(128) % 127 + 1
    q[2 * s:2 * s + 301] = 127
    q[3 * s], q[3 * s + 1], q[3 * s + 2] = 1, 1, 2               # 4 / 3 -> 1, and 5 / 3 -> 2 below
    q[3 * s + 2, 64:] = 3
    obs = case["obs"].copy()
    at = 0
    for f, n in enumerate(lengths):
        obs["frame"][at:at + n], obs["record"][at:at + n] = f, np.arange(n)
        at += n
    case.update(q=q, obs=obs)
    return case


DESCRIBE_GPU_CASES = ("T 0", "T 1", "T 63", "T 64", "T 65", "T 257", "lengths padded", "lengths packed",
                      "hostile padded", "hostile packed", "bad frames padded", "bad frames packed", "ties",
                      "T -1", "T below", "T beyond", "T INT_MAX O INT_MAX", "O below", "O -5", "T INT_MIN O INT_MIN")
_MEMO = {}


def describe_gpu_cases():
    if "describe" in _MEMO:
        return _MEMO["describe"]
    out = {}
    rng = np.random.default_rng(3)
    for T in (0, 1, 63, 64, 65, 257):
        out["T %d" % T] = describe_case(tuple(rng.integers(0, 7, T).tolist()), seed=10 + T, packed=T % 2 == 1)
    out["lengths padded"] = describe_case(LENGTHS, seed=2)
    out["lengths packed"] = describe_case(LENGTHS, seed=2, packed=True)
    for packed in (False, True):
        out["hostile %s" % ("packed" if packed else "padded")] = hostile_describe_case(packed)
        out["bad frames %s" % ("packed" if packed else "padded")] = bad_frames_case(packed)
    out["ties"] = ties_case()
    base = out["lengths padded"]
    T0, O0 = RC.counts(base)
    for name, T, O in (("T -1", -1, O0), ("T below", 9, O0), ("T beyond", base["max_tracks"] + 65, 10 ** 9),
                       ("T INT_MAX O INT_MAX", INT_MAX, INT_MAX), ("O below", T0, 100), ("O -5", T0, -5),
                       ("T INT_MIN O INT_MIN", INT_MIN, INT_MIN)):
        out[name] = RC.with_counts(base, T, O)
    assert sorted(out) == sorted(DESCRIBE_GPU_CASES)
    _MEMO["describe"] = out
    return out


# ---- localise: the definition restated

def frame_rows(case, f):
    """The rows of frame f, or None when it holds more than max_pts."""
    c = int(case["counts"][f])
    if c > case["max_pts"]:
        return None
    base = int(case["offsets"][f]) if case["offsets"] is not None else f * case["stride"]
    return case["rows"][base:base + max(c, 0)]


def candidates(rows, T, points, point_status, min_score, max_ambiguity):
    """Step 2: (row indices, tracks, xy (n, 2), X (n, 3)) of the candidates in ascending row order."""
    pts = np.asarray(points, f32).reshape(-1, 4)
    st = np.asarray(point_status, np.int32)
    with np.errstate(invalid="ignore"):
        ok = (rows["score"] > f32(min_score)) & (rows["ambiguity"] < f32(max_ambiguity))
    t = rows["match"].astype(np.int64)
    ok &= (t >= 0) & (t < T)
    tc = np.where(ok, t, 0)
    if T > 0:
        ok &= (st[tc] == 0) & np.isfinite(pts[tc, :3]).all(1)
    ok &= np.isfinite(rows["xpos"]) & np.isfinite(rows["ypos"])
    r = np.nonzero(ok)[0]
    return r, t[r], np.stack([rows["xpos"][r], rows["ypos"][r]], 1).astype(f32), pts[t[r], :3]


def inlier_mask(cam, k4, X, xy, thresh, dt=f32):
    """Step 5 per candidate under one camera (resect_cases.count_inliers, one hypothesis, not summed)."""
    k = np.asarray(k4, f32).astype(dt)
    X, xy = np.asarray(X, f32).astype(dt), np.asarray(xy, f32).astype(dt)
    thresh2 = f32(thresh) * f32(thresh) if dt is f32 else dt(f32(thresh)) * dt(f32(thresh))
    with np.errstate(all="ignore"):
        c = [dt(v) for v in cam]
        _, _, zc, _, _, _, ru, rv = RC.view(c, k, X, xy[:, 0], xy[:, 1], dt)
        front = zc > 0
        return front if np.isinf(thresh2) else front & (ru * ru + rv * rv < thresh2)


def expected_loc_entry(case, e, dt=f32):
    i = int(case["images"][e])
    out = dict(cam=np.zeros(12, dt), cand=0, inliers=0, status=C.OK, image=i, finds=None, search=None)
    if case["only_unset"] and int(case["cam_pair"][i]) != C.UNSET:
        out["status"] = C.SKIPPED
        return out
    rows = frame_rows(case, int(case["frames"][e]))
    if rows is None:
        out["status"] = C.OVER
        return out
    T = RC.counts(dict(case, max_obs=1))[0]
    r, t, xy, X = candidates(rows, T, case["points"], case["point_status"], case["min_score"], case["max_ambiguity"])
    n = out["cand"] = len(r)
    if n < max(6, case["min_inliers"]):
        out["status"] = C.FEW_CAND
        return out
    memo = case.setdefault("memo_localize", {})
    key = (e, int(case["frames"][e]), i, int(case["seeds"][e]), case["num_loops"], float(case["thresh"]), dt)
    if key not in memo:
        memo[key] = C.search(int(case["seeds"][e]), case["intrinsics"][i], X, xy, case["num_loops"], case["thresh"], dt)
    s = out["search"] = memo[key]
    out["inliers"] = s["inliers"]
    if s["inliers"] < case["min_inliers"]:
        out["status"] = C.NO_MODEL
        return out
    out["cam"] = s["cams"][s["index"]].copy()
    mask = inlier_mask(out["cam"], case["intrinsics"][i], X, xy, case["thresh"], dt)
    assert int(mask.sum()) == s["inliers"]
    out["finds"] = (r[mask], t[mask], xy[mask])
    return out


def localize_sizes(case):
    n, m = len(case["frames"]), case["max_found"]
    return dict(res_cam=12 * n, res_cand=n, res_inliers=n, res_status=n, summary=8, found_offsets=m + 1,
                found_obs=4 * m, found_summary=8, found_points=4 * m, found_views=m, found_status=m, found_map=m)


def expected_localize(case):
    """The twelve outputs as uint32 arrays of exactly the stated sizes (untouched words are POISON_WORD), cam and cam_pair
    as the call leaves them, and the per-entry dicts under 'entries'."""
    ents = [expected_loc_entry(case, e) for e in range(len(case["frames"]))]
    cam = np.ascontiguousarray(case["cam"], f32).reshape(-1, 12).copy()
    pair = np.ascontiguousarray(case["cam_pair"], np.int32).copy()
    pts = np.asarray(case["points"], f32).reshape(-1, 4)
    summary = np.zeros(8, np.int32)
    summary[0] = RC.counts(dict(case, max_obs=1))[0]
    mf = case["max_found"]
    out = {k: np.full(n, POISON_WORD, np.uint32) for k, n in localize_sizes(case).items()}
    fobs = out["found_obs"].view(OBS_DTYPE)
    fpts = out["found_points"].reshape(-1, 4)
    a = 0
    for x in ents:
        summary[(1, 3, 4, 5, 6)[x["status"]]] += 1
        if x["status"] != C.OK:
            continue
        summary[2] += x["inliers"]
        if case["install"]:
            cam[x["image"]], pair[x["image"]] = x["cam"].astype(f32), C.RESECTED
        for r, t, xy in zip(*x["finds"]):
            if a < mf:
                out["found_offsets"][a] = a
                fobs[a] = (x["image"], r, xy[0], xy[1])
                out["found_map"][a] = t
                fpts[a] = pts[t].view(np.uint32)
                out["found_views"][a], out["found_status"][a] = 1, 0
            a += 1
    N, Tp = a, min(a, mf)
    out["found_offsets"][Tp] = Tp
    out["found_summary"] = np.array([N, N, Tp, Tp, 1 if Tp else 0, 0, 0, 0], np.int32).view(np.uint32)
    summary[7] = Tp
    out["res_cam"] = np.array([x["cam"] for x in ents], f32).reshape(-1).view(np.uint32)
    for k in ("cand", "inliers", "status"):
        out["res_" + k] = np.array([x[k] for x in ents], np.int32).view(np.uint32)
    out["summary"] = summary.view(np.uint32)
    out.update(cam=cam.reshape(-1).view(np.uint32), cam_pair=pair.view(np.uint32), entries=ents, N=N)
    return out


def hook_candidates(rows, T, points, point_status, min_score, max_ambiguity):
    """The library's candidate list of one frame of rows: (row indices, tracks, xyXYZ (n, 5))."""
    from cudasift_amd import capi
    rows = np.ascontiguousarray(rows)
    n = len(rows)
    pts = np.ascontiguousarray(points, f32).reshape(-1, 4)
    st = np.ascontiguousarray(point_status, np.int32)
    out5, out_row, out_t = np.full((max(n, 1), 5), 3.5, f32), np.full(max(n, 1), -77, np.int32), np.full(max(n, 1), -77, np.int32)
    cnt = np.full(1, -77, np.int32)
    rc = capi.lib().misift_test_localize_candidates(rows.ctypes.data if n else None, n, T, pts.ctypes.data,
                                                    st.ctypes.data, min_score, max_ambiguity, out5.ctypes.data,
                                                    out_row.ctypes.data, out_t.ctypes.data, cnt.ctypes.data)
    assert rc == 0
    k = int(cnt[0])
    return out_row[:k], out_t[:k], out5[:k]


# ---- localise: cases

def hostile_rows(rng, T, bad_points, min_score, max_ambiguity):
    """Rows that are no candidates, one per rule: the gates exactly met and NaN, match outside [0, T), points that failed
    or are not finite, positions that are not finite."""
    rows = np.zeros(12 + len(bad_points), point_dtype())
    rows["xpos"], rows["ypos"] = rng.uniform(0, 1000, (2, len(rows))).astype(f32)
    rows["score"], rows["ambiguity"] = 0.99, 0.5
    rows["match"] = rng.integers(0, max(T, 1), len(rows))
    rows["score"][0], rows["ambiguity"][1] = min_score, max_ambiguity
    rows["score"][2], rows["ambiguity"][3] = np.nan, np.nan
    rows["match"][4:8] = [-1, T, INT_MIN, INT_MAX]
    rows["xpos"][8], rows["ypos"][9], rows["xpos"][10], rows["ypos"][11] = np.nan, np.inf, -np.inf, np.nan
    rows["match"][12:] = bad_points
    return rows


def from_resect(rcase, images=None, packed=False, hostile=False, max_pts=None, max_found=None, slack_found=3,
                counts=None, **kw):
    """A localise case from a resect case: frame e holds, in slot order, the candidates resect gathers for images[e] (score
    and ambiguity inside the gates, match = the owner of the slot); with `hostile`, rows that are no candidates are mixed
    in, and a few points are spoiled that no candidate names (which resect's candidates never do either)."""
    images = list(rcase["images"] if images is None else images)
    rng = np.random.default_rng(17)
    keys = RC.candidate_keys(rcase)
    T = RC.counts(rcase)[0]
    pts = np.asarray(rcase["points"], f32).reshape(-1, 4).copy()
    st = np.asarray(rcase["point_status"], np.int32).copy()
    frames, cands = [], []
    for i in images:
        slots, X, xy = RC.image_candidates(rcase, i, keys)
        rows = np.zeros(len(slots), point_dtype())
        rows["xpos"], rows["ypos"] = xy[:, 0], xy[:, 1]
        rows["score"], rows["ambiguity"] = 0.99, 0.5
        rows["match"] = keys[1][slots]
        frames.append(rows)
        cands.append(len(slots))
    if hostile:
        named = np.concatenate([f["match"] for f in frames] + [np.zeros(0, np.int32)])
        free = np.setdiff1d(np.arange(T), named)[:4]
        assert len(free) == 4
        st[free[0]], st[free[1]] = 1, 4
        pts[free[2], 1], pts[free[3], 2] = np.nan, np.inf
        for e, rows in enumerate(frames):
            bad = hostile_rows(rng, T, free, GATES[0], GATES[1])
            at = np.sort(rng.integers(0, len(rows) + 1, len(bad)))
            frames[e] = np.insert(rows, at, bad)
    sizes = np.array([len(f) for f in frames] + [0], np.int32)   # one more frame, empty and unused
    nf = len(sizes)
    if packed:
        offsets, stride = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32), -1
        total = int(sizes.sum()) + 1
        base = offsets
    else:
        stride = int(sizes.max()) + 2
        offsets, total = None, stride * nf
        base = np.arange(nf) * stride
    allrows = np.zeros(total, point_dtype())
    allrows["match"], allrows["score"] = 0, 0.99                 # beyond the counts: candidates if they were read
    allrows["ambiguity"] = 0.1
    for f, rows in enumerate(frames):
        allrows[base[f]:base[f] + len(rows)] = rows
    if counts is not None:
        sizes = np.array(counts, np.int32)
    nsel = len(images)
    mp = int(max(sizes.max(), 1)) if max_pts is None else max_pts
    case = dict(rows=allrows, nframes_rows=nf, counts=sizes, offsets=offsets, stride=stride,
                max_tracks=rcase["max_tracks"], export_summary=rcase["export_summary"], points=pts, point_status=st,
                nimages=rcase["nimages"], intrinsics=rcase["intrinsics"], frames=np.arange(nsel, dtype=np.int32),
                images=np.asarray(images, np.int32), seeds=np.asarray(rcase["seeds"], np.uint32), max_pts=mp,
                min_score=GATES[0], max_ambiguity=GATES[1], num_loops=rcase["num_loops"], thresh=rcase["thresh"],
                min_inliers=rcase["min_inliers"], only_unset=rcase["only_unset"], install=rcase["install"],
                cam=rcase["cam"], cam_pair=rcase["cam_pair"], resect=rcase, resect_cand=cands)
    case.update(kw)
    if max_found is None:
        max_found = max(expected_localize(dict(case, max_found=1))["N"] + slack_found, 1)
    case["max_found"] = max_found
    return case


def loc_variant(case, **kw):
    out = dict(case, **kw)
    out.pop("memo_localize", None)
    return out


RESECT_TWINS = ("candidates 0 5 6", "candidates 7 511 512", "candidates 513 1025", "num_loops 1", "num_loops 63",
                "num_loops 64", "num_loops 65", "num_loops 100", "nsel 0", "nsel 3 of different status",
                "min_inliers count -1", "min_inliers count +0", "min_inliers count +1", "only_unset, install 0",
                "only_unset, install 1", "install over set cameras", "seed a", "seed b", "tie", "thresh inf",
                "T 150 O 226", "T -1 O 226", "T 2147483647 O 2147483647")
LOCALIZE_GPU_CASES = tuple("resect: " + k for k in RESECT_TWINS) + (
    "hostile padded", "hostile packed", "max_pts 1030", "max_pts one below n", "count -1", "all statuses",
    "max_found N-1", "max_found N", "max_found N+1", "max_found cuts an entry", "max_found 1", "several rows to one point")


def localize_gpu_cases():
    if "localize" in _MEMO:
        return _MEMO["localize"]
    R = C.gpu_cases()
    out = {}
    for k in RESECT_TWINS:
        out["resect: " + k] = from_resect(R[k], packed=len(out) % 2 == 1)
    small = C.resect_case(C.small_scene()["case"], [0, 1, 3], num_loops=48)
    out["hostile padded"] = from_resect(small, hostile=True)
    out["hostile packed"] = from_resect(small, hostile=True, packed=True)
    edge = C.resect_case(C.edge_scene()["case"], [5, 6, 7], num_loops=16, max_cand=2000)
    out["max_pts 1030"] = from_resect(edge, max_pts=1030)
    out["max_pts one below n"] = from_resect(edge, max_pts=1024)
    out["count -1"] = from_resect(small, counts=[40, -1, 90, 0])
    # status 0 (images 0 and 1), 1 (ten rows), 2 (24 rows, fewer than 20 of them planted), 3 (a camera is there), 4 (over
    # max_pts)
    sc = C.planted((40, 60, 24, 90, 10, 30), 76)
    cam = sc["case"]["cam"].copy()
    cam[5] = sc["true"][5].astype(f32)
    pair = np.array([C.UNSET] * 5 + [C.ROOT], np.int32)
    mixed = C.resect_case(dict(sc["case"], cam=cam, cam_pair=pair), [0, 4, 2, 5, 3, 1], num_loops=48, only_unset=1,
                          install=1, min_inliers=20)
    out["all statuses"] = from_resect(mixed, max_pts=64)
    two = from_resect(small, packed=True)
    N = expected_localize(two)["N"]
    first = expected_localize(two)["entries"][0]["inliers"]
    assert 0 < first < N
    for name, mf in (("N-1", N - 1), ("N", N), ("N+1", N + 1), ("cuts an entry", first + 2), ("1", 1)):
        out["max_found " + name] = loc_variant(two, max_found=mf)
    many = from_resect(small)
    rows = many["rows"].copy()
    r0 = int(expected_localize(many)["entries"][0]["finds"][0][0])          # a find of frame 0 (which starts at row 0)
    for r in (r0 + 1, r0 + 2):                                   # two more rows see the same point at the same place
        rows[r] = rows[r0]
    out["several rows to one point"] = loc_variant(many, rows=rows)
    assert sorted(out) == sorted(LOCALIZE_GPU_CASES)
    _MEMO["localize"] = out
    return out


# ---- the chain: a window of cameras, a new image, the merge

def found_scene(case, out):
    """The finds (uint32 outputs of expected_localize or of the device) as scene A of merge_cases, under the cameras the
    call left behind."""
    mf = case["max_found"]
    return dict(max_tracks=mf, max_obs=mf, track_offsets=out["found_offsets"].view(np.int32).copy(),
                obs=out["found_obs"].view(OBS_DTYPE).copy(), export_summary=out["found_summary"].view(np.int32).copy(),
                points=out["found_points"].view(f32).reshape(mf, 4).copy(),
                point_views=out["found_views"].view(np.int32).copy(),
                point_status=out["found_status"].view(np.int32).copy(), nimages=case["nimages"],
                cam=out["cam"].view(f32).reshape(-1, 12).copy(), cam_pair=out["cam_pair"].view(np.int32).copy(),
                max_records=0, record_obs=None)


def window(npts=120, ncams=8, nq=1, seed=21, noise=0.3, wrong=12):
    """A planted window: ncams cameras see npts points; the tracks hold the observations of every image but the last nq,
    whose records are the query frames (`wrong` of each moved anywhere in the frame).  Every point has a random unit
    descriptor, every view of it its own small noise, quantised as misift_quantize_batch does.  Record r of frame f is
    point perm[f][r].  dict(describe: the describe case, K, true (ncams, 12), query, query_q: per query frame its
    records and their int8 rows, perm, moved, cam, cam_pair: the cameras of the window with the new images unset)."""
    import batch_util as BU
    key = ("window", npts, ncams, nq, seed, noise, wrong)
    if key in _MEMO:
        return _MEMO[key]
    rng = np.random.default_rng(seed)
    cams = TC.cameras(ncams, 0.4, rng)
    K = np.array([TC.INTRINSICS[i % 2] for i in range(ncams)], f32)
    R3, t3 = cams[ncams // 2]
    z = rng.uniform(4, 12, npts)
    Xc = np.stack([rng.uniform(-0.2, 0.2, npts) * z, rng.uniform(-0.15, 0.15, npts) * z, z], 1)
    X = ((Xc - t3) @ R3).astype(f32).astype(np.float64)          # R3^T (Xc - t3)
    d = np.abs(rng.normal(0, 1, (npts, 128)))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    perm = [rng.permutation(npts) for _ in range(ncams)]
    inv = [np.argsort(p) for p in perm]
    q = np.zeros((ncams * npts, 128), np.int8)
    px = np.zeros((ncams, npts, 2))
    for f in range(ncams):
        v = d + rng.normal(0, 0.004, d.shape)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        q[f * npts:(f + 1) * npts] = BU.quantize_np(v.astype(f32))[perm[f]]
        for j in range(npts):
            px[f, j] = TC.project(cams, K, [f], X[j])[0][0] + rng.normal(0, noise, 2)
    nb = ncams - nq                                              # the images of the window
    tracks = [(list(range(nb)), px[:nb, j]) for j in range(npts)]
    pair = [C.ROOT] + list(range(nb - 1)) + [C.UNSET] * nq
    tri = TC.pack(cams, K, tracks, cam_pair=pair, slack_tracks=3, slack_obs=4, seed=seed)
    obs = tri["obs"]
    for j in range(npts):
        obs["record"][j * nb:(j + 1) * nb] = [inv[f][j] for f in range(nb)]
    rc = RC.refine_case(tri, X)
    cam = rc["cam"].copy()
    cam[nb:] = 0
    describe = dict(max_tracks=rc["max_tracks"], max_obs=rc["max_obs"], track_offsets=rc["track_offsets"], obs=obs,
                    export_summary=rc["export_summary"], points=rc["points"], point_status=rc["point_status"], q=q,
                    nframes=ncams, counts=np.full(ncams, npts, np.int32), offsets=None, stride=npts,
                    max_records=ncams * npts)
    query, query_q, moved = [], [], []
    for f in range(nb, ncams):
        rows = np.zeros(npts, point_dtype())
        rows["xpos"], rows["ypos"] = px[f][perm[f]].T.astype(f32)
        mv = rng.choice(npts, wrong, replace=False)
        rows["xpos"][mv], rows["ypos"][mv] = rng.uniform(0, 1920, wrong), rng.uniform(0, 1080, wrong)
        query.append(rows)
        query_q.append(q[f * npts:(f + 1) * npts])
        moved.append(set(mv.tolist()))
    out = dict(describe=describe, K=K, true=np.array([np.concatenate([R.reshape(9), t]) for R, t in cams]), query=query,
               query_q=query_q, perm=perm, moved=moved, cam=cam, cam_pair=np.asarray(pair, np.int32), nimages=ncams,
               npts=npts, nq=nq, nb=nb)
    _MEMO[key] = out
    return out


def scene_records(case, out):
    """describe's outputs (uint32) as what the matcher takes for set 2: (records of T points, their int8 rows)."""
    T = int(out["scene_count"].view(np.int32)[0])
    recs = out["scene_recs"].view(point_dtype())[:T]
    return recs, out["scene_q"].view(np.int8).reshape(-1, 128)[:T]


def window_localize_case(w, rows, num_loops=256, **kw):
    """The localise case of the window's query frames from their match rows against the scene (frame i: query i)."""
    d = w["describe"]
    n, nq = w["npts"], w["nq"]
    assert len(rows) == n * nq
    case = dict(rows=rows, nframes_rows=nq, counts=np.full(nq, n, np.int32), offsets=None, stride=n,
                max_tracks=d["max_tracks"], export_summary=d["export_summary"], points=d["points"],
                point_status=d["point_status"], nimages=w["nimages"], intrinsics=w["K"],
                frames=np.arange(nq, dtype=np.int32), images=np.arange(w["nb"], w["nimages"], dtype=np.int32),
                seeds=np.arange(nq, dtype=np.uint32) + 77, max_pts=n, min_score=0.5, max_ambiguity=0.95,
                num_loops=num_loops, thresh=4.0, min_inliers=12, only_unset=1, install=1, cam=w["cam"],
                cam_pair=w["cam_pair"], max_found=n * nq)
    case.update(kw)
    return case


def window_merge_case(w, loc_case, loc_out, describe_views=None):
    """merge(A = the finds, B = the window's scene) as merge_cases takes it: no shifts, the same cameras on both sides."""
    import merge_cases as MC
    d = w["describe"]
    a = found_scene(loc_case, loc_out)
    b = dict(max_tracks=d["max_tracks"], max_obs=d["max_obs"], track_offsets=d["track_offsets"], obs=d["obs"],
             export_summary=d["export_summary"], points=d["points"],
             point_views=np.full(d["max_tracks"], w["nb"], np.int32), point_status=d["point_status"],
             nimages=w["nimages"], cam=a["cam"], cam_pair=a["cam_pair"], max_records=0, record_obs=None)
    Tp = int(a["export_summary"][2])
    return MC.merge_case(a, b, loc_out["found_map"].view(np.int32)[:Tp], slack_images=0, want=(True, True, False))

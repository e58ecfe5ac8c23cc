"""misift_triangulate_tracks_batch: expected_triangulate, the numpy restatement of the definition in include/misift.h, the
wrapper of the library's host hook, and the cases of its tests (test_triangulate_cpu.py pins the restatement to the hook
and to float64, test_gpu_triangulate.py holds the device to it byte for byte).  A case is a dict of the call's arguments,
CASE_KEYS.  The restatement takes its number format as an argument: with float32 every operation is rounded as the
library rounds it, with float64 the same algorithm is the yardstick.  No GPU in here, and cudasift_amd.capi is imported
inside functions only."""
import numpy as np

import pose_cases as PC
import posegraph_cases as G
from test_fundamental_cpu import f32

OK, FEW_VIEWS, SINGULAR, BEHIND, BAD_RANGE = 0, 1, 2, 3, 4
UNSET = G.UNSET
POISON_WORD = 0x5A5A5A5A                                         # batch_util.POISON_WORD, asserted in the GPU file
OBS_DTYPE = np.dtype([("frame", "<i4"), ("record", "<i4"), ("xpos", "<f4"), ("ypos", "<f4")])
CASE_KEYS = ("max_tracks", "max_obs", "track_offsets", "obs", "export_summary", "nimages", "cam", "cam_pair",
             "intrinsics", "min_views", "num_loops")


# ---- the definition restated: arrays over the usable views of one track, every operation rounded to dt

def _sum(terms, dt):
    """0 + t0 + t1 + ... one term at a time, every sum rounded to dt."""
    return np.add.accumulate(np.concatenate([np.zeros(1, dt), terms.astype(dt)]), dtype=dt)[-1]


def _normal(a, rhs, dt):
    """M (six entries) and g of the rows a (m, 2, 3) with right-hand sides rhs (m, 2): the u row before the v row."""
    a, r = a.reshape(-1, 3), rhs.reshape(-1)
    a0, a1, a2 = a[:, 0], a[:, 1], a[:, 2]
    return [_sum(t, dt) for t in (a0 * a0, a0 * a1, a0 * a2, a1 * a1, a1 * a2, a2 * a2, a0 * r, a1 * r, a2 * r)]


def _pivot(d):
    return bool(d > 0) and bool(np.isfinite(d))


def solve(N):
    """LDL^T without pivoting as the header writes it out: the solution, or None where the solve fails."""
    m00, m01, m02, m11, m12, m22, g0, g1, g2 = N
    d0 = m00
    if not _pivot(d0):
        return None
    l10, l20 = m01 / d0, m02 / d0
    d1 = m11 - l10 * m01
    if not _pivot(d1):
        return None
    e = m12 - l20 * m01
    l21 = e / d1
    d2 = (m22 - l20 * m02) - l21 * e
    if not _pivot(d2):
        return None
    y0 = g0
    y1 = g1 - l10 * y0
    y2 = (g2 - l20 * y0) - l21 * y1
    x2 = y2 / d2
    x1 = y1 / d1 - l21 * x2
    x0 = (y0 / d0 - l10 * x1) - l20 * x2
    if not (np.isfinite(x0) and np.isfinite(x1) and np.isfinite(x2)):
        return None
    return [x0, x1, x2]


def usable_views(cam, cam_pair, nimages, obs):
    """Step 1: a flag per observation."""
    f = obs["frame"].astype(np.int64)
    ok = (f >= 0) & (f < nimages)
    fc = np.where(ok, f, 0)
    ok &= (np.asarray(cam_pair)[fc] != UNSET) & np.isfinite(np.asarray(cam, f32).reshape(-1, 12)[fc]).all(1)
    return ok & np.isfinite(obs["xpos"]) & np.isfinite(obs["ypos"])


def _residuals(c, k, x, y, X, dt):
    """Step 3 under X over the views (c: their cameras (m, 12), k: their intrinsics (m, 4)): None when a view is not in
    front, otherwise (cost, N, ru, rv)."""
    xc = ((c[:, 0] * X[0] + c[:, 1] * X[1]) + c[:, 2] * X[2]) + c[:, 9]
    yc = ((c[:, 3] * X[0] + c[:, 4] * X[1]) + c[:, 5] * X[2]) + c[:, 10]
    zc = ((c[:, 6] * X[0] + c[:, 7] * X[1]) + c[:, 8] * X[2]) + c[:, 11]
    if not (zc > 0).all():
        return None
    iz = dt(1) / zc
    a, b = xc * iz, yc * iz
    ru, rv = x - (k[:, 0] * a + k[:, 2]), y - (k[:, 1] * b + k[:, 3])
    cost = _sum(ru * ru + rv * rv, dt)
    su, sv = (k[:, 0] * iz)[:, None], (k[:, 1] * iz)[:, None]
    ju = su * (c[:, 0:3] - a[:, None] * c[:, 6:9])
    jv = sv * (c[:, 3:6] - b[:, None] * c[:, 6:9])
    return cost, _normal(np.stack([ju, jv], 1), np.stack([ru, rv], 1), dt), ru, rv


def expected_track(cam, cam_pair, intrinsics, nimages, obs, min_views, num_loops, dt=f32):
    """Steps 1-5 for one track: dict(point4, views, status, obs_error (one per observation), accepted)."""
    nan = PC.ONE_NAN if dt is f32 else dt(np.nan)
    use = usable_views(cam, cam_pair, nimages, obs)
    m = int(use.sum())
    out = dict(point4=np.full(4, nan, dt), views=m, status=OK, obs_error=np.full(len(obs), nan, dt), accepted=0)
    if m < min_views:
        out["status"] = FEW_VIEWS
        return out
    o = obs[use]
    c = np.asarray(cam, f32).reshape(-1, 12)[o["frame"]].astype(dt)
    k = np.asarray(intrinsics, f32).reshape(-1, 4)[o["frame"]].astype(dt)
    x, y = o["xpos"].astype(dt), o["ypos"].astype(dt)
    with np.errstate(all="ignore"):
        u, v = (x - k[:, 2]) / k[:, 0], (y - k[:, 3]) / k[:, 1]
        au = c[:, 0:3] - u[:, None] * c[:, 6:9]
        av = c[:, 3:6] - v[:, None] * c[:, 6:9]
        rhs = np.stack([u * c[:, 11] - c[:, 9], v * c[:, 11] - c[:, 10]], 1)
        X = solve(_normal(np.stack([au, av], 1), rhs, dt))
        if X is None:
            out["status"] = SINGULAR
            return out
        res = _residuals(c, k, x, y, X, dt)
        if res is None:
            out["status"] = BEHIND
            return out
        for _ in range(num_loops):
            d = solve(res[1])
            if d is None:
                break
            X2 = [X[0] + d[0], X[1] + d[1], X[2] + d[2]]
            res2 = _residuals(c, k, x, y, X2, dt)
            if res2 is None or not res2[0] < res[0]:
                break
            X, res = X2, res2
            out["accepted"] += 1
        cost, _, ru, rv = res
        rms = np.sqrt(cost / dt(m))
        out["point4"][:] = [X[0], X[1], X[2], nan if np.isnan(rms) else rms]
        err = np.sqrt(ru * ru + rv * rv)
        out["obs_error"][use] = np.where(np.isnan(err), nan, err)
    return out


def range_ok(off, end, max_obs):
    return 0 <= off <= end <= max_obs


def expected_triangulate(case, obs_error=True):
    """The five outputs of the call on poisoned buffers of exactly the stated sizes, as uint32 arrays: points (4 per
    track), point_views, point_status, obs_error (None when left out), summary.  Tracks of equal range, min_views and
    num_loops are computed once per case family (case["memo"], shared by the variants of one pool)."""
    mt, mo = case["max_tracks"], case["max_obs"]
    T = min(max(int(case["export_summary"][2]), 0), mt)
    points, views = np.full(4 * mt, POISON_WORD, np.uint32), np.full(mt, POISON_WORD, np.uint32)
    status, err = np.full(mt, POISON_WORD, np.uint32), np.full(mo, POISON_WORD, np.uint32)
    summary = np.zeros(8, np.int32)
    summary[0] = T
    memo = case.setdefault("memo", {})
    for t in range(T):
        off, end = int(case["track_offsets"][t]), int(case["track_offsets"][t + 1])
        if not range_ok(off, end, mo):
            points[4 * t:4 * t + 4], views[t], status[t] = PC.NAN_BITS, 0, BAD_RANGE
            summary[7] += 1
            continue
        key = (off, end, case["min_views"], case["num_loops"])
        if key not in memo:
            memo[key] = expected_track(case["cam"], case["cam_pair"], case["intrinsics"], case["nimages"],
                                       case["obs"][off:end], case["min_views"], case["num_loops"])
        e = memo[key]
        points[4 * t:4 * t + 4], views[t], status[t] = e["point4"].view(np.uint32), e["views"], e["status"]
        err[off:end] = e["obs_error"].view(np.uint32)
        summary[(1, 3, 4, 5)[e["status"]]] += 1
        summary[2] += e["views"] if e["status"] == OK else 0
        summary[6] += e["accepted"]
    return dict(points=points, point_views=views, point_status=status, obs_error=err if obs_error else None,
                summary=summary.view(np.uint32))


# ---- the hook

def hook_track(cam, cam_pair, intrinsics, nimages, obs, min_views, num_loops, obs_error=True):
    from cudasift_amd import capi
    cam, cam_pair = np.ascontiguousarray(cam, f32), np.ascontiguousarray(cam_pair, np.int32)
    intrinsics, obs = np.ascontiguousarray(intrinsics, f32), np.ascontiguousarray(obs, OBS_DTYPE)
    point, err = np.full(4, 3.5, f32), np.full(max(len(obs), 1), 3.5, f32)
    ints = np.full(3, -77, np.int32)
    assert capi.lib().misift_test_triangulate_track(
        cam.ctypes.data, cam_pair.ctypes.data, intrinsics.ctypes.data, nimages, obs.ctypes.data if len(obs) else None,
        len(obs), min_views, num_loops, point.ctypes.data, ints.ctypes.data, ints.ctypes.data + 4,
        err.ctypes.data if obs_error else None, ints.ctypes.data + 8) == 0
    return dict(point4=point, views=int(ints[0]), status=int(ints[1]), obs_error=err[:len(obs)], accepted=int(ints[2]))


def capacity():
    from cudasift_amd import capi
    return int(capi.lib().misift_test_triangulate_capacity())


# ---- planted scenes

INTRINSICS = (PC.K_A, PC.K_B)


def cameras(ncams, step, rng, angle=0.05):
    """World-to-camera (R, t) float64: centres `step` apart along x with a jitter of a fifth of it, small rotations."""
    out = []
    for i in range(ncams):
        C = np.array([i * step, 0.0, 0.0]) + rng.normal(0, 0.2 * step, 3)
        R = PC.rodrigues(rng.normal(0, 1, 3), angle * rng.uniform(0.2, 1))
        out.append((R, -R @ C))
    return out


def project(cams, K, frames, X):
    """The pixel positions of the world point X in the cameras `frames` (float64), and its depths there."""
    px, z = [], []
    for f in frames:
        R, t = cams[f]
        Xc = R @ X + t
        fx, fy, cx, cy = K[f]
        px.append((fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy))
        z.append(Xc[2])
    return np.array(px), np.array(z)


def pack(cams, K, tracks, min_views=2, num_loops=5, cam_pair=None, slack_tracks=0, slack_obs=0, seed=0):
    """A case from cameras [(R, t)] or an (n, 12) array, intrinsics (n, 4) and tracks [(frames, xy (m, 2))]: the
    observation lists as misift_export_tracks_batch lays them out, the record field random."""
    rng = np.random.default_rng(900 + seed)
    cam = np.array([np.concatenate([R.reshape(9), t]) for R, t in cams]) if isinstance(cams, list) else cams
    cam = np.ascontiguousarray(cam, f32).reshape(-1, 12)
    n = sum(len(f) for f, _ in tracks)
    obs = np.zeros(n + slack_obs, OBS_DTYPE)
    obs["frame"][n:], obs["xpos"][n:], obs["ypos"][n:] = 0, 100, 100         # beyond the tracks: must not be read
    offs = np.full(len(tracks) + slack_tracks + 1, POISON_WORD, np.uint32).view(np.int32)
    offs[0] = at = 0
    for t, (frames, xy) in enumerate(tracks):
        m = len(frames)
        obs["frame"][at:at + m] = frames
        obs["xpos"][at:at + m], obs["ypos"][at:at + m] = np.asarray(xy, f32).reshape(-1, 2).T
        at += m
        offs[t + 1] = at
    obs["record"] = rng.integers(-2 ** 31, 2 ** 31 - 1, len(obs))
    T = len(tracks)
    longest = max([len(f) for f, _ in tracks] + [0])
    return dict(max_tracks=max(T + slack_tracks, 1), max_obs=max(n + slack_obs, 1), track_offsets=offs,
                obs=obs if len(obs) else np.zeros(1, OBS_DTYPE), export_summary=np.array([T, n, T, n, longest, 0, 0, 0],
                                                                                         np.int32),
                nimages=len(cam), cam=cam, cam_pair=np.zeros(len(cam), np.int32) if cam_pair is None else
                np.asarray(cam_pair, np.int32), intrinsics=np.ascontiguousarray(K, f32).reshape(-1, 4),
                min_views=min_views, num_loops=num_loops, memo={})


def variant(case, **kw):
    """The same pool under other arguments; the memo of per-track answers is shared (its key holds min_views, num_loops
    and the range), so cam, obs and intrinsics must stay as they are."""
    assert not {"cam", "cam_pair", "obs", "intrinsics", "nimages"} & set(kw)
    return dict(case, **kw)


def with_T(case, T, max_tracks=None):
    """T as the device would report it; max_tracks cuts the outputs and the offsets to exactly that many."""
    s = case["export_summary"].copy()
    s[2] = T
    kw = dict(export_summary=s)
    if max_tracks is not None:
        kw.update(max_tracks=max_tracks, track_offsets=case["track_offsets"][:max_tracks + 1].copy())
    return variant(case, **kw)


_SCENES = {}


def planted(ratio, noise, ntracks=300, ncams=6, seed=51, num_loops=5, lengths=(2, 3, 4, 5, 6), nimages=None, long=None):
    """ntracks points 4 to 12 deep seen by runs of cameras whose neighbouring centres are ratio * 8 apart, `noise` px of
    Gaussian noise on every position: dict(case, X (ntracks, 3) float64, cams, K).  With nimages > ncams the cameras
    repeat with period ncams and every observation picks one of its camera's copies.  long = (t, m): track t has m observations instead."""
    key = (ratio, noise, ntracks, ncams, seed, num_loops, lengths, nimages, long)
    if key not in _SCENES:
        rng = np.random.default_rng(seed)
        cams = cameras(ncams, ratio * 8.0, rng)
        K = [INTRINSICS[i % 2] for i in range(ncams)]
        tracks, Xs = [], []
        for t in range(ntracks):
            m = long[1] if long and t == long[0] else lengths[t % len(lengths)]
            first = int(rng.integers(0, ncams - min(m, ncams) + 1))
            frames = [first + j % ncams for j in range(m)] if m <= ncams else list(rng.integers(0, ncams, m))
            mid = -cams[frames[len(frames) // 2]][0].T @ cams[frames[len(frames) // 2]][1]
            z = rng.uniform(4, 12)
            X = mid + np.array([rng.uniform(-0.3, 0.3) * z, rng.uniform(-0.2, 0.2) * z, z])
            px, depth = project(cams, K, frames, X)
            assert (depth > 1).all()
            tracks.append((frames, px + rng.normal(0, noise, px.shape) if noise else px))
            Xs.append(X)
        if nimages:
            reps = -(-nimages // ncams)
            cams, K = (cams * reps)[:nimages], (K * reps)[:nimages]
            for frames, _ in tracks:
                for j, f in enumerate(frames):
                    frames[j] = f + ncams * int(rng.integers(0, (nimages - 1 - f) // ncams + 1))
        _SCENES[key] = dict(case=pack(cams, K, tracks, num_loops=num_loops, seed=seed), X=np.array(Xs), cams=cams, K=K)
    return _SCENES[key]


def triangulate64(case):
    """The same algorithm in float64 on the same inputs: (points (T, 4), status (T,), accepted (T,))."""
    T = int(case["export_summary"][2])
    out = [expected_track(case["cam"], case["cam_pair"], case["intrinsics"], case["nimages"],
                          case["obs"][case["track_offsets"][t]:case["track_offsets"][t + 1]], case["min_views"],
                          case["num_loops"], np.float64) for t in range(T)]
    return (np.array([e["point4"] for e in out]), np.array([e["status"] for e in out]),
            np.array([e["accepted"] for e in out]))


def pool_case(num_loops=5, min_views=2):
    """258 tracks of lengths 1, 2, 3, 7 in rotation, 0.5 px noise, with one track of 301 observations among them (its
    cameras repeat): the pool the GPU file cuts its T from."""
    sc = planted(0.05, 0.5, ntracks=258, ncams=8, seed=52, lengths=(1, 2, 3, 7), long=(5, 301))
    return variant(sc["case"], num_loops=num_loops, min_views=min_views)


def capacity_case(nimages):
    """70 tracks whose observations reach the last of nimages images."""
    sc = planted(0.05, 0.5, ntracks=70, ncams=8, seed=53, nimages=nimages, lengths=(2, 3, 4, 5))
    case = sc["case"]
    f = case["obs"]["frame"]
    f[np.nonzero(f % 8 == (nimages - 1) % 8)[0][:3]] = nimages - 1       # the last image is a copy of their camera
    assert f.max() == nimages - 1 and case["nimages"] == nimages
    return case


def chain_case(num_loops=5):
    """The 64-image chain of posegraph_cases under the cameras misift_link_poses_batch links (fp32, with their drift), far
    from the origin at the end: 4 points per window of 4 images, observed exactly under the planted cameras."""
    key = ("chain", num_loops)
    if key not in _SCENES:
        x = G.exact_chain()
        with np.errstate(all="ignore"):
            linked = G.expected_link_poses(x["case"])
        gt = G.planted_cameras(x["cams"], 0, x["pairs"][0])
        cams = [(c[:9].reshape(3, 3), c[9:]) for c in gt]
        K = [INTRINSICS[i % 2] for i in range(64)]
        rng = np.random.default_rng(54)
        tracks, Xs = [], []
        for i in range(61):
            for _ in range(4):
                R, t = cams[i + 1]
                z = rng.uniform(30, 60)
                X = R.T @ (np.array([rng.uniform(-0.25, 0.25) * z, rng.uniform(-0.15, 0.15) * z, z]) - t)
                frames = [i, i + 1, i + 2, i + 3]
                px, depth = project(cams, K, frames, X)
                assert (depth > 1).all()
                tracks.append((frames, px))
                Xs.append(X)
        case = pack(linked["cam"], K, tracks, num_loops=num_loops, cam_pair=linked["cam_pair"], seed=54)
        _SCENES[key] = dict(case=case, X=np.array(Xs), gt=gt)
    return _SCENES[key]


# ---- hostile inputs

def hostile_case(num_loops=5, min_views=2):
    """Every hostile input of the issue, one or two tracks each, among good tracks; names[t] says what track t holds."""
    rng = np.random.default_rng(55)
    cams = cameras(8, 0.4, rng)
    K = [INTRINSICS[i % 2] for i in range(8)]
    C0 = -cams[0][0].T @ cams[0][1]
    back = PC.rodrigues([0, 1, 0], np.pi) @ cams[2][0]           # image 8: at image 2's centre, looking the other way
    C2 = -cams[2][0].T @ cams[2][1]
    cams += [(back, -back @ C2), (np.zeros((3, 3)), np.zeros(3)),            # 9: no camera (d_cam_pair -2)
             (cams[1][0].copy(), cams[1][1].copy()), (cams[1][0].copy(), cams[1][1].copy()),     # 10, 11: NaN, inf
             (cams[3][0].copy(), cams[3][1].copy()), (cams[3][0].copy(), cams[3][1].copy())]     # 12, 13: identical
    for back_off in ([0.3, 0.0, 5.0], [-0.4, 0.1, 6.0]):         # 14, 15: behind image 0, they see its centre
        R = PC.rodrigues(rng.normal(0, 1, 3), 0.02)
        cams.append((R, -R @ (C0 - np.array(back_off))))
    K += [K[2], K[0], K[1], K[1], K[1], K[1], K[0], K[1]]
    cam_pair = [-1, 0, 1, 2, 3, 4, 5, 6, 7, UNSET, 8, 9, 10, 11, 12, 13]
    n = len(cams)
    X = C0 + np.array([0.8, -0.5, 7.0])
    tracks, names = [], []

    def add(name, frames, xy=None, at=X, edit=None):
        if xy is None:
            px, _ = project(cams, K, [f if 0 <= f < n and f != 9 else 0 for f in frames], at)
            px = px + rng.normal(0, 0.3, px.shape)
        else:
            px = np.asarray(xy, np.float64)
        if edit:
            edit(px)
        tracks.append((list(frames), px))
        names.append(name)

    def put(i, j, v):
        def edit(px):
            px[i, j] = v
        return edit

    add("good", [0, 1, 2, 3])
    add("frame -1", [0, -1, 2])
    add("frame nimages", [1, n, 3])
    add("frame far out of range", [2 ** 31 - 1, 1, -2 ** 31, 3])
    add("only out-of-range frames", [-1, n, n + 5])
    add("an unset camera", [0, 9, 2])
    add("an unset camera leaves one view", [0, 9])
    add("a NaN in a camera", [0, 10, 2])
    add("an inf in a camera", [3, 11, 4])
    add("a NaN x", [0, 1, 2, 3], edit=put(1, 0, np.nan))
    add("an inf y", [0, 1, 2, 3], edit=put(2, 1, np.inf))
    add("a -inf x leaves one view", [0, 1], edit=put(0, 0, -np.inf))
    add("behind one camera", [0, 1, 8, 3])
    add("behind one of two", [1, 8])
    add("identical cameras, identical positions", [12, 13], xy=np.tile(project(cams, K, [12], X)[0], (2, 1)))
    add("identical cameras, noise", [12, 13])
    add("identical cameras, three times", [12, 13, 3], xy=np.tile(project(cams, K, [12], X)[0], (3, 1)))
    centre = [[K[0][2], K[0][3]]]
    add("on a camera centre", [0, 14, 15], at=C0, xy=np.concatenate([centre, project(cams, K, [14, 15], C0)[0]]))
    add("near a camera centre", [0, 14, 15], at=C0 + [0, 0, 1e-3])
    add("two observations from one frame", [0, 1, 1, 2])
    add("one frame only, twice", [4, 4])
    add("one observation", [5])
    add("no observation", [])
    add("all positions equal", [0, 1, 2], xy=[[900, 500]] * 3)
    add("huge positions", [0, 1, 2], xy=[[3e38, 1e30], [-3e38, 2.0], [1e20, -3e38]])
    add("good again", [4, 5, 6, 7])
    cam = np.array([np.concatenate([R.reshape(9), t]) for R, t in cams], f32)
    cam[10, 4], cam[11, 10] = np.nan, np.inf
    case = pack(cam, K, tracks, min_views=min_views, num_loops=num_loops, cam_pair=cam_pair, slack_obs=3, seed=55)
    case["names"] = names
    return case


def bad_offsets_case():
    """Offsets that decrease, pass max_obs, are negative, or skip: the tracks around them are good."""
    sc = planted(0.05, 0.5, ntracks=12, ncams=6, seed=56)
    case = dict(sc["case"], memo={})
    offs = case["track_offsets"].copy()
    mo = case["max_obs"]
    offs[3] = 2 ** 31 - 1                                        # track 2 ends far past max_obs, track 3 decreases
    offs[6] = mo + 1                                             # track 5 ends one past max_obs, track 6 starts there
    offs[9] = -4                                                 # track 8 ends below 0, track 9 starts there
    offs[12] = offs[11] - 2                                      # the last track decreases
    case["track_offsets"] = offs
    case["bad"] = [2, 3, 5, 6, 8, 9, 11]                         # no two valid ranges overlap: every output has one writer
    return case

"""misift_refine_cameras_batch: expected_refine, the numpy restatement of the definition in include/misift.h, the wrapper
of the library's host hook, and the cases of its tests (test_refine_cpu.py pins the restatement to the hook and to
float64, test_gpu_refine.py holds the device to it byte for byte).  A case is a triangulate case (triangulate_cases.pack)
with the call's further arguments: points, point_status, hold, min_obs, num_loops, max_error, orthonormalise.  The
restatement takes its number format as an argument: with float32 every operation is rounded as the library rounds it,
with float64 the same algorithm is the yardstick.  No GPU in here, and cudasift_amd.capi is imported inside functions
only."""
import numpy as np

import pose_cases as PC
import posegraph_cases as G
import triangulate_cases as TC
from test_fundamental_cpu import f32

OK, FEW_OBS, SINGULAR, HELD, NO_CAMERA = 0, 1, 2, 3, 4
UNSET, ROOT = G.UNSET, G.ROOT
SLOTS = 256
INF = float("inf")
OUTPUTS = ("cam_out", "cam_obs", "cam_rms", "cam_steps", "cam_status", "summary")


# ---- the definition restated

def slot_sum(terms, slots, dt):
    """The sum of the call for every column of terms (n, K): 256 partial sums, slot o mod 256 in ascending o, the tree."""
    terms = np.asarray(terms, dt)
    p = np.zeros((SLOTS, terms.shape[1]), dt)
    s = np.asarray(slots, np.int64) % SLOTS
    order = np.argsort(s, kind="stable")                         # the slots are ascending, so each group is too
    first = np.concatenate([[0], np.nonzero(np.diff(s[order]))[0] + 1]) if len(s) else np.zeros(0, np.int64)
    rank = np.zeros(len(s), np.int64)
    rank[order] = np.arange(len(s)) - np.repeat(first, np.diff(np.concatenate([first, [len(s)]])))
    for r in range(int(rank.max()) + 1 if len(s) else 0):
        sel = rank == r
        p[s[sel]] = p[s[sel]] + terms[sel]
    off = SLOTS // 2
    while off:
        p[:off] = p[:off] + p[off:2 * off]
        off //= 2
    return p[0]


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def orthonormalise(c, dt):
    r0, r1 = c[0:3], c[3:6]
    r0 = r0 / np.sqrt(dot3(r0, r0))
    w = r1 - dot3(r1, r0) * r0
    r1 = w / np.sqrt(dot3(w, w))
    r2 = np.array([r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]], dt)
    return np.concatenate([r0, r1, r2, c[9:12]]).astype(dt)


def view(c, k, X, x, y, dt):
    """Step 3 of triangulate for every candidate under one camera."""
    xc = ((c[0] * X[:, 0] + c[1] * X[:, 1]) + c[2] * X[:, 2]) + c[9]
    yc = ((c[3] * X[:, 0] + c[4] * X[:, 1]) + c[5] * X[:, 2]) + c[10]
    zc = ((c[6] * X[:, 0] + c[7] * X[:, 1]) + c[8] * X[:, 2]) + c[11]
    iz = dt(1) / zc
    a, b = xc * iz, yc * iz
    return xc, yc, zc, iz, a, b, x - (k[0] * a + k[2]), y - (k[1] * b + k[3])


def sums(c, k, X, x, y, slots, dt):
    """Step 3: None when the camera is not in front of every member, otherwise the 28 sums."""
    xc, yc, zc, iz, a, b, ru, rv = view(c, k, X, x, y, dt)
    if not (zc > 0).all():
        return None
    gx, gy = k[0] * iz, k[1] * iz
    ju = [gx * -(a * yc), gx * (zc + a * xc), gx * -yc, gx * dt(1), gx * dt(0), gx * -a]
    jv = [gy * -(zc + b * yc), gy * (b * xc), gy * xc, gy * dt(0), gy * dt(1), gy * -b]
    cols = [ru * ru + rv * rv]
    cols += [ju[r] * ju[q] + jv[r] * jv[q] for r in range(6) for q in range(r, 6)]
    cols += [ju[r] * ru + jv[r] * rv for r in range(6)]
    return slot_sum(np.stack(cols, 1), slots, dt)


def solve6(S):
    """LDL^T without pivoting as the header writes it out: delta, or None where the solve fails."""
    M = np.zeros((6, 6), S.dtype)
    i = 1
    for r in range(6):
        for q in range(r, 6):
            M[r, q] = M[q, r] = S[i]
            i += 1
    g = S[22:28]
    L = np.zeros((6, 6), S.dtype)
    d, v, y, x = [None] * 6, [None] * 6, [None] * 6, [None] * 6
    for j in range(6):
        dj = M[j, j]
        for k in range(j):
            v[k] = L[j, k] * d[k]
            dj = dj - L[j, k] * v[k]
        d[j] = dj
        if not (dj > 0 and np.isfinite(dj)):
            return None
        for i in range(j + 1, 6):
            e = M[i, j]
            for k in range(j):
                e = e - L[i, k] * v[k]
            L[i, j] = e / dj
    for i in range(6):
        e = g[i]
        for k in range(i):
            e = e - L[i, k] * y[k]
        y[i] = e
    for i in range(5, -1, -1):
        e = y[i] / d[i]
        for k in range(i + 1, 6):
            e = e - L[k, i] * x[k]
        x[i] = e
    return x if all(np.isfinite(e) for e in x) else None


def update(c, delta, dt):
    """Step 5: the Cayley map of omega / 2 applied to (R, t), then + upsilon."""
    h = [dt(0.5) * delta[0], dt(0.5) * delta[1], dt(0.5) * delta[2]]
    s = dot3(h, h)
    den, e, two = dt(1) + s, dt(1) - s, dt(2)
    xy, xz, yz = two * (h[0] * h[1]), two * (h[0] * h[2]), two * (h[1] * h[2])
    x2, y2, z2 = two * h[0], two * h[1], two * h[2]
    C = [[(e + two * (h[0] * h[0])) / den, (xy - z2) / den, (xz + y2) / den],
         [(xy + z2) / den, (e + two * (h[1] * h[1])) / den, (yz - x2) / den],
         [(xz - y2) / den, (yz + x2) / den, (e + two * (h[2] * h[2])) / den]]
    out = np.zeros(12, dt)
    for i in range(3):
        for j in range(3):
            out[3 * i + j] = (C[i][0] * c[j] + C[i][1] * c[3 + j]) + C[i][2] * c[6 + j]
        out[9 + i] = ((C[i][0] * c[9] + C[i][1] * c[10]) + C[i][2] * c[11]) + delta[3 + i]
    return out


def expected_camera(cam12, cam_pair, held, k4, slots, X, xy, min_obs, num_loops, max_error, orth, dt=f32):
    """Steps 0-7 for one image from its candidates (slots ascending, X (n, 3), xy (n, 2)): dict(cam (12 values of dt; the
    input's bits when as_given), as_given, nobs, rms (2), steps, status, trace).  trace lists what ended or continued each
    loop: 'kept', 'worse', 'behind', 'singular'; gated = the candidates in front that max_error turned away."""
    nan = PC.ONE_NAN if dt is f32 else dt(np.nan)
    cam_in = np.asarray(cam12, f32)
    out = dict(cam=cam_in.astype(dt), as_given=True, nobs=0, rms=np.array([nan, nan], dt), steps=0, status=OK, trace=[],
               gated=0)
    if cam_pair == UNSET or not np.isfinite(cam_in).all():
        out["status"] = NO_CAMERA
        return out
    if cam_pair == ROOT or held:
        out["status"] = HELD
        return out
    with np.errstate(all="ignore"):
        c = cam_in.astype(dt)
        if orth:
            c = orthonormalise(c, dt)
            if not np.isfinite(c).all():
                out["status"] = NO_CAMERA
                return out
            out["cam"], out["as_given"] = c, False
        k = np.asarray(k4, f32).astype(dt)
        X, xy = np.asarray(X, f32).reshape(-1, 3).astype(dt), np.asarray(xy, f32).reshape(-1, 2).astype(dt)
        slots = np.asarray(slots, np.int64)
        thresh2 = dt(f32(max_error)) * dt(f32(max_error)) if dt is not f32 else f32(max_error) * f32(max_error)
        _, _, zc, _, _, _, ru, rv = view(c, k, X, xy[:, 0], xy[:, 1], dt)
        front = zc > 0
        member = front if np.isinf(thresh2) else front & (ru * ru + rv * rv < thresh2)
        out["gated"] = int(front.sum() - member.sum())
        n = out["nobs"] = int(member.sum())
        if n < min_obs:
            out["status"] = FEW_OBS
            return out
        X, x, y, slots = X[member], xy[member, 0], xy[member, 1], slots[member]
        S = sums(c, k, X, x, y, slots, dt)
        c0 = S[0]
        for loop in range(num_loops):
            delta = solve6(S)
            if delta is None:
                out["trace"].append("singular")
                if loop == 0:
                    out["status"] = SINGULAR
                break
            c2 = update(c, delta, dt)
            S2 = sums(c2, k, X, x, y, slots, dt)
            if S2 is None or not S2[0] < S[0]:
                out["trace"].append("behind" if S2 is None else "worse")
                break
            c, S = c2, S2
            out["steps"] += 1
            out["trace"].append("kept")
        if out["steps"]:
            out["cam"], out["as_given"] = c, False
        rms = np.array([np.sqrt(c0 / dt(n)), np.sqrt(S[0] / dt(n))], dt)
        out["rms"] = np.where(np.isnan(rms), nan, rms).astype(dt)
    return out


def counts(case):
    T = min(max(int(case["export_summary"][2]), 0), case["max_tracks"])
    O = min(max(int(case["export_summary"][3]), 0), case["max_obs"])
    return T, O


def candidate_keys(case):
    """key[o] for o < O: the image slot o is a candidate of, or -1."""
    T, O = counts(case)
    owner = np.full(O, -1, np.int64)
    offs = np.asarray(case["track_offsets"], np.int64)
    for t in range(T):
        off, end = offs[t], offs[t + 1]
        if 0 <= off <= end <= O:
            owner[off:end] = np.maximum(owner[off:end], t)
    obs = case["obs"][:O]
    pts = np.asarray(case["points"], f32).reshape(-1, 4)
    st = np.asarray(case["point_status"], np.int32)
    oc = np.maximum(owner, 0)
    ok = (owner >= 0) & (st[oc] == 0) & np.isfinite(pts[oc, :3]).all(1) & np.isfinite(obs["xpos"]) & np.isfinite(obs["ypos"])
    ok &= (obs["frame"] >= 0) & (obs["frame"] < case["nimages"])
    return np.where(ok, obs["frame"], -1), owner


def image_candidates(case, i, keys=None):
    key, owner = candidate_keys(case) if keys is None else keys
    slots = np.nonzero(key == i)[0]
    pts = np.asarray(case["points"], f32).reshape(-1, 4)
    obs = case["obs"]
    return slots, pts[owner[slots], :3], np.stack([obs["xpos"][slots], obs["ypos"][slots]], 1)


def per_image(case, dt=f32):
    keys = candidate_keys(case)
    cam = np.asarray(case["cam"], f32).reshape(-1, 12)
    hold = set(int(h) for h in case["hold"])
    out = []
    for i in range(case["nimages"]):
        slots, X, xy = image_candidates(case, i, keys)
        out.append(expected_camera(cam[i], int(case["cam_pair"][i]), i in hold, case["intrinsics"][i], slots, X, xy,
                                   case["min_obs"], case["num_loops"], case["max_error"], case["orthonormalise"], dt))
    return out


def expected_refine(case):
    """The six outputs of the call as uint32 arrays of exactly the stated sizes, and the per-image dicts under 'images'."""
    n = case["nimages"]
    imgs = per_image(case)
    cam_in = np.ascontiguousarray(case["cam"], f32).reshape(-1, 12).view(np.uint32)
    cam_out = np.stack([cam_in[i] if e["as_given"] else e["cam"].astype(f32).view(np.uint32) for i, e in enumerate(imgs)])
    summary = np.zeros(8, np.int32)
    summary[0] = counts(case)[0]
    for e in imgs:
        summary[(1, 3, 4, 5, 7)[e["status"]]] += 1
        summary[2] += e["nobs"] if e["status"] == OK else 0
        summary[6] += e["steps"]
    return dict(cam_out=cam_out.reshape(-1), cam_obs=np.array([e["nobs"] for e in imgs], np.int32).view(np.uint32),
                cam_rms=np.stack([e["rms"].astype(f32) for e in imgs]).reshape(-1).view(np.uint32),
                cam_steps=np.array([e["steps"] for e in imgs], np.int32).view(np.uint32),
                cam_status=np.array([e["status"] for e in imgs], np.int32).view(np.uint32),
                summary=summary.view(np.uint32), images=imgs, n=n)


# ---- the hook

def hook_camera(cam12, cam_pair, held, k4, slots, X, xy, min_obs, num_loops, max_error, orth, in_place=False):
    from cudasift_amd import capi
    cam = np.ascontiguousarray(cam12, f32).copy()
    k = np.ascontiguousarray(k4, f32)
    slots, X, xy = (np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(X, f32).reshape(-1, 3),
                    np.ascontiguousarray(xy, f32).reshape(-1, 2))
    out = cam if in_place else np.full(12, 3.5, f32)
    ints, rms = np.full(3, -77, np.int32), np.full(2, 3.5, f32)
    n = len(slots)
    assert capi.lib().misift_test_refine_camera(
        cam.ctypes.data, int(cam_pair), int(bool(held)), k.ctypes.data, n, slots.ctypes.data if n else None,
        X.ctypes.data if n else None, xy.ctypes.data if n else None, min_obs, num_loops, float(max_error), int(orth),
        out.ctypes.data, ints.ctypes.data, rms.ctypes.data, ints.ctypes.data + 4, ints.ctypes.data + 8) == 0
    return dict(cam=out, nobs=int(ints[0]), rms=rms, steps=int(ints[1]), status=int(ints[2]))


# ---- cases

def refine_case(tri, points, point_status=None, hold=(), min_obs=6, num_loops=5, max_error=INF, orthonormalise=0):
    """A case of this call from a triangulate case and the points (T, 3) or (max_tracks, 4) of its tracks."""
    mt = tri["max_tracks"]
    p = np.zeros((mt, 4), f32)
    points = np.asarray(points, f32)
    p[:len(points), :points.shape[1]] = points
    st = np.zeros(mt, np.int32)
    if point_status is not None:
        st[:len(point_status)] = point_status
    case = {k: tri[k] for k in TC.CASE_KEYS if k not in ("min_views", "num_loops")}
    short = mt + 1 - len(case["track_offsets"])                  # no track at all: max_tracks is 1 all the same
    if short > 0:
        fill = np.full(short, TC.POISON_WORD, np.uint32).view(np.int32)
        case["track_offsets"] = np.concatenate([case["track_offsets"], fill])
    return dict(case, points=p, point_status=st, hold=tuple(hold), min_obs=min_obs, num_loops=num_loops,
                max_error=max_error, orthonormalise=orthonormalise)


def variant(case, **kw):
    return dict(case, **kw)


def with_counts(case, T=None, O=None):
    """T and O as the device would report them."""
    s = case["export_summary"].copy()
    if T is not None:
        s[2] = T
    if O is not None:
        s[3] = O
    return variant(case, export_summary=s)


def drifted(cams, rng, angle, shift, keep=(0,)):
    """The cameras [(R, t)] turned by up to `angle` rad and moved by `shift` (Gaussian), but for those in `keep`."""
    out = []
    for i, (R, t) in enumerate(cams):
        if i in keep:
            out.append((R.copy(), t.copy()))
            continue
        D = PC.rodrigues(rng.normal(0, 1, 3), angle * rng.uniform(0.3, 1))
        out.append((D @ R, D @ t + rng.normal(0, shift, 3)))
    return out


_SCENES = {}


def scene(frames_of, nimages, seed, noise=0.3, angle=0.01, shift=0.02, point_noise=0.0, step=0.4, **kw):
    """A planted scene: nimages cameras `step` apart, track t seen by the images frames_of[t] (a point 4 to 12 deep in
    front of the middle one), `noise` px on every position, the cameras the call is given drifted but for image 0, the
    root.  dict(case, true (the planted cameras, (n, 12) float64), X).  kw goes to refine_case."""
    key = (tuple(map(tuple, frames_of)), nimages, seed, noise, angle, shift, point_noise, step, tuple(sorted(kw.items())))
    if key in _SCENES:
        return _SCENES[key]
    rng = np.random.default_rng(seed)
    cams = TC.cameras(nimages, step, rng)
    K = [TC.INTRINSICS[i % 2] for i in range(nimages)]
    tracks, Xs = [], []
    for frames in frames_of:
        frames = list(frames)
        R, t = cams[frames[len(frames) // 2]] if frames else cams[0]
        z = rng.uniform(4, 12)
        X = R.T @ (np.array([rng.uniform(-0.3, 0.3) * z, rng.uniform(-0.2, 0.2) * z, z]) - t)
        px, depth = TC.project(cams, K, frames, X) if frames else (np.zeros((0, 2)), np.ones(0))
        assert (depth > 1).all()
        tracks.append((frames, px + rng.normal(0, noise, px.shape)))
        Xs.append(X + rng.normal(0, point_noise, 3))
    start = drifted(cams, rng, angle, shift)
    tri = TC.pack(start, K, tracks, cam_pair=[ROOT] + list(range(nimages - 1)), seed=seed)
    out = dict(case=refine_case(tri, np.array(Xs).reshape(-1, 3), **kw), X=np.array(Xs),
               true=np.array([np.concatenate([R.reshape(9), t]) for R, t in cams]))
    _SCENES[key] = out
    return out


def runs(ntracks, nimages, seed, lengths=(2, 3, 4)):
    """frames_of for scene(): runs of neighbouring images."""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for t in range(ntracks):
        m = min(lengths[t % len(lengths)], nimages)
        first = int(rng.integers(0, nimages - m + 1))
        out.append(range(first, first + m))
    return out


def spread_case(nslots, nimages=4, seed=61, **kw):
    """About nslots slots in tracks of 2 to 4 views, every image's members spread over the lane slots."""
    frames_of, total = [], 0
    for fr in runs(nslots, nimages, seed):
        if total + len(fr) > nslots:
            fr = range(fr[0], fr[0] + nslots - total)
        if len(fr):
            frames_of.append(fr)
        total += len(fr)
        if total == nslots:
            break
    sc = scene(frames_of, nimages, seed, **kw)
    assert counts(sc["case"])[1] == nslots or nslots == 0
    return sc["case"]


def one_lane_case(members=8, lane=5, seed=62, **kw):
    """Tracks of one observation each: image 1 sees exactly the slots lane, lane + 256, ..., images 2 and 3 the others."""
    rng = np.random.default_rng(seed)
    n = (members - 1) * SLOTS + lane + 40
    frames = rng.integers(2, 4, n)
    frames[lane::SLOTS] = 1
    assert (frames == 1).sum() == members
    return scene([[f] for f in frames], 4, seed, **kw)["case"]


def member_counts_case(min_obs=6, seed=63, **kw):
    """Images 1, 2, 3 with min_obs - 1, min_obs and min_obs + 1 observations, image 4 with none, image 5 with plenty."""
    frames = [1] * (min_obs - 1) + [2] * min_obs + [3] * (min_obs + 1) + [5] * 40
    frames = list(np.random.default_rng(seed).permutation(frames))
    return scene([[f] for f in frames], 6, seed, min_obs=min_obs, **kw)["case"]


def resection(n, noise, err, seed, **kw):
    """One camera (image 1) off by `err` rad and 5 * err units seen against n planted points; image 0 is the root."""
    return scene([[1]] * n, 2, seed, noise=noise, angle=err, shift=5.0 * err, **kw)


def hostile_case(**kw):
    """Every hostile input of the issue among good observations; names[i] says what image i is."""
    rng = np.random.default_rng(64)
    nimg = 10
    sc = scene(runs(150, nimg, 64, lengths=(3, 4, 5)), nimg, 64, **kw)
    case = dict(sc["case"])
    cam, pair = case["cam"].copy(), np.asarray(case["cam_pair"], np.int32).copy()
    obs, pts, st = case["obs"].copy(), case["points"].copy(), case["point_status"].copy()
    names = ["root", "held", "good", "unset", "a NaN", "an inf", "good", "behind", "good", "good"]
    pair[3] = UNSET
    cam[4, 7], cam[5, 9] = np.nan, -np.inf
    T, O = counts(case)
    offs = case["track_offsets"]
    st[10:14] = [1, 2, 3, 4]                                     # points of every failed status
    pts[10:14, :3] = rng.normal(0, 1, (4, 3))                    # with finite coordinates, so the status decides
    pts[14, 1], pts[15, 0], pts[16, 2] = np.nan, np.inf, -np.inf  # status 0, non-finite
    o = np.arange(O)
    obs["frame"][o[20]], obs["frame"][o[33]] = -1, nimg
    obs["frame"][o[47]], obs["frame"][o[48]] = 2 ** 31 - 1, -2 ** 31
    obs["xpos"][o[60]], obs["ypos"][o[61]], obs["xpos"][o[62]] = np.nan, np.inf, -np.inf
    # image 7 sees three points that lie behind it
    R, t = cam[7, :9].reshape(3, 3).astype(np.float64), cam[7, 9:].astype(np.float64)
    seen = np.nonzero(obs["frame"][:O] == 7)[0][:3]
    owner = np.searchsorted(offs[:T + 1], seen, side="right") - 1
    for tr in owner:
        pts[tr, :3] = R.T @ (np.array([0.1, -0.2, -rng.uniform(2, 5)]) - t)
    case.update(cam=cam, cam_pair=pair, obs=obs, points=pts, point_status=st, hold=(1,), names=names, behind=owner)
    return case


def bad_offsets_case(**kw):
    """Offsets that are negative, decrease, overlap and pass O; the owner of a slot is the largest valid track."""
    sc = scene(runs(40, 4, 65, lengths=(3, 4)), 4, 65, **kw)
    case = dict(sc["case"])
    offs = case["track_offsets"].copy()
    T, O = counts(case)
    offs[5] = -3                                                 # track 4 ends below 0, track 5 starts there: no owner
    offs[9] = offs[7]                                            # track 8 decreases; track 9 overlaps 7 and 8 and owns them
    offs[20] = O + 5                                             # track 19 ends beyond O, track 20 starts there
    case["track_offsets"] = offs
    return case


def chain_start(orthonormalise=1, **kw):
    """The triangulate chain case (64 linked cameras with their drift, exact observations) with the points the
    restatement of triangulate gives under them."""
    key = ("chain", orthonormalise, tuple(sorted(kw.items())))
    if key not in _SCENES:
        sc = TC.chain_case()
        with np.errstate(all="ignore"):
            e = TC.expected_triangulate(sc["case"], obs_error=False)
        case = refine_case(sc["case"], e["points"].view(f32).reshape(-1, 4), e["point_status"].view(np.int32),
                           orthonormalise=orthonormalise, **kw)
        _SCENES[key] = dict(case=case, gt=sc["gt"], X=sc["X"])
    return _SCENES[key]


def triangulate_under(case, cam, num_loops=5):
    """The restatement of triangulate under other cameras: (points (max_tracks, 4) f32, status, obs_error f32)."""
    tri = {k: case[k] for k in TC.CASE_KEYS if k in case}
    tri.update(cam=np.ascontiguousarray(cam, f32).reshape(-1, 12), min_views=2, num_loops=num_loops, memo={})
    with np.errstate(all="ignore"):
        e = TC.expected_triangulate(tri)
    T = counts(case)[0]
    pts = e["points"].view(f32).reshape(-1, 4).copy()
    st = e["point_status"].view(np.int32).copy()
    pts[T:], st[T:] = 0, 4
    return pts, st, e["obs_error"].view(f32)


def rejected_step_case():
    """Twelve exact observations of a camera 1e-4 rad off: the first step reaches the rounding floor, the second is
    turned away as no better."""
    return resection(12, 0.0, 1e-4, 70, num_loops=5)["case"]


def behind_trial_case():
    """Six exact observations of a camera 0.3 rad and 2 units off: the first trial step puts a member behind it."""
    return scene([[1]] * 6, 2, 114, noise=0.0, angle=0.3, shift=2.0, num_loops=5)["case"]

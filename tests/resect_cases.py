"""misift_resect_cameras_batch: expected_resect, the numpy restatement of the definition in include/misift.h, the wrappers
of the library's host hooks, and the cases of its tests (test_resect_cpu.py pins the restatement to the hooks and to
float64 and asserts the premises of the cases, test_gpu_resect.py holds the device to it byte for byte).  A case is a
refine case (refine_cases.refine_case: the observation lists, the points and their status, the cameras) with the call's
own arguments: images, seeds, max_cand, num_loops, thresh, min_inliers, only_unset, install.  The restatement takes its
number format as an argument: with float32 every operation is rounded as the library rounds it, with float64 the same
algorithm is the yardstick.  No GPU in here, and cudasift_amd.capi is imported inside functions only."""
import numpy as np

import refine_cases as RC
import triangulate_cases as TC
from test_fundamental_cpu import f32, libc_stream

OK, FEW_CAND, NO_MODEL, SKIPPED, OVER = 0, 1, 2, 3, 4
UNSET, ROOT, RESECTED = RC.UNSET, RC.ROOT, -3
SWEEPS = 6
OUTPUTS = ("res_cam", "res_cand", "res_inliers", "res_status", "summary")


# ---- the definition restated

def draw6(seed, n, num_loops):
    """Step 3: (num_loops, 6) positions: per hypothesis six draws first, then p[1..5] in turn redrawn while they repeat an
    earlier one; all hypotheses from one stream."""
    need = 16 * num_loops + 64
    while True:
        r = iter(libc_stream(seed, need).tolist())
        out = np.zeros((num_loops, 6), np.int64)
        try:
            for i in range(num_loops):
                p = [next(r) % n for _ in range(6)]
                for k in range(1, 6):
                    while p[k] in p[:k]:
                        p[k] = next(r) % n
                out[i] = p
            return out
        except StopIteration:
            need *= 4


def scale(dt):
    """6 sqrt(3): the constant as the header writes it in float32, the number itself in float64."""
    return f32(10.3923048) if dt is f32 else dt(6.0) * np.sqrt(dt(3.0))


def null_vector(A, dt):
    """Step 4b on (L, 11, 12) systems: (P (L, 12), ok (L,)).  A is overwritten."""
    L = A.shape[0]
    ar = np.arange(L)
    col = np.tile(np.arange(12), (L, 1))
    ok = np.ones(L, bool)
    for k in range(11):
        mag = np.abs(A[:, k:, k:]).reshape(L, -1)
        mag = np.where(np.isnan(mag), dt(-1), mag)               # a NaN never wins
        j = np.argmax(mag, 1)                                    # row-major, the first maximum
        pr, pc = k + j // (12 - k), k + j % (12 - k)
        t = A[ar, k, :].copy(); A[ar, k, :] = A[ar, pr, :]; A[ar, pr, :] = t                # noqa: E702
        t = A[ar, :, k].copy(); A[ar, :, k] = A[ar, :, pc]; A[ar, :, pc] = t                # noqa: E702
        t = col[ar, k].copy(); col[ar, k] = col[ar, pc]; col[ar, pc] = t                    # noqa: E702
        piv = A[:, k, k].copy()
        ok &= (piv != 0) & np.isfinite(piv)
        for r in range(k + 1, 11):
            f = A[:, r, k] / piv
            A[:, r, k + 1:] = A[:, r, k + 1:] - f[:, None] * A[:, k, k + 1:]
    z = np.zeros((L, 12), dt)
    z[:, 11] = 1
    for k in range(10, -1, -1):
        s = np.zeros(L, dt)
        for c in range(k + 1, 12):
            s = s + A[:, k, c] * z[:, c]
        z[:, k] = (-s) / A[:, k, k]
    P = np.zeros((L, 12), dt)
    P[ar[:, None], col] = z
    return P, ok


def camera_of(P, c, s, dt):
    """Step 4c on (L, 12) null vectors with the centroids c (three (L,) arrays) and scales s: (cam (L, 12), ok)."""
    one, two = dt(1), dt(2)
    ok = np.isfinite(P).all(1)
    m = np.abs(P).max(1)
    ok &= m != 0
    P = P / m[:, None]
    p = [P[:, j] for j in range(12)]
    det = (p[0] * (p[5] * p[10] - p[6] * p[9]) - p[1] * (p[4] * p[10] - p[6] * p[8])) + p[2] * (p[4] * p[9] - p[5] * p[8])
    ok &= (det != 0) & np.isfinite(det)
    P = np.where((det < 0)[:, None], -P, P)
    A = [[P[:, 4 * r + q].copy() for q in range(3)] for r in range(3)]
    V = [[np.full(len(P), 1 if r == q else 0, dt) for q in range(3)] for r in range(3)]

    def dot(M, i, j):
        return M[0][i] * M[0][j] + M[1][i] * M[1][j] + M[2][i] * M[2][j]

    for _ in range(SWEEPS):
        for a, b in ((0, 1), (0, 2), (1, 2)):
            alpha, beta, gamma = dot(A, a, a), dot(A, b, b), dot(A, a, b)
            skip = gamma == 0
            zeta = (beta - alpha) / (two * gamma)
            tau = one / (np.abs(zeta) + np.sqrt(one + zeta * zeta))
            tau = np.where(zeta < 0, -tau, tau)
            cs = one / np.sqrt(one + tau * tau)
            sn = cs * tau
            for M in (A, V):
                for r in range(3):
                    ma, mb = M[r][a], M[r][b]
                    M[r][a] = np.where(skip, ma, cs * ma - sn * mb)
                    M[r][b] = np.where(skip, mb, sn * ma + cs * mb)
    sg = [np.sqrt(dot(A, j, j)) for j in range(3)]
    for j in range(3):
        ok &= np.isfinite(sg[j]) & (sg[j] > 0)
    U = [[A[r][j] / sg[j] for j in range(3)] for r in range(3)]
    cam = np.zeros((len(P), 12), dt)
    for r in range(3):
        for q in range(3):
            cam[:, 3 * r + q] = (U[r][0] * V[q][0] + U[r][1] * V[q][1]) + U[r][2] * V[q][2]
    lam = ((sg[0] + sg[1]) + sg[2]) / dt(3)
    for r in range(3):
        tn = P[:, 4 * r + 3] / lam
        cam[:, 9 + r] = tn / s - ((cam[:, 3 * r] * c[0] + cam[:, 3 * r + 1] * c[1]) + cam[:, 3 * r + 2] * c[2])
    ok &= np.isfinite(cam).all(1)
    return cam, ok


def solve6(xy, X, k4, dt=f32):
    """Step 4 for L samples: xy (L, 6, 2) and X (L, 6, 3) float32, k4 = fx fy cx cy.  Returns cam (L, 12) of dt and valid
    (L,); an invalid hypothesis is twelve zeros."""
    xy, X = np.asarray(xy, f32).astype(dt), np.asarray(X, f32).astype(dt)
    k = [dt(f32(v)) for v in k4]
    L = xy.shape[0]
    with np.errstate(all="ignore"):
        u, v = (xy[:, :, 0] - k[2]) / k[0], (xy[:, :, 1] - k[3]) / k[1]
        S = [np.zeros(L, dt) for _ in range(3)]
        for j in range(6):
            for a in range(3):
                S[a] = S[a] + X[:, j, a]
        c = [S[a] / dt(6) for a in range(3)]
        d = np.zeros(L, dt)
        for j in range(6):
            dx, dy, dz = X[:, j, 0] - c[0], X[:, j, 1] - c[1], X[:, j, 2] - c[2]
            d = d + np.sqrt((dx * dx + dy * dy) + dz * dz)
        s = scale(dt) / d
        n = [(X[:, :, a] - c[a][:, None]) * s[:, None] for a in range(3)]
        A = np.zeros((L, 11, 12), dt)
        for j in range(6):
            for r, w, at in ((2 * j, u[:, j], 0), (2 * j + 1, v[:, j], 4)):
                if r == 11:
                    continue                                     # point 5 has no v-row
                for a in range(3):
                    A[:, r, at + a] = n[a][:, j]
                    A[:, r, 8 + a] = -(w * n[a][:, j])
                A[:, r, at + 3] = 1
                A[:, r, 11] = -w
        P, ok = null_vector(A, dt)
        cam, ok2 = camera_of(P, c, s, dt)
        ok &= ok2
    cam[~ok] = 0
    return cam, ok


def count_inliers(cams, k4, X, xy, thresh, dt=f32):
    """Step 5: the inliers of every hypothesis (L,) over the candidates X (n, 3), xy (n, 2)."""
    k = np.asarray(k4, f32).astype(dt)
    X, xy = np.asarray(X, f32).astype(dt), np.asarray(xy, f32).astype(dt)
    thresh2 = f32(thresh) * f32(thresh) if dt is f32 else dt(f32(thresh)) * dt(f32(thresh))
    out = np.zeros(len(cams), np.int64)
    with np.errstate(all="ignore"):
        for at in range(0, len(cams), 128):
            c = [np.asarray(cams[at:at + 128, j], dt)[:, None] for j in range(12)]
            _, _, zc, _, _, _, ru, rv = RC.view(c, k, X, xy[:, 0], xy[:, 1], dt)
            front = zc > 0
            out[at:at + 128] = (front if np.isinf(thresh2) else front & (ru * ru + rv * rv < thresh2)).sum(1)
    return out


def search(seed, k4, X, xy, num_loops, thresh, dt=f32):
    """Steps 3 to 6 over n >= 6 candidates: dict(cams, valid, counts, index, inliers, samples)."""
    pos = draw6(seed, len(X), num_loops)
    X, xy = np.asarray(X, f32), np.asarray(xy, f32)
    cams, valid = solve6(xy[pos], X[pos], k4, dt)
    counts = count_inliers(cams, k4, X, xy, thresh, dt)
    idx = int(np.argmax(counts))                                 # the first maximum
    return dict(cams=cams, valid=valid, counts=counts, index=idx, inliers=int(counts[idx]), samples=pos)


def expected_entry(case, e, keys=None, dt=f32):
    """One entry: dict(cam (12,), cand, inliers, status) and, where the search ran, what search() returns under 'search'."""
    i = int(case["images"][e])
    out = dict(cam=np.zeros(12, dt), cand=0, inliers=0, status=OK, image=i, search=None)
    if case["only_unset"] and int(case["cam_pair"][i]) != UNSET:
        out["status"] = SKIPPED
        return out
    slots, X, xy = RC.image_candidates(case, i, keys)
    n = out["cand"] = len(slots)
    if n > case["max_cand"]:
        out["status"] = OVER
        return out
    if n < max(6, case["min_inliers"]):
        out["status"] = FEW_CAND
        return out
    memo = case.setdefault("memo_resect", {})
    key = (i, int(case["seeds"][e]), case["num_loops"], float(case["thresh"]), dt, id(case["obs"]), id(case["points"]),
           id(case["track_offsets"]), id(case["export_summary"]), id(case["point_status"]))
    if key not in memo:
        memo[key] = search(int(case["seeds"][e]), case["intrinsics"][i], X, xy, case["num_loops"], case["thresh"], dt)
    s = out["search"] = memo[key]
    out["inliers"] = s["inliers"]
    if s["inliers"] < case["min_inliers"]:
        out["status"] = NO_MODEL
        return out
    out["cam"] = s["cams"][s["index"]].copy()
    return out


def expected_resect(case):
    """The five outputs of the call as uint32 arrays of exactly the stated sizes, cam and cam_pair as the call leaves them,
    and the per-entry dicts under 'entries'."""
    keys = RC.candidate_keys(case)
    ents = [expected_entry(case, e, keys) for e in range(len(case["images"]))]
    cam = np.ascontiguousarray(case["cam"], f32).reshape(-1, 12).copy()
    pair = np.ascontiguousarray(case["cam_pair"], np.int32).copy()
    summary = np.zeros(8, np.int32)
    summary[0] = RC.counts(case)[0]
    for x in ents:
        summary[(1, 3, 4, 5, 6)[x["status"]]] += 1
        if x["status"] == OK:
            summary[2] += x["inliers"]
            if case["install"]:
                cam[x["image"]], pair[x["image"]] = x["cam"].astype(f32), RESECTED
    res_cam = np.array([x["cam"] for x in ents], f32).reshape(-1)
    ints = {k: np.array([x[k] for x in ents], np.int32).view(np.uint32) for k in ("cand", "inliers", "status")}
    return dict(res_cam=res_cam.view(np.uint32), res_cand=ints["cand"], res_inliers=ints["inliers"],
                res_status=ints["status"], summary=summary.view(np.uint32), cam=cam.reshape(-1).view(np.uint32),
                cam_pair=pair.view(np.uint32), entries=ents)


# ---- the hooks

def hook_samples(seed, n, num_loops):
    from cudasift_amd import capi
    out = np.full((max(num_loops, 1), 6), -77, np.int32)
    assert capi.lib().misift_test_resect_samples(seed, n, num_loops, out.ctypes.data) == 0
    return out[:num_loops]


def hook_solve(xy, X, k4):
    """The library's solve of one sample: (cam (12,) float32, valid)."""
    from cudasift_amd import capi
    rows = np.ascontiguousarray(np.concatenate([np.asarray(xy, f32).reshape(6, 2), np.asarray(X, f32).reshape(6, 3)], 1))
    k = np.ascontiguousarray(k4, f32)
    cam, valid = np.full(12, 3.5, f32), np.full(1, -77, np.int32)
    assert capi.lib().misift_test_resect_solve(rows.ctypes.data, k.ctypes.data, cam.ctypes.data, valid.ctypes.data) == 0
    return cam, int(valid[0])


# ---- cases

_SCENES = {}


def resect_case(base, images, seeds=None, max_cand=2048, num_loops=64, thresh=4.0, min_inliers=6, only_unset=0,
                install=0, **kw):
    images = np.asarray(images, np.int32).reshape(-1)
    seeds = np.asarray([100 + 7 * e for e in range(len(images))] if seeds is None else seeds, np.uint32).reshape(-1)
    case = {k: v for k, v in base.items() if k not in ("memo", "memo_resect")}
    case.update(images=images, seeds=seeds, max_cand=max_cand, num_loops=num_loops, thresh=thresh, min_inliers=min_inliers,
                only_unset=only_unset, install=install, memo_resect=base.setdefault("memo_resect", {}), **kw)
    return case


def variant(case, **kw):
    """The same scene under other arguments; the memo of searches is shared (its key holds what a search depends on)."""
    out = dict(case, **kw)
    for k in ("images", "seeds"):
        out[k] = np.asarray(out[k], np.uint32 if k == "seeds" else np.int32).reshape(-1)
    return out


def planted(counts, seed, wrong=0.25, noise=0.5, shape="volume", slack_tracks=0, slack_obs=0, behind=0):
    """A planted scene: image i sees counts[i] points of its own, each a track of one observation, the slots of all images
    shuffled together.  A share `wrong` of an image's observations is anywhere in the frame, the others carry `noise` px;
    `behind` further points per image lie behind its camera.  shape: 'volume' (4 to 12 deep), 'plane' (the world plane
    Z = 4, exactly), 'point' (every point of an image the same).  No image has a camera yet (d_cam_pair = -2, zeros).
    dict(case (a refine case), true (n, 12) float64, good: per image the slots of its planted inliers)."""
    key = (tuple(counts), seed, wrong, noise, shape, slack_tracks, slack_obs, behind)
    if key in _SCENES:
        return _SCENES[key]
    rng = np.random.default_rng(seed)
    nimg = len(counts)
    cams = TC.cameras(nimg, 0.4, rng)
    K = [TC.INTRINSICS[i % 2] for i in range(nimg)]
    rows = []                                                    # (image, X, px, good)
    for i, n in enumerate(counts):
        R, t = cams[i]
        bad = set(rng.choice(n, int(round(wrong * n)), replace=False).tolist()) if n else set()
        same = None
        for j in range(n + behind):
            z = rng.uniform(4, 12) * (-1 if j >= n else 1)
            Xc = np.array([rng.uniform(-0.3, 0.3) * z, rng.uniform(-0.2, 0.2) * z, z])
            X = R.T @ (Xc - t)
            if shape == "plane":
                X = np.array([X[0], X[1], 4.0])
            if shape == "point":
                same = X if same is None else same
                X = same
            X = X.astype(f32).astype(np.float64)                 # what the call is given
            px, _ = TC.project(cams, K, [i], X)
            px = px[0] + rng.normal(0, noise, 2)
            if j in bad:
                px = rng.uniform([0, 0], [1920, 1080])
            rows.append((i, X, px, j < n and j not in bad))
    order = rng.permutation(len(rows))
    rows = [rows[j] for j in order]
    tracks = [([r[0]], r[2][None, :]) for r in rows]
    zero = [(np.zeros((3, 3)), np.zeros(3)) for _ in range(nimg)]
    tri = TC.pack(zero, K, tracks, cam_pair=[UNSET] * nimg, slack_tracks=slack_tracks, slack_obs=slack_obs, seed=seed)
    case = RC.refine_case(tri, np.array([r[1] for r in rows]).reshape(-1, 3))
    good = {i: np.array([o for o, r in enumerate(rows) if r[0] == i and r[3]], np.int64) for i in range(nimg)}
    out = dict(case=case, good=good, true=np.array([np.concatenate([R.reshape(9), t]) for R, t in cams]))
    _SCENES[key] = out
    return out


def pose_error(cam, true12):
    """(the rotation angle in rad, the distance of the camera centres) between a camera and the planted one, in float64."""
    cam, true12 = np.asarray(cam, np.float64), np.asarray(true12, np.float64)
    R, t, Rt, tt = cam[:9].reshape(3, 3), cam[9:], true12[:9].reshape(3, 3), true12[9:]
    cosang = np.clip((np.trace(R @ Rt.T) - 1) / 2, -1, 1)
    return float(np.arccos(cosang)), float(np.linalg.norm(-R.T @ t + Rt.T @ tt))


EDGE_COUNTS = (0, 5, 6, 7, 511, 512, 513, 1025)                  # either side of 6 and of one and two count chunks


def edge_scene():
    return planted(EDGE_COUNTS, 71)


def small_scene(**kw):
    """Four images of 40, 60, 24 and 90 points in front and three behind each, with room behind T and O."""
    return planted((40, 60, 24, 90), 72, slack_tracks=9, slack_obs=21, behind=3, **kw)


def exact_scene():
    """Two images of 30 and 12 candidates without noise or wrong observations: many hypotheses collect every one."""
    return planted((30, 12), 73, wrong=0.0, noise=0.0)


def hostile_case(**kw):
    """The small scene with hostile inputs among the good ones: failed and non-finite points, non-finite observations,
    frames outside the images."""
    case = dict(small_scene()["case"])
    T, O = RC.counts(case)
    obs, pts, st = case["obs"].copy(), case["points"].copy(), case["point_status"].copy()
    st[10:14] = [1, 2, 3, 4]
    pts[14, 1], pts[15, 0], pts[16, 2] = np.nan, np.inf, -np.inf
    obs["frame"][20], obs["frame"][33], obs["frame"][47], obs["frame"][48] = -1, case["nimages"], 2 ** 31 - 1, -2 ** 31
    obs["xpos"][60], obs["ypos"][61], obs["xpos"][62] = np.nan, np.inf, -np.inf
    case.update(obs=obs, points=pts, point_status=st)
    case.pop("memo_resect", None)
    return resect_case(case, [0, 1, 3], **kw)


def bad_offsets_case(**kw):
    """Offsets that are negative, decrease, overlap and pass O; the owner of a slot is the largest valid track, so slot 7
    is seen with the point of track 9."""
    case = dict(small_scene()["case"])
    offs = case["track_offsets"].copy()
    T, O = RC.counts(case)
    offs[5] = -3
    offs[9] = offs[7]
    offs[20] = O + 5
    case["track_offsets"] = offs
    case.pop("memo_resect", None)
    return resect_case(case, [1, 3, 0], **kw)


def mixed_pairs_case(install, only_unset=1, **kw):
    """The small scene with d_cam_pair = (-2, -1, a pair index, -3) and cameras already there for the last three."""
    sc = small_scene()
    case = dict(sc["case"])
    cam = case["cam"].copy()
    cam[1:] = sc["true"][1:].astype(f32)
    case.update(cam=cam, cam_pair=np.array([UNSET, ROOT, 1, RESECTED], np.int32))
    return resect_case(case, [3, 0, 2, 1], only_unset=only_unset, install=install, **kw)


# the names of gpu_cases(), so that collecting the GPU tests builds nothing
GPU_CASES = (
    "T -1 O 226", "T -2147483648 O -2147483648", "T 100 O 100", "T 150 O 226", "T 2147483647 O 2147483647",
    "T 226 O -5", "T 226 O 100", "T 300 O 1000000000", "bad offsets", "candidates 0 5 6", "candidates 513 1025",
    "candidates 7 511 512", "coplanar", "hostile", "install over set cameras", "max_cand 1025",
    "max_cand one below n", "min_inliers count +0", "min_inliers count +1", "min_inliers count -1", "no candidates",
    "nsel 0", "nsel 3 of different status", "num_loops 1", "num_loops 100", "num_loops 63", "num_loops 64",
    "num_loops 65", "one point", "only_unset, install 0", "only_unset, install 1", "seed a", "seed b", "thresh inf",
    "tie",
)


def gpu_cases():
    """name -> case: everything test_gpu_resect.py compares byte for byte; test_resect_cpu.py asserts what each is built
    to hit."""
    if "gpu" in _SCENES:
        return _SCENES["gpu"]
    edge, small, exact = edge_scene()["case"], small_scene()["case"], exact_scene()["case"]
    out = {}
    out["candidates 0 5 6"] = resect_case(edge, [0, 1, 2], max_cand=1030, num_loops=64)
    out["candidates 7 511 512"] = resect_case(edge, [3, 4, 5], max_cand=1030, num_loops=65)
    out["candidates 513 1025"] = resect_case(edge, [7, 6], max_cand=1030, num_loops=100, min_inliers=12)
    out["max_cand one below n"] = resect_case(edge, [5, 6, 7], max_cand=512, num_loops=16)
    out["max_cand 1025"] = resect_case(edge, [7], max_cand=1025, num_loops=33)
    for L in (1, 63, 64, 65, 100):
        out["num_loops %d" % L] = resect_case(small, [1], num_loops=L, max_cand=91)
    out["nsel 0"] = resect_case(small, [])
    out["nsel 3 of different status"] = resect_case(small, [2, 3, 0], max_cand=60, min_inliers=28, num_loops=48)
    T0, O0 = RC.counts(small)
    assert T0 < small["max_tracks"] and O0 < small["max_obs"]
    for T, O in ((-1, O0), (150, O0), (T0, 100), (small["max_tracks"] + 65, 10 ** 9), (2 ** 31 - 1, 2 ** 31 - 1), (T0, -5),
                 (100, 100), (-2 ** 31, -2 ** 31)):
        out["T %d O %d" % (T, O)] = resect_case(RC.with_counts(small, T, O), [0, 3], num_loops=32)
    out["hostile"] = hostile_case(num_loops=48)
    out["bad offsets"] = bad_offsets_case(num_loops=48)
    out["one point"] = resect_case(planted((20, 9), 74, shape="point")["case"], [0, 1], num_loops=40)
    out["coplanar"] = resect_case(planted((50, 30), 75, shape="plane")["case"], [1, 0], num_loops=80)
    out["no candidates"] = resect_case(edge, [0], num_loops=8)
    base = resect_case(small, [3], num_loops=64)
    c = expected_entry(base, 0)["inliers"]
    for d in (-1, 0, 1):
        out["min_inliers count %+d" % d] = variant(base, min_inliers=c + d)
    for install in (0, 1):
        out["only_unset, install %d" % install] = mixed_pairs_case(install, num_loops=64)
    out["install over set cameras"] = mixed_pairs_case(1, only_unset=0, num_loops=100)
    out["seed a"] = resect_case(small, [0, 1], seeds=[1, 2], num_loops=64)
    out["seed b"] = resect_case(small, [0, 1], seeds=[3, 0], num_loops=64)
    out["tie"] = resect_case(exact, [0, 1], num_loops=64, thresh=1.0)
    out["thresh inf"] = resect_case(small, [0], num_loops=16, thresh=np.inf)
    assert sorted(out) == sorted(GPU_CASES)
    _SCENES["gpu"] = out
    return out

"""misift_recover_pose_batch: expected_pose, the numpy float32 restatement of steps 1-7 of the definition in
include/misift.h, and the scenes and hostile inputs of its tests (test_pose_cpu.py pins the restatement to the library's
host hooks and to float64, test_gpu_pose.py holds the device to it byte for byte).  No GPU in here, and
cudasift_amd.capi is imported inside functions only."""
import numpy as np

from test_fundamental_cpu import GATES, f32, gate, sampson

POS = ("xpos", "ypos", "match_xpos", "match_ypos")
SWEEPS = 6
NAN_BITS = 0x7FC00000
ONE_NAN = np.uint32(NAN_BITS).view(f32)
K_A = (1500.0, 1500.0, 960.0, 540.0)
K_B = (1200.0, 1250.0, 900.0, 500.0)
K_UNIT = (1.0, 1.0, 0.0, 0.0)
THRESH = 3.0                                                     # px, the scenes' inlier threshold


# ---- the expected answer, restated in numpy: scalars in steps 1-4, one array over the records in steps 5 and 7

def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def essential(F, K8):
    """Step 1: (E before the division as (3, 3) float32, A = E / m or None for an invalid entry)."""
    F = np.ascontiguousarray(F, f32).reshape(3, 3)
    fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2 = (f32(v) for v in K8)
    G, E = np.zeros((3, 3), f32), np.zeros((3, 3), f32)
    with np.errstate(all="ignore"):
        for r in range(3):
            G[r, 0] = F[r, 0] * fx1
            G[r, 1] = F[r, 1] * fy1
            G[r, 2] = (F[r, 0] * cx1 + F[r, 1] * cy1) + F[r, 2]
        for c in range(3):
            E[0, c] = fx2 * G[0, c]
            E[1, c] = fy2 * G[1, c]
            E[2, c] = (cx2 * G[0, c] + cy2 * G[1, c]) + G[2, c]
        if not np.isfinite(E).all():
            return E, None
        m = np.abs(E).max()
        if m == 0:
            return E, None
        return E, (E / m).astype(f32)


def decompose(F, K8, sweeps=SWEEPS, trace=None):
    """Steps 1-4: (the four hypotheses as (4, 12) float32, R row-major then t; valid).  An invalid entry gives zeros.
    trace, a list, receives the gamma of every column pair in the order they are visited."""
    zeros = np.zeros((4, 12), f32)
    _, A = essential(F, K8)
    if A is None:
        return zeros, False
    A = A.copy()
    V = np.eye(3, dtype=f32)
    one, two = f32(1), f32(2)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                alpha = _dot(A[:, p], A[:, p])
                beta = _dot(A[:, q], A[:, q])
                gamma = _dot(A[:, p], A[:, q])
                if trace is not None:
                    trace.append(gamma)
                if gamma == 0:
                    continue
                zeta = (beta - alpha) / (two * gamma)
                tau = one / (np.abs(zeta) + np.sqrt(one + zeta * zeta))
                if zeta < 0:
                    tau = -tau
                c = one / np.sqrt(one + tau * tau)
                s = c * tau
                for M in (A, V):
                    mp, mq = M[:, p].copy(), M[:, q].copy()
                    M[:, p] = c * mp - s * mq
                    M[:, q] = s * mp + c * mq
        w = [_dot(A[:, j], A[:, j]) for j in range(3)]
        i1 = 0
        for j in (1, 2):
            if w[j] > w[i1]:
                i1 = j
        ja, jb = [j for j in range(3) if j != i1]
        i2 = jb if w[jb] > w[ja] else ja
        if not w[i2] > 0:
            return zeros, False
        u1, u2 = A[:, i1] / np.sqrt(w[i1]), A[:, i2] / np.sqrt(w[i2])
        u3 = _cross(u1, u2)
        v1, v2 = V[:, i1], V[:, i2]
        v3 = _cross(v1, v2)
        Ra, Rb = np.zeros((3, 3), f32), np.zeros((3, 3), f32)
        for r in range(3):
            for c in range(3):
                Ra[r, c] = (u2[r] * v1[c] - u1[r] * v2[c]) + u3[r] * v3[c]
                Rb[r, c] = (u1[r] * v2[c] - u2[r] * v1[c]) + u3[r] * v3[c]
        t = np.array(u3, f32)
    out = np.zeros((4, 12), f32)
    for k in range(4):
        out[k, :9] = (Ra if k < 2 else Rb).reshape(9)
        out[k, 9:] = -t if k & 1 else t
    return out, True


def depth_terms(pose12, K8, xy):
    """Step 5 for every row of xy (n, 4) under one pose: (den, n1, n2, p1x, p1y), float32 arrays."""
    xy = np.ascontiguousarray(xy, f32).reshape(-1, 4)
    fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2 = (f32(v) for v in K8)
    R, t = np.asarray(pose12[:9], f32).reshape(3, 3), [f32(v) for v in pose12[9:]]
    one = np.ones(len(xy), f32)
    with np.errstate(all="ignore"):
        p1 = ((xy[:, 0] - cx1) / fx1, (xy[:, 1] - cy1) / fy1, one)
        p2 = ((xy[:, 2] - cx2) / fx2, (xy[:, 3] - cy2) / fy2, one)
        a = [R[r, 0] * p1[0] + R[r, 1] * p1[1] + R[r, 2] * p1[2] for r in range(3)]
        n = _cross(a, p2)
        p2t, at = _cross(p2, t), _cross(a, t)
        return _dot(n, n), _dot(p2t, n), _dot(at, n), p1[0], p1[1]


def in_front(den, n1, n2):
    with np.errstate(all="ignore"):
        return (den > 0) & (n1 > 0) & (n2 > 0)


def xyz_rows(valid, den, n1, n2, p1x, p1y):
    """Step 7: (n, 4) float32."""
    with np.errstate(all="ignore"):
        z1, z2 = n1 / den, n2 / den
        out = np.stack([z1 * p1x, z1 * p1y, z1, z2], 1).astype(f32)
        out = np.where(np.isnan(out), ONE_NAN, out)
        ok = (den > 0) & valid
        return np.where(ok[:, None], out, ONE_NAN).astype(f32)


def coordinates(recs, n):
    p = recs[:max(int(n), 0)]
    return np.ascontiguousarray(np.stack([p[k] for k in POS], 1), f32).reshape(len(p), 4)


def inliers_under(recs, n, F, min_score, max_ambiguity, thresh):
    """inl(F) over the first max(n, 0) records."""
    p = recs[:max(int(n), 0)]
    e2, den = sampson(F, p["xpos"], p["ypos"], p["match_xpos"], p["match_ypos"])
    with np.errstate(all="ignore"):
        t2 = f32(thresh) * f32(thresh)
        return gate(p, min_score, max_ambiguity) & (e2[0] < t2 * den[0])


def expected_pose(recs, n, F, K8, min_score, max_ambiguity, thresh):
    """One entry: dict(pose (12,) float32, num_front, votes (4,) int32, xyz (max(n, 0), 4) float32, valid, best, hyps)."""
    hyps, valid = decompose(F, K8)
    xy = coordinates(recs, n)
    votes = np.zeros(4, np.int32)
    if valid:
        member = inliers_under(recs, n, F, min_score, max_ambiguity, thresh)
        for k in range(4):
            den, n1, n2, _, _ = depth_terms(hyps[k], K8, xy)
            votes[k] = int((in_front(den, n1, n2) & member).sum())
    best = int(np.argmax(votes))                                 # the largest vote at the smallest k
    den, n1, n2, p1x, p1y = depth_terms(hyps[best], K8, xy)
    xyz = xyz_rows(valid, den, n1, n2, p1x, p1y)
    return dict(pose=hyps[best].copy(), num_front=int(votes[best]), votes=votes, xyz=xyz, valid=valid, best=best,
                hyps=hyps)


# ---- planted scenes

def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    S = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


def kmat(K4):
    fx, fy, cx, cy = K4
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])


def fit8_float64(xy):
    """The normalised 8-point fit of all rows of xy in float64: the smallest right singular vector, no rank-2 step."""
    def norm(x, y):
        cx, cy = x.mean(), y.mean()
        s = np.sqrt(2.0) / np.hypot(x - cx, y - cy).mean()
        return (x - cx) * s, (y - cy) * s, np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1]])
    xy = np.asarray(xy, np.float64)
    u1, v1, T1 = norm(xy[:, 0], xy[:, 1])
    u2, v2, T2 = norm(xy[:, 2], xy[:, 3])
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], 1)
    return T2.T @ np.linalg.svd(A)[2][-1].reshape(3, 3) @ T1


def records(xy, seed, fail=0.0):
    """Records at the positions xy (n, 4) that pass GATES, but for a share `fail` of them; every other byte random."""
    from cudasift_amd import capi
    rng = np.random.default_rng(7000 + seed)
    n = len(xy)
    recs = np.frombuffer(rng.bytes(576 * n), capi.POINT_DTYPE).copy()
    for c, k in enumerate(POS):
        recs[k] = np.asarray(xy, f32)[:, c]
    recs["score"], recs["ambiguity"] = 0.97, 0.3
    bad = rng.random(n) < fail
    recs["score"][bad & (rng.random(n) < 0.5)] = GATES[0]        # score == min_score: rejected
    recs["ambiguity"][bad & (recs["score"] > GATES[0])] = GATES[1]
    return recs


def planted(seed, n=64, k2=K_A, angle=0.3, tscale=1.0, fit=False, fscale=1.0, noise=0.5, outliers=0.0, behind=0.0):
    """Two pinhole views of n random points: dict(recs, F (9,) float32, K8, R, t (unit), inl).  F is the exact one of the
    planted pose or a float64 8-point fit of the noisy matches, scaled to a largest entry of fscale.  `outliers` of the
    matches get a random second position; `behind` of the points lie behind both cameras."""
    rng = np.random.default_rng(seed)
    X = rng.uniform([-4, -2.5, 4], [4, 2.5, 12], (n, 3))
    R = rodrigues(rng.normal(0, 1, 3), angle)
    t = rng.normal(0, 1, 3)
    t /= np.linalg.norm(t)
    if behind:
        flip = rng.random(n) < behind
        X[flip] = -X[flip]                                       # negative depth in both views (|t| < the depths)
    K1, K2 = kmat(K_A), kmat(k2)
    X2 = (R @ X.T).T + tscale * t
    p1, p2 = (K1 @ X.T).T, (K2 @ X2.T).T
    xy = np.concatenate([p1[:, :2] / p1[:, 2:], p2[:, :2] / p2[:, 2:]], 1) + rng.normal(0, noise, (n, 4))
    inl = np.ones(n, bool)
    if outliers:
        inl[rng.choice(n, int(n * outliers), replace=False)] = False
        xy[~inl, 2:] = rng.uniform([0, 0], [1920, 1080], (int((~inl).sum()), 2))
    F = fit8_float64(xy) if fit else np.linalg.inv(K2).T @ skew(t) @ R @ np.linalg.inv(K1)
    F = (F / np.abs(F).max() * fscale).astype(f32).reshape(9)
    return dict(recs=records(xy, seed), F=F, K8=np.array(K_A + tuple(k2), f32), R=R, t=t, inl=inl, xy=xy)


def planted_frame(n, seed, k2):
    """n records of a planted scene, a fifth of them wrong matches and (from 10 records on) a tenth failing the gate, with
    the scene's exact F and intrinsics."""
    s = planted(seed=seed, n=max(n, 1), k2=k2, outliers=0.2 if n >= 10 else 0.0)
    recs = records(s["xy"], seed, fail=0.1 if n >= 10 else 0.0)[:n]
    return recs, s["F"], s["K8"]


def scenes():
    """The grid of the planted scenes, three seeds each: K2 = K1 or not, 0.01 or 0.3 rad, |t| 0.05 or 1, F exact or fitted,
    and the scale of F from 1e-3 to 1e3.  (name, keyword arguments of planted())."""
    out = []
    scales = (1e-3, 1.0, 1e3, 0.03, 40.0)
    i = 0
    for k2 in (K_A, K_B):
        for angle in (0.01, 0.3):
            for tscale in (0.05, 1.0):
                for fit in (False, True):
                    for rep in range(3):
                        kw = dict(seed=100 + i, k2=k2, angle=angle, tscale=tscale, fit=fit, fscale=scales[i % 5])
                        out.append(("scene %d K2 %s angle %g |t| %g %s scale %g" % (
                            i, "= K1" if k2 == K_A else "differs", angle, tscale, "fitted" if fit else "exact",
                            scales[i % 5]), kw))
                        i += 1
    return out


_SCENES = {}


def scene(kw):
    key = tuple(sorted((k, v if not isinstance(v, tuple) else v) for k, v in kw.items()))
    if key not in _SCENES:
        _SCENES[key] = planted(**kw)
    return _SCENES[key]


# ---- hostile inputs

FORWARD = np.array([0, -1, 0, 1, 0, 0, 0, 0, 0], f32)            # [t]x of t = (0, 0, 1) with R = I: Rb is exactly I
GAMMA0 = np.array([1, 0, 0.5, 0, -1, 0, 0.5, 0, 0.25], f32)      # symmetric, rank 2, columns 0 and 1 orthogonal
K_UNIT8 = np.array(K_UNIT + K_UNIT, f32)


def forward_xy(n, seed):
    """Matches of a camera that moves one unit along its axis, in normalised coordinates (K = identity)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform([-2, -2, 3], [2, 2, 8], (n, 3))
    return np.concatenate([X[:, :2] / X[:, 2:], X[:, :2] / (X[:, 2:] + 1)], 1).astype(f32)


def hostile_matrices():
    """(name, F, K8, what decompose() must say: 'valid' or 'invalid')."""
    s = scene(dict(seed=3))
    K8, F = s["K8"], s["F"]
    nan, inf = F.copy(), F.copy()
    nan[4], inf[2] = np.nan, np.inf
    one = np.zeros(9, f32)
    one[8] = 1
    return [("zeros", np.zeros(9, f32), K8, "invalid"), ("a NaN", nan, K8, "invalid"), ("an inf", inf, K8, "invalid"),
            ("E overflows", np.full(9, 3e38, f32), K8, "invalid"),
            ("near 1e-30", (F * f32(1e-30)).astype(f32), K8, "valid"),
            ("near 1e30", (F * f32(1e30)).astype(f32), K8, "valid"),
            ("one entry", one, K8, "invalid"),
            ("gamma 0 in the first pair", GAMMA0, K_UNIT8, "valid"), ("forward motion", FORWARD, K_UNIT8, "valid")]


def hostile_frames():
    """(name, records, F, K8, thresh) of the record sets the vote and the triangulation must survive."""
    from fundamental_cases import HOSTILE
    out = []
    s = scene(dict(seed=5, n=200))
    recs = s["recs"].copy()
    rng = np.random.default_rng(11)
    rows = rng.choice(len(recs), 40, replace=False)
    for i, r in enumerate(rows):                                 # NaN, +-inf, +-1e30, 1e-40, 3e38 in one coordinate
        recs[POS[i % 4]][r] = HOSTILE[i % len(HOSTILE)]
    out.append(("non-finite coordinates", recs, s["F"], s["K8"], THRESH))
    xy = forward_xy(120, 12)
    xy[::6] = 0                                                  # at the epipole of both images
    xy[3::12, 2:] = xy[3::12, :2]                                # no parallax: a is p2
    out.append(("at the epipole", records(xy, 12), FORWARD, K_UNIT8, 1e-3))
    b = planted(seed=13, n=100, behind=1.0)
    out.append(("behind both cameras", b["recs"], b["F"], b["K8"], THRESH))
    m = planted(seed=14, n=100, behind=0.3)
    out.append(("some behind both cameras", m["recs"], m["F"], m["K8"], THRESH))
    return out


# ---- the chain find -> improve -> recover_pose

CHAIN = dict(seed=21, n=400, find_seed=9, find_loops=256, improve_loops=5, thresh=1.0)
_CHAIN = []


def chain_scene():
    return planted(seed=CHAIN["seed"], n=CHAIN["n"], k2=K_B, angle=0.3, tscale=1.0, outliers=0.25)


def expected_chain():
    """The three calls restated, computed once: dict(scene, F0, found, recs (as improve leaves them), F, fit, pose)."""
    from test_fundamental_cpu import expected_find
    from test_fundamental_refine_cpu import expected_improve
    if not _CHAIN:
        s = chain_scene()
        n, th = CHAIN["n"], CHAIN["thresh"]
        with np.errstate(all="ignore"):
            F0, found = expected_find(s["recs"], n, CHAIN["find_seed"], CHAIN["find_loops"], *GATES, th, max_pts=n)
            recs, F, fit, _ = expected_improve(s["recs"], n, F0, CHAIN["improve_loops"], *GATES, th)
            pose = expected_pose(recs, n, F, s["K8"], *GATES, th)
        _CHAIN.append(dict(scene=s, F0=F0, found=found, recs=recs, F=F, fit=fit, pose=pose))
    return _CHAIN[0]

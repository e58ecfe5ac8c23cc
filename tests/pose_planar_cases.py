"""misift_recover_pose_planar_batch: expected_planar, the numpy float32 restatement of steps 1-8 of the definition in
include/misift.h, its float64 twin (the same code run in float64), and the scenes and hostile inputs of its tests
(test_pose_planar_cpu.py pins the restatement to the library's host hooks and to float64, test_gpu_pose_planar.py holds
the device to it byte for byte).  What misift_recover_pose_batch and the fundamental calls already restate is imported
from pose_cases.py and test_fundamental_cpu.py.  No GPU in here, and cudasift_amd.capi is imported inside functions only."""
import numpy as np

import pose_cases as PC
from test_fundamental_cpu import GATES, f32, gate

f64 = np.float64
INVALID, GENERAL, PLANE, ROTATION = -1, 0, 1, 2
THRESH_H, THRESH_F = 3.0, 3.0                                    # px, the scenes' inlier thresholds
RATIO, MIN_INLIERS, MIN_BASELINE = 0.8, 8, 0.02
PARAMS = dict(thresh_h=THRESH_H, thresh_f=THRESH_F, planar_ratio=RATIO, min_inliers=MIN_INLIERS,
              min_baseline=MIN_BASELINE)


# ---- the expected answer, restated in numpy: scalars in steps 2-6, one array over the records in steps 1, 7 and 8.
# ft is the arithmetic: f32 is the restatement, f64 its twin.

def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _apply(M, v):
    return [M[r, 0] * v[0] + M[r, 1] * v[1] + M[r, 2] * v[2] for r in range(3)]


def _k8(K8, ft):
    return tuple(ft(v) for v in np.asarray(K8, f32))


def h_inliers(H, xy, thresh_h, ft=f32):
    """Step 1 without the gate: which rows of xy (n, 4) are H-inliers."""
    h = [ft(v) for v in np.asarray(H, f32).reshape(9)]
    xy = np.ascontiguousarray(np.asarray(xy, f32).reshape(-1, 4), ft)
    x1, y1, x2, y2 = xy[:, 0], xy[:, 1], xy[:, 2], xy[:, 3]
    with np.errstate(all="ignore"):
        deno = (h[6] * x1 + h[7] * y1) + h[8]
        nomx = (h[0] * x1 + h[1] * y1) + h[2]
        nomy = (h[3] * x1 + h[4] * y1) + h[5]
        errx, erry = x2 * deno - nomx, y2 * deno - nomy
        t2 = ft(f32(thresh_h)) * ft(f32(thresh_h))
        return errx * errx + erry * erry < t2 * (deno * deno)


def f_inliers(F, xy, thresh_f, ft=f32):
    """The inlier test of the fundamental calls without the gate."""
    F = [ft(v) for v in np.asarray(F, f32).reshape(9)]
    xy = np.ascontiguousarray(np.asarray(xy, f32).reshape(-1, 4), ft)
    x1, y1, x2, y2 = xy[:, 0], xy[:, 1], xy[:, 2], xy[:, 3]
    return _f_inliers(F, x1, y1, x2, y2, ft(f32(thresh_f)))


def _f_inliers(F, x1, y1, x2, y2, thresh):
    with np.errstate(all="ignore"):
        a0 = F[0] * x1 + F[1] * y1 + F[2]
        a1 = F[3] * x1 + F[4] * y1 + F[5]
        a2 = F[6] * x1 + F[7] * y1 + F[8]
        b0 = F[0] * x2 + F[3] * y2 + F[6]
        b1 = F[1] * x2 + F[4] * y2 + F[7]
        e = x2 * a0 + y2 * a1 + a2
        den = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1
        return e * e < (thresh * thresh) * den


def candidate(nH, nF, has_f, planar_ratio, min_inliers):
    """Step 2."""
    if nH < min_inliers:
        return False
    if has_f and not f32(nH) >= f32(planar_ratio) * f32(nF):
        return False
    return True


def _det(A):
    return ((A[0, 0] * (A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1]) - A[0, 1] * (A[1, 0] * A[2, 2] - A[1, 2] * A[2, 0]))
            + A[0, 2] * (A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]))


def normalise(H, K8, ft=f32):
    """Step 3: A (3, 3) or None for an invalid entry."""
    H = np.ascontiguousarray(np.asarray(H, f32).reshape(3, 3), ft)
    fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2 = _k8(K8, ft)
    G, A = np.zeros((3, 3), ft), np.zeros((3, 3), ft)
    with np.errstate(all="ignore"):
        for r in range(3):
            G[r, 0] = H[r, 0] * fx1
            G[r, 1] = H[r, 1] * fy1
            G[r, 2] = (H[r, 0] * cx1 + H[r, 1] * cy1) + H[r, 2]
        for c in range(3):
            A[0, c] = (G[0, c] - cx2 * G[2, c]) / fx2
            A[1, c] = (G[1, c] - cy2 * G[2, c]) / fy2
            A[2, c] = G[2, c]
        if not np.isfinite(A).all():
            return None
        m = np.abs(A).max()
        if m == 0:
            return None
        A = (A / m).astype(ft)
        det = _det(A)
        if det < 0:
            A = -A
            det = _det(A)
        return A if det > 0 else None


def fundamental_of(R, t, K8, ft=f32):
    """Step 7: F_k (9,) of (R (3, 3), t)."""
    fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2 = _k8(K8, ft)
    E, G, F = np.zeros((3, 3), ft), np.zeros((3, 3), ft), np.zeros((3, 3), ft)
    with np.errstate(all="ignore"):
        for c in range(3):
            E[0, c] = t[1] * R[2, c] - t[2] * R[1, c]
            E[1, c] = t[2] * R[0, c] - t[0] * R[2, c]
            E[2, c] = t[0] * R[1, c] - t[1] * R[0, c]
        for r in range(3):
            G[r, 0] = E[r, 0] / fx1
            G[r, 1] = E[r, 1] / fy1
            G[r, 2] = (E[r, 2] - G[r, 0] * cx1) - G[r, 1] * cy1
        for c in range(3):
            F[0, c] = G[0, c] / fx2
            F[1, c] = G[1, c] / fy2
            F[2, c] = (G[2, c] - cx2 * F[0, c]) - cy2 * F[1, c]
    return F.reshape(9)


def _solution(Hn, v2, u, ft):
    """Step 6 for one u: (R (3, 3), t, N, d) or None."""
    with np.errstate(all="ignore"):
        N = _cross(v2, u)
        p, q = _apply(Hn, v2), _apply(Hn, u)
        s = _cross(p, q)
        R = np.zeros((3, 3), ft)
        for r in range(3):
            for c in range(3):
                R[r, c] = (p[r] * v2[c] + q[r] * u[c]) + s[r] * N[c]
        T = [((Hn[r, 0] - R[r, 0]) * N[0] + (Hn[r, 1] - R[r, 1]) * N[1]) + (Hn[r, 2] - R[r, 2]) * N[2] for r in range(3)]
        nT = np.sqrt(_dot(T, T))
        if not (np.isfinite(nT) and nT > 0):
            return None
        return R, np.array([T[r] / nT for r in range(3)], ft), np.array(N, ft), ft(1) / nT


def decompose(H, K8, min_baseline, sweeps=PC.SWEEPS, ft=f32, trace=None):
    """Steps 3-6 and the F of step 7: dict(model, s1, s3, hyps (4, 16): R, t, N, d of each hypothesis, F (2, 9), Hn).
    An invalid entry gives zeros.  trace, a dict, receives w, hi, mid, lo and b."""
    out = dict(model=INVALID, s1=ft(0), s3=ft(0), hyps=np.zeros((4, 16), ft), F=np.zeros((2, 9), ft), Hn=None)
    A = normalise(H, K8, ft)
    if A is None:
        return out
    B, V = A.copy(), np.eye(3, dtype=ft)
    one, two = ft(1), ft(2)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                alpha = _dot(B[:, p], B[:, p])
                beta = _dot(B[:, q], B[:, q])
                gamma = _dot(B[:, p], B[:, q])
                if gamma == 0:
                    continue
                zeta = (beta - alpha) / (two * gamma)
                tau = one / (np.abs(zeta) + np.sqrt(one + zeta * zeta))
                if zeta < 0:
                    tau = -tau
                c = one / np.sqrt(one + tau * tau)
                s = c * tau
                for M in (B, V):
                    mp, mq = M[:, p].copy(), M[:, q].copy()
                    M[:, p] = c * mp - s * mq
                    M[:, q] = s * mp + c * mq
        w = [_dot(B[:, j], B[:, j]) for j in range(3)]
        hi = 0
        for j in (1, 2):
            if w[j] > w[hi]:
                hi = j
        ja, jb = [j for j in range(3) if j != hi]
        mid, lo = (jb, ja) if w[jb] > w[ja] else (ja, jb)
        if trace is not None:
            trace.update(w=w, hi=hi, mid=mid, lo=lo)
        if not w[lo] > 0:
            return out
        s1, s3 = w[hi] / w[mid], w[lo] / w[mid]
        b = np.sqrt(s1) - np.sqrt(s3)
        if trace is not None:
            trace.update(b=b)
        out.update(s1=s1, s3=s3)
        if not b > ft(f32(min_baseline)):
            u = [B[:, j] / np.sqrt(w[j]) for j in range(3)]
            R = np.zeros((3, 3), ft)
            for r in range(3):
                for c in range(3):
                    R[r, c] = (u[0][r] * V[c, 0] + u[1][r] * V[c, 1]) + u[2][r] * V[c, 2]
            out["hyps"][:, :9] = R.reshape(9)
            out["model"] = ROTATION
            return out
        Hn = (A / np.sqrt(w[mid])).astype(ft)
        v1, v2, v3 = V[:, hi], V[:, mid], V[:, lo]
        a, c, dd = np.sqrt(one - s3), np.sqrt(s1 - one), np.sqrt(s1 - s3)
        ua = [(a * v1[r] + c * v3[r]) / dd for r in range(3)]
        ub = [(a * v1[r] - c * v3[r]) / dd for r in range(3)]
        sa, sb = _solution(Hn, v2, ua, ft), _solution(Hn, v2, ub, ft)
        if sa is None or sb is None:
            out.update(s1=ft(0), s3=ft(0))
            return out
        for k, (R, t, N, d) in enumerate((sa, sa, sb, sb)):
            sign = -one if k & 1 else one
            out["hyps"][k] = np.concatenate([R.reshape(9), sign * t, sign * N, [d]])
        out["F"][0] = fundamental_of(sa[0], sa[1], K8, ft)
        out["F"][1] = fundamental_of(sb[0], sb[1], K8, ft)
        out.update(model=PLANE, Hn=Hn)
    return out


def depth_terms(pose12, K8, xy, ft=f32):
    """pose_cases.depth_terms, in float64 for the twin."""
    if ft is f32:
        return PC.depth_terms(np.asarray(pose12, f32), K8, xy)
    xy = np.ascontiguousarray(np.asarray(xy, f32).reshape(-1, 4), ft)
    fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2 = _k8(K8, ft)
    R, t = np.asarray(pose12[:9], ft).reshape(3, 3), [ft(v) for v in pose12[9:12]]
    one = np.ones(len(xy), ft)
    with np.errstate(all="ignore"):
        p1 = ((xy[:, 0] - cx1) / fx1, (xy[:, 1] - cy1) / fy1, one)
        p2 = ((xy[:, 2] - cx2) / fx2, (xy[:, 3] - cy2) / fy2, one)
        a = [R[r, 0] * p1[0] + R[r, 1] * p1[1] + R[r, 2] * p1[2] for r in range(3)]
        n = _cross(a, p2)
        p2t, at = _cross(p2, t), _cross(a, t)
        return _dot(n, n), _dot(p2t, n), _dot(at, n), p1[0], p1[1]


def record_votes(dec, K8, xy, thresh_f, ft=f32):
    """Step 7 without the gate: (n, 4) bool, whether each row of xy counts for each hypothesis."""
    xyt = np.ascontiguousarray(np.asarray(xy, f32).reshape(-1, 4), ft)
    out = np.zeros((len(xyt), 4), bool)
    for k in range(4):
        F = [ft(v) for v in dec["F"][k // 2]]
        inl = _f_inliers(F, xyt[:, 0], xyt[:, 1], xyt[:, 2], xyt[:, 3], ft(f32(thresh_f)))
        den, n1, n2, _, _ = depth_terms(dec["hyps"][k, :12], K8, xy, ft)
        out[:, k] = inl & PC.in_front(den, n1, n2)
    return out


def pick(votes):
    """(the largest vote at the smallest k, the better-voted hypothesis of the other rotation)."""
    best = int(np.argmax(votes))
    alt = (3 if votes[3] > votes[2] else 2) if best < 2 else (1 if votes[1] > votes[0] else 0)
    return best, alt


def expected_planar(recs, n, H, F, K8, min_score=GATES[0], max_ambiguity=GATES[1], thresh_h=THRESH_H, thresh_f=THRESH_F,
                    planar_ratio=RATIO, min_inliers=MIN_INLIERS, min_baseline=MIN_BASELINE, ft=f32):
    """One entry: dict(model, hf (2,) int32, and for model 1 and 2: pose (12,), num_front, votes (4,) int32, xyz
    (max(n, 0), 4) float32, pose_alt (12,), plane (4,), best, alt, dec).  F may be None."""
    xy = PC.coordinates(recs, n)
    g = gate(recs[:len(xy)], min_score, max_ambiguity)
    nH = int((g & h_inliers(H, xy, thresh_h, ft)).sum())
    nF = int((g & f_inliers(F, xy, thresh_f, ft)).sum()) if F is not None else 0
    out = dict(model=GENERAL, hf=np.array([nH, nF], np.int32))
    if not candidate(nH, nF, F is not None, planar_ratio, min_inliers):
        return out
    dec = decompose(H, K8, min_baseline, ft=ft)
    out.update(model=dec["model"], dec=dec)
    if dec["model"] == INVALID:
        return out
    hyps = dec["hyps"]
    if dec["model"] == ROTATION:
        pose = np.concatenate([hyps[0, :9], np.zeros(3, ft)])
        out.update(pose=pose, pose_alt=pose.copy(), num_front=0, votes=np.zeros(4, np.int32), plane=np.zeros(4, ft),
                   xyz=np.full((len(xy), 4), PC.ONE_NAN, f32), best=0, alt=0)
        return out
    votes = (record_votes(dec, K8, xy, thresh_f, ft) & g[:, None]).sum(0).astype(np.int32)
    best, alt = pick(votes)
    den, n1, n2, p1x, p1y = depth_terms(hyps[best, :12], K8, xy, ft)
    xyz = PC.xyz_rows(True, den, n1, n2, p1x, p1y) if ft is f32 else None
    out.update(pose=hyps[best, :12].copy(), pose_alt=hyps[alt, :12].copy(), num_front=int(votes[best]), votes=votes,
               plane=hyps[best, 12:].copy(), xyz=xyz, best=best, alt=alt)
    return out


# ---- planted scenes (float64)

def fit_homography(xy):
    """The normalised least-squares (DLT) homography of all rows of xy in float64, set-1 to set-2 pixels, h8 = 1."""
    def norm(x, y):
        cx, cy = x.mean(), y.mean()
        s = np.sqrt(2.0) / np.hypot(x - cx, y - cy).mean()
        return (x - cx) * s, (y - cy) * s, np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1]])
    xy = np.asarray(xy, f64)
    u1, v1, T1 = norm(xy[:, 0], xy[:, 1])
    u2, v2, T2 = norm(xy[:, 2], xy[:, 3])
    z, o = np.zeros_like(u1), np.ones_like(u1)
    rows = np.concatenate([np.stack([-u1, -v1, -o, z, z, z, u2 * u1, u2 * v1, u2], 1),
                           np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], 1)])
    H = np.linalg.inv(T2) @ np.linalg.svd(rows)[2][-1].reshape(3, 3) @ T1
    return H / H[2, 2]


def planar_scene(seed, n=400, baseline=0.5, off=0.0, noise=0.5, angle=0.15, k2=PC.K_B, depth=5.0, second_plane=0.0,
                 general=False):
    """Two views of n points on one plane at `depth` in front of camera 1, tilted up to 0.4 rad, |t| = baseline * depth:
    dict(recs, xy, H (9,) float32 from a least-squares fit of the on-plane matches, K8, R, t (unit), N, d (in units of
    |t|), on (which points are on the plane)).  `off` of the points lie 0.1 to 0.3 of the depth off the plane;
    `second_plane` of them on a second plane, tilted the other way; `general`: a cloud 0.6 of the depth thick.  baseline
    0: a rotation only (t is zeros)."""
    rng = np.random.default_rng(5000 + seed)
    K1, K2 = PC.kmat(PC.K_A), PC.kmat(k2)
    tilt = PC.rodrigues(rng.normal(0, 1, 3) * [1, 1, 0] + [1e-9, 0, 0], rng.uniform(0.1, 0.4))
    N = tilt @ np.array([0, 0, 1.0])
    d0 = depth * N[2]                                            # the plane passes through (0, 0, depth)
    px = np.stack([rng.uniform(300, 1620, n), rng.uniform(150, 930, n), np.ones(n)], 1)
    rays = (np.linalg.inv(K1) @ px.T).T
    X = rays * (d0 / (rays @ N))[:, None]
    on = np.ones(n, bool)
    if off:
        on[rng.choice(n, int(n * off), replace=False)] = False
        shift = rng.uniform(0.1, 0.3, n) * depth * rng.choice([-1, 1], n)
        X[~on] = X[~on] + shift[~on, None] * rays[~on] / np.linalg.norm(rays[~on], axis=1)[:, None]
    if second_plane:
        on[rng.choice(n, int(n * second_plane), replace=False)] = False
        N2 = PC.rodrigues([0, 1, 0], 0.6) @ np.array([0, 0, 1.0])
        X[~on] = rays[~on] * ((depth * 1.3 * N2[2]) / (rays[~on] @ N2))[:, None]
    if general:
        on[:] = False
        X = rays * rng.uniform(0.7, 1.3, n)[:, None] * depth
    R = PC.rodrigues(rng.normal(0, 1, 3), angle)
    t = rng.normal(0, 1, 3) * [1, 1, 0.3]
    t = t / np.linalg.norm(t) * baseline * depth
    X2 = (R @ X.T).T + t
    p1, p2 = (K1 @ X.T).T, (K2 @ X2.T).T
    xy = np.concatenate([p1[:, :2] / p1[:, 2:], p2[:, :2] / p2[:, 2:]], 1) + rng.normal(0, noise, (n, 4))
    H = fit_homography(xy[on] if on.any() else xy).astype(f32).reshape(9)
    nt = np.linalg.norm(t)
    return dict(recs=PC.records(xy, 900 + seed), xy=xy, H=H, K8=np.array(PC.K_A + tuple(k2), f32), R=R,
                t=t / nt if nt else t, N=N, d=d0 / nt if nt else 0.0, on=on)


SETTINGS = ((0.5, 0.0), (0.5, 0.1), (0.1, 0.0), (0.1, 0.1))      # baseline over depth, share of points off the plane
SCENES_EACH = 12
_SCENES = {}


def scene(baseline, off, i):
    key = (baseline, off, i)
    if key not in _SCENES:
        _SCENES[key] = planar_scene(seed=100 * SETTINGS.index((baseline, off)) + i, baseline=baseline, off=off)
    return _SCENES[key]


def pose_distance(pose, R, t):
    """|| R Rgt^T - I ||_F + || t - tgt ||: the combined distance of a pose (12,) to (R, t)."""
    p = np.asarray(pose, f64)
    return float(np.linalg.norm(p[:9].reshape(3, 3) @ np.asarray(R, f64).reshape(3, 3).T - np.eye(3)) +
                 np.linalg.norm(p[9:12] - np.asarray(t, f64)))


# ---- hostile inputs

def hostile_matrices():
    """(name, H (9,), K8, min_baseline, the model decompose() must give)."""
    s = scene(0.5, 0.0, 0)
    K8, H = s["K8"], s["H"]
    U8 = PC.K_UNIT8
    nan, inf = H.copy(), H.copy()
    nan[4], inf[2] = np.nan, np.inf
    rot = PC.rodrigues([0.2, -0.5, 0.7], 0.3).astype(f32).reshape(9)
    rank1 = np.array([0, 0, 3, 0, 0, 2, 0, 0, 1], f32)
    rank2 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0], f32)
    mirror = np.array([-1, 0, 0, 0, 1, 0, 0, 0, 1], f32)
    tie = np.array([1, 0, 0, 0, 1, 0, 0, 0, 2], f32)             # w = (1/4, 1/4, 1): hi = 2, a tie of the other two
    tie2 = np.array([2, 0, 0, 0, 2, 0, 0, 0, 1], f32)            # w = (1, 1, 1/4): a tie for hi
    shear = np.array([1, 0, 0.5, 0, 1, 0, 0, 0, 1], f32)         # R = I, t along x, N along z, exactly representable
    return [("planted", H, K8, MIN_BASELINE, PLANE), ("zeros", np.zeros(9, f32), K8, MIN_BASELINE, INVALID),
            ("a NaN", nan, K8, MIN_BASELINE, INVALID), ("an inf", inf, K8, MIN_BASELINE, INVALID),
            ("A overflows", np.full(9, 3e38, f32), K8, MIN_BASELINE, INVALID),
            ("scaled by 1e-20", (H * f32(1e-20)).astype(f32), K8, MIN_BASELINE, PLANE),
            ("scaled by 1e20", (H * f32(1e20)).astype(f32), K8, MIN_BASELINE, PLANE),
            ("negated", (-H).astype(f32), K8, MIN_BASELINE, PLANE),
            ("det < 0", mirror, U8, MIN_BASELINE, ROTATION), ("det = 0", rank2, U8, MIN_BASELINE, INVALID),
            ("rank 1", rank1, U8, MIN_BASELINE, INVALID), ("identity", np.eye(3, dtype=f32).reshape(9), U8, 0.0, ROTATION),
            ("a rotation", rot, U8, MIN_BASELINE, ROTATION), ("a rotation, min_baseline 0", rot, U8, 0.0, None),
            ("a tie of w for mid", tie, U8, MIN_BASELINE, PLANE), ("a tie of w for hi", tie2, U8, MIN_BASELINE, PLANE),
            ("a shear", shear, U8, MIN_BASELINE, PLANE)] + extreme_intrinsics(H, shear) + random_matrices()


def extreme_intrinsics(H, shear):
    """Intrinsics that misift_recover_pose_planar_batch accepts (focal lengths finite and > 0, principal points finite)
    but no camera has: tiny and huge focal lengths and principal points, which feed the divisions of step 3 and of F_k.
    The model is whatever the definition gives."""
    out = []
    for name, k8 in (("tiny focal lengths", (1e-30, 1e-30, 0, 0, 1e-30, 1e-30, 0, 0)),
                     ("huge focal lengths", (1e30, 1e30, 0, 0, 1e30, 1e30, 0, 0)),
                     ("tiny over huge focal lengths", (1e-30, 1e30, 3, -2, 1e30, 1e-30, -5, 7)),
                     ("the smallest and the largest focal length", (1e-45, 3e38, 0, 0, 3e38, 1e-45, 0, 0)),
                     ("huge principal points", (1500, 1500, 1e20, -1e20, 1200, 1250, -1e20, 1e20)),
                     ("principal points at the largest float", (1, 1, 3e38, 3e38, 1, 1, -3e38, 3e38)),
                     ("fx 1e-30, cx 1e20", (1e-30, 1, 1e20, 0, 1, 1e30, 0, -1e20))):
        for hname, h in (("planted", H), ("a shear", shear)):
            out.append(("%s, %s H" % (name, hname), h, np.array(k8, f32), MIN_BASELINE, None))
    # the same extremes with an H that belongs to them, H = K2 (R + t N^T / d) K1^-1 of a planted scene: these decompose
    sc = scene(0.5, 0.0, 0)
    A0 = sc["R"] + np.outer(sc["t"], sc["N"]) / sc["d"]
    for name, k8 in (("focal lengths 1e-10", (1e-10, 2e-10, 3e-11, -1e-10, 1e-10, 1e-10, 0, 2e-10)),
                     ("focal lengths 1e10", (1e10, 1e10, 4e9, 6e9, 2e10, 1e10, -3e9, 1e9)),
                     ("focal lengths 1e-8 and 1e8", (1e-8, 1e-8, 1e-8, 0, 1e8, 1e8, 0, 5e7)),
                     ("principal points 1e4 focal lengths away", (1, 1, 1e4, -1e4, 1, 1, -1e4, 1e4))):
        k8 = np.array(k8, f32)
        Hm = PC.kmat(k8[4:].astype(f64)) @ A0 @ np.linalg.inv(PC.kmat(k8[:4].astype(f64)))
        out.append(("%s, its own H" % name, Hm.astype(f32).reshape(9), k8, MIN_BASELINE, None))
    return out


def random_matrices(count=24):
    """Random H: entries uniform in [-1, 1] under the unit K, the same scaled into pixels under the scene's K, and near a
    rotation; tiny and huge overall scales among them."""
    rng = np.random.default_rng(61)
    K8s = (PC.K_UNIT8, np.array(PC.K_A + PC.K_B, f32))
    out = []
    for i in range(count):
        M = rng.uniform(-1, 1, (3, 3))
        if i % 3 == 2:
            M = PC.rodrigues(rng.normal(0, 1, 3), rng.uniform(0, 1)) + 0.05 * M
        K8 = K8s[i % 2]
        if i % 2:
            M = PC.kmat(K8[4:].astype(f64)) @ M @ np.linalg.inv(PC.kmat(K8[:4].astype(f64)))
        M = M * (1e-25, 1.0, 1e25, 1.0)[i % 4]
        out.append(("random %d" % i, M.astype(f32).reshape(9), K8, (0.0, MIN_BASELINE)[i % 2], None))
    return out


def baseline_edges():
    """(name, H, K8, min_baseline, model) with b == min_baseline exactly and one ulp either side."""
    s = scene(0.1, 0.0, 1)
    tr = {}
    decompose(s["H"], s["K8"], 0.0, trace=tr)
    b = f32(tr["b"])
    assert b > 0
    return [("b one ulp above min_baseline", s["H"], s["K8"], np.nextafter(b, f32(0)), PLANE),
            ("b == min_baseline", s["H"], s["K8"], b, ROTATION),
            ("b one ulp below min_baseline", s["H"], s["K8"], np.nextafter(b, f32(1)), ROTATION)]


def hostile_frame():
    """The records the counts, the vote and the triangulation must survive, over the planted scene (0.5, 0.1, 2):
    non-finite and huge positions, and a record with deno = 0.  (recs, H, K8)."""
    from fundamental_cases import HOSTILE
    s = scene(0.5, 0.1, 2)
    recs = s["recs"][:200].copy()
    rng = np.random.default_rng(17)
    rows = rng.choice(len(recs), 40, replace=False)
    for i, r in enumerate(rows):
        recs[PC.POS[i % 4]][r] = HOSTILE[i % len(HOSTILE)]
    return recs, s["H"], s["K8"]


DENO0_H = np.array([1, 0, 0, 0, 1, 0, 1, 0, -4], f32)             # deno = x1 - 4: exactly 0 on the line x1 = 4


def deno0_frame():
    """12 records under DENO0_H: eight fit it exactly (deno 1, 2 and 4), four have deno = 0.  (recs, H, K8)"""
    xy = [[5, 1, 5, 1], [5, -2, 5, -2], [6, 1, 3, 0.5], [6, -3, 3, -1.5], [8, 2, 2, 0.5], [8, -1, 2, -0.25],
          [5, 0.5, 5, 0.5], [6, 0, 3, 0], [4, 1, 7, 7], [4, 0, 0, 0], [4, -2, 1, 1], [4, 3, -1, 2]]
    return PC.records(np.array(xy, f32), 29), DENO0_H, PC.K_UNIT8


def tie_frame():
    """A tie between the two rotations' votes: the shear of hostile_matrices() over records that all lie on its plane
    z = 1 and on one side of the other solution's plane (x1 >= 0), so both rotations get every record.  (recs, H, K8)."""
    rng = np.random.default_rng(23)
    x = rng.integers(-8, 9, (40, 2)).astype(f32) / f32(16)
    x[:, 0] = np.abs(x[:, 0])
    xy = np.concatenate([x, x + np.array([0.5, 0], f32)], 1)
    return PC.records(xy, 23), np.array([1, 0, 0.5, 0, 1, 0, 0, 0, 1], f32), PC.K_UNIT8


RATIO_F = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], f32)             # [t]x of the shear's t = x: the epipolar lines y2 = y1


def ratio_frame():
    """(float)nH == planar_ratio * nF exactly at planar_ratio 0.5: 16 records of tie_frame(), all on their epipolar line
    under RATIO_F, the first 8 under the shear as well, the others a quarter off it along the line.  (recs, H, F, K8)."""
    recs, H, K8 = tie_frame()
    xy = PC.coordinates(recs, 16).copy()
    xy[8:, 2] += f32(0.25)
    return PC.records(xy, 23), H, RATIO_F, K8

"""misift_adjust_bundle_batch: adjust, the numpy restatement of the definition in include/misift.h, the wrapper of the
library's host hook, and the cases of its tests (test_bundle_cpu.py pins the restatement to the hook and to float64 and
to dense linear algebra, test_gpu_bundle.py holds the device to it byte for byte).  A case is a refine case
(refine_cases.refine_case) with the call's further arguments: min_views, cg_iters, lambda0.  The restatement takes its
number format as an argument: with float32 every operation is rounded as the library rounds it, with float64 the same
algorithm is the yardstick.  No GPU in here, and cudasift_amd.capi is imported inside functions only."""
import numpy as np

import pose_cases as PC
import refine_cases as RC
import triangulate_cases as TC
from test_fundamental_cpu import f32

ADJUSTED, FEW_OBS, HELD, NO_CAMERA = 0, 1, 3, 4
POISON_WORD = TC.POISON_WORD
LAMBDA_FLOOR = 1e-7
OUTPUTS = ("cam_out", "points_out", "cam_obs", "cam_status", "cam_rms", "point_obs", "history", "cost", "summary")
INT_OUTPUTS = ("cam_obs", "cam_status", "point_obs", "summary")


# ---- the sums

def track_sum(terms, group, ngroups, dt):
    """Per group, 0 + t0 + t1 + ... in the order given (ascending slot), one term at a time: (ngroups, K)."""
    terms = np.asarray(terms, dt)
    acc = np.zeros((ngroups, terms.shape[1]), dt)
    group = np.asarray(group, np.int64)
    if not len(group):
        return acc
    order = np.argsort(group, kind="stable")
    g = group[order]
    first = np.concatenate([[0], np.nonzero(np.diff(g))[0] + 1])
    rank = np.zeros(len(g), np.int64)
    rank[order] = np.arange(len(g)) - np.repeat(first, np.diff(np.concatenate([first, [len(g)]])))
    for r in range(int(rank.max()) + 1):
        sel = rank == r
        acc[group[sel]] = acc[group[sel]] + terms[sel]
    return acc


def pos_sum(terms, dt):
    """The 256-slot rule on the position in the list: (K,)."""
    return RC.slot_sum(terms, np.arange(len(terms)), dt)


def cross_sum(values, images, dt):
    """The 256-slot rule on the image index over the images that take part."""
    return RC.slot_sum(np.asarray(values, dt).reshape(-1, 1), images, dt)[0]


def dot6(a, b):
    return ((((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) + a[..., 3] * b[..., 3]) +
            a[..., 4] * b[..., 4]) + a[..., 5] * b[..., 5]


# ---- the solves, over arrays: a failed solve gives zeros and ok = False

def solve3(V, g):
    """SOLVE of triangulate for every row of V (n, 6: M00 M01 M02 M11 M12 M22) and g (n, 3): x (n, 3), ok (n,)."""
    m00, m01, m02, m11, m12, m22 = (V[:, j] for j in range(6))
    g0, g1, g2 = g[:, 0], g[:, 1], g[:, 2]
    piv = lambda d: (d > 0) & np.isfinite(d)
    d0 = m00
    ok = piv(d0)
    l10, l20 = m01 / d0, m02 / d0
    d1 = m11 - l10 * m01
    ok = ok & piv(d1)
    e = m12 - l20 * m01
    l21 = e / d1
    d2 = (m22 - l20 * m02) - l21 * e
    ok = ok & piv(d2)
    y0 = g0
    y1 = g1 - l10 * y0
    y2 = (g2 - l20 * y0) - l21 * y1
    x2 = y2 / d2
    x1 = y1 / d1 - l21 * x2
    x0 = (y0 / d0 - l10 * x1) - l20 * x2
    x = np.stack([x0, x1, x2], 1)
    ok = ok & np.isfinite(x).all(1)
    return np.where(ok[:, None], x, 0).astype(V.dtype), ok


def solve6(U, g):
    """SOLVE of refine for every image: U (n, 6, 6) symmetric, g (n, 6): delta (n, 6), ok (n,)."""
    n = len(U)
    dt = U.dtype
    L = np.zeros((n, 6, 6), dt)
    d, v, y, x = [None] * 6, [None] * 6, [None] * 6, [None] * 6
    ok = np.ones(n, bool)
    for j in range(6):
        dj = U[:, j, j]
        for k in range(j):
            v[k] = L[:, j, k] * d[k]
            dj = dj - L[:, j, k] * v[k]
        d[j] = dj
        ok = ok & (dj > 0) & np.isfinite(dj)
        for i in range(j + 1, 6):
            e = U[:, i, j]
            for k in range(j):
                e = e - L[:, i, k] * v[k]
            L[:, i, j] = e / dj
    for i in range(6):
        e = g[:, i]
        for k in range(i):
            e = e - L[:, i, k] * y[k]
        y[i] = e
    for i in range(5, -1, -1):
        e = y[i] / d[i]
        for k in range(i + 1, 6):
            e = e - L[:, k, i] * x[k]
        x[i] = e
    x = np.stack(x, 1) if n else np.zeros((0, 6), dt)
    ok = ok & np.isfinite(x).all(1)
    return np.where(ok[:, None], x, 0).astype(dt), ok


# ---- a member under a state

def linearise(C, K, X, x, y, dt):
    """Step 1 for every member: C (m, 12), K (m, 4), X (m, 3): front (m,), lin (m, 20)."""
    c, k = C.T, K.T
    xc, yc, zc, iz, a, b, ru, rv = RC.view(c, k, X, x, y, dt)
    gx, gy = k[0] * iz, k[1] * iz
    one, zero = dt(1), dt(0)
    cols = [gx * -(a * yc), gx * (zc + a * xc), gx * -yc, gx * one, gx * zero, gx * -a,
            gy * -(zc + b * yc), gy * (b * xc), gy * xc, gy * zero, gy * one, gy * -b,
            gx * (c[0] - a * c[6]), gx * (c[1] - a * c[7]), gx * (c[2] - a * c[8]),
            gy * (c[3] - b * c[6]), gy * (c[4] - b * c[7]), gy * (c[5] - b * c[8]), ru, rv]
    return zc > 0, np.stack(cols, 1).astype(dt) if len(x) else np.zeros((0, 20), dt)


def w(l, r, q):
    return l[:, r] * l[:, 12 + q] + l[:, 6 + r] * l[:, 15 + q]


def w3(l, v):
    """(W v) for a 3-vector per member: (m, 6)."""
    return np.stack([(w(l, r, 0) * v[:, 0] + w(l, r, 1) * v[:, 1]) + w(l, r, 2) * v[:, 2] for r in range(6)], 1)


def wt6(l, v):
    """(W^T v) for a 6-vector per member: (m, 3)."""
    return np.stack([((((w(l, 0, q) * v[:, 0] + w(l, 1, q) * v[:, 1]) + w(l, 2, q) * v[:, 2]) + w(l, 3, q) * v[:, 3]) +
                      w(l, 4, q) * v[:, 4]) + w(l, 5, q) * v[:, 5] for q in range(3)], 1)


class Problem:
    """The sets of the call, decided once: members in ascending slot with their image and track, the images' states."""

    def __init__(self, case, dt):
        self.case, self.dt = case, dt
        n = self.n = case["nimages"]
        T, O = RC.counts(case)
        self.T, self.O = T, O
        key, owner = RC.candidate_keys(case)
        cam_in = np.ascontiguousarray(case["cam"], f32).reshape(-1, 12)
        pair = np.asarray(case["cam_pair"], np.int32)
        hold = set(int(h) for h in case["hold"])
        state = np.zeros(n, np.int64)
        cams = cam_in.astype(dt)
        with np.errstate(all="ignore"):
            for i in range(n):
                if pair[i] == RC.UNSET or not np.isfinite(cam_in[i]).all():
                    state[i] = NO_CAMERA
                elif pair[i] == RC.ROOT or i in hold:
                    state[i] = HELD
                elif case["orthonormalise"]:
                    c = RC.orthonormalise(cams[i], dt)
                    if np.isfinite(c).all():
                        cams[i] = c
                    else:
                        state[i] = NO_CAMERA
            self.K = np.asarray(case["intrinsics"], f32).reshape(-1, 4).astype(dt)
            pts = np.asarray(case["points"], f32).reshape(-1, 4)
            obs = case["obs"][:O]
            me = f32(case["max_error"])
            thresh2 = me * me if dt is f32 else dt(me) * dt(me)
            cand = np.nonzero(key >= 0)[0]
            cand = cand[state[key[cand]] != NO_CAMERA]
            ck, ct = key[cand], owner[cand]
            X = pts[ct, :3].astype(dt)
            x, y = obs["xpos"][cand].astype(dt), obs["ypos"][cand].astype(dt)
            _, _, zc, _, _, _, ru, rv = RC.view(cams[ck].T, self.K[ck].T, X, x, y, dt)
            pre = zc > 0
            if not np.isinf(thresh2):
                pre = pre & (ru * ru + rv * rv < thresh2)
        cand, ck, ct = cand[pre], ck[pre], ct[pre]
        self.tcount = np.bincount(ct, minlength=max(T, 1))            # one entry at the least; owners lie below T
        self.active = self.tcount >= case["min_views"]
        keep = self.active[ct] if len(ct) else np.zeros(0, bool)
        self.slot, self.img, self.trk = cand[keep], ck[keep], ct[keep]
        self.x, self.y = obs["xpos"][self.slot].astype(dt), obs["ypos"][self.slot].astype(dt)
        self.icount = np.bincount(self.img, minlength=n)
        state[(state == ADJUSTED) & (self.icount < case["min_obs"])] = FEW_OBS
        self.state = state
        self.free = np.nonzero(state == ADJUSTED)[0]
        self.of_image = [np.nonzero(self.img == i)[0] for i in range(n)]
        self.in_free = state[self.img] == ADJUSTED
        self.cams0 = cams
        self.pts0 = pts[:max(T, 1), :3].astype(dt)
        self.cam_in, self.pts_in = cam_in, pts

    def costs(self, cams, pts):
        """(in front, the squared residual per member, c_i per image, c) of a state."""
        dt = self.dt
        _, _, zc, _, _, _, ru, rv = RC.view(cams[self.img].T, self.K[self.img].T, pts[self.trk], self.x, self.y, dt)
        e = ru * ru + rv * rv
        ci = np.array([pos_sum(e[m].reshape(-1, 1), dt)[0] for m in self.of_image], dt)
        return bool((zc > 0).all()), e, ci, cross_sum(ci, np.arange(self.n), dt)


def lm_step(P, cams, pts, lam, cg_iters, dt):
    """Steps 1-5 at damping lam: dict(fail, cams, pts (the trial state), iters, x, delta)."""
    n, T = P.n, len(P.pts0)
    lam1 = dt(1) + lam
    front, l = linearise(cams[P.img], P.K[P.img], pts[P.trk], P.x, P.y, dt)
    assert front.all()
    rows = np.empty((2 * len(l), 9), dt)
    for h, (a, r) in enumerate(((12, 18), (15, 19))):
        a0, a1, a2, rhs = l[:, a], l[:, a + 1], l[:, a + 2], l[:, r]
        rows[h::2] = np.stack([a0 * a0, a0 * a1, a0 * a2, a1 * a1, a1 * a2, a2 * a2, a0 * rhs, a1 * rhs, a2 * rhs], 1)
    N = track_sum(rows, np.repeat(P.trk, 2), T, dt)
    V, gp = N[:, :6].copy(), N[:, 6:]
    for j in (0, 3, 5):
        V[:, j] = V[:, j] * lam1
    act = np.nonzero(P.active)[0]
    yt = np.zeros((T, 3), dt)
    yt[act], ok = solve3(V[act], gp[act])
    fail = not ok.all()
    nf = len(P.free)
    U = np.zeros((nf, 6, 6), dt)
    b = np.zeros((nf, 6), dt)
    for f, i in enumerate(P.free):
        m = P.of_image[i]
        lm = l[m]
        cols = [lm[:, r] * lm[:, c] + lm[:, 6 + r] * lm[:, 6 + c] for r in range(6) for c in range(r, 6)]
        cols += [lm[:, r] * lm[:, 18] + lm[:, 6 + r] * lm[:, 19] for r in range(6)]
        s = pos_sum(np.concatenate([np.stack(cols, 1), w3(lm, yt[P.trk[m]])], 1), dt)
        j = 0
        for r in range(6):
            for c in range(r, 6):
                U[f, r, c] = U[f, c, r] = s[j] * lam1 if r == c else s[j]
                j += 1
        b[f] = s[21:27] - s[27:33]
    _, ok = solve6(U, b)
    fail = fail or not ok.all()
    out = dict(fail=fail, iters=0, x=np.zeros((nf, 6), dt), cams=cams, pts=pts)
    if fail:
        return out
    fpos = np.full(n, -1, np.int64)
    fpos[P.free] = np.arange(nf)
    mf = np.nonzero(P.in_free)[0]                                # the members in free images, ascending slot
    x = np.zeros((nf, 6), dt)
    r = b.copy()
    z, _ = solve6(U, r)
    p = z.copy()
    rho = cross_sum(dot6(r, z), P.free, dt)
    alive = bool(np.isfinite(rho))
    iters = 0
    for _ in range(cg_iters):
        if not alive:
            break
        st = track_sum(wt6(l[mf], p[fpos[P.img[mf]]]), P.trk[mf], T, dt)
        q = np.zeros((T, 3), dt)
        q[act], _ = solve3(V[act], st[act])
        yv = np.zeros((nf, 6), dt)
        for f, i in enumerate(P.free):
            m = P.of_image[i]
            s = pos_sum(w3(l[m], q[P.trk[m]]), dt)
            yv[f] = np.array([dot6(U[f, rr], p[f]) for rr in range(6)], dt) - s
        sigma = cross_sum(dot6(p, yv), P.free, dt)
        if not (np.isfinite(sigma) and sigma > 0):
            break
        alpha = rho / sigma
        x = x + alpha * p
        r = r - alpha * yv
        z, _ = solve6(U, r)
        rho2 = cross_sum(dot6(r, z), P.free, dt)
        iters += 1
        if not np.isfinite(rho2):
            break
        beta = rho2 / rho
        p = z + beta * p
        rho = rho2
    st = track_sum(wt6(l[mf], x[fpos[P.img[mf]]]), P.trk[mf], T, dt)
    delta = np.zeros((T, 3), dt)
    delta[act], _ = solve3(V[act], gp[act] - st[act])
    pts2 = pts.copy()
    pts2[act] = pts[act] + delta[act]
    cams2 = cams.copy()
    for f, i in enumerate(P.free):
        cams2[i] = RC.update(cams[i], x[f], dt)
    return dict(fail=False, iters=iters, x=x, delta=delta, cams=cams2, pts=pts2, U=U, b=b, V=V, gp=gp, lin=l)


def adjust(case, dt=f32):
    """The call restated: dict(problem, cams, pts (the final state), cost (2), history [(c', lambda, kept, iters)],
    ci0, ci1 (per-image costs), e (squared residual per member under the final state), kept, trace: what became of each
    step, 'kept', 'worse', 'behind', 'not finite' or 'singular')."""
    P = Problem(case, dt)
    nan = PC.ONE_NAN if dt is f32 else dt(np.nan)
    with np.errstate(all="ignore"):
        cams, pts = P.cams0.copy(), P.pts0.copy()
        _, e, ci, c = P.costs(cams, pts)
        ci0, c0 = ci, c
        lam = dt(f32(case["lambda0"]))
        floor = dt(f32(LAMBDA_FLOOR))
        history, trace, kept_steps = [], [], 0
        for _ in range(case["num_loops"]):
            s = lm_step(P, cams, pts, lam, case["cg_iters"], dt)
            kept, c2, why = False, nan, "singular"
            if not s["fail"]:
                free = P.free
                act = np.nonzero(P.active)[0]
                finite = np.isfinite(s["cams"][free]).all() and np.isfinite(s["pts"][act]).all()
                front, e2, ci2, cc = P.costs(s["cams"], s["pts"])
                why = "not finite" if not finite else "behind"
                if finite and front:
                    c2 = nan if np.isnan(cc) else cc
                    kept = bool(cc < c)
                    why = "kept" if kept else "worse"
            trace.append(why)
            history.append((c2, lam, int(kept), s["iters"]))
            if kept:
                cams, pts, e, ci, c = s["cams"], s["pts"], e2, ci2, cc
                kept_steps += 1
                lo = lam / dt(10)
                lam = lo if lo > floor else floor
            else:
                lam = lam * dt(10)
    return dict(problem=P, cams=cams, pts=pts, cost=(c0, c), history=history, ci0=ci0, ci1=ci, e=e, kept=kept_steps,
                trace=trace)


def pooled_rms(res):
    """The rms over all members under the final state, in float64."""
    return float(np.sqrt(np.asarray(res["e"], np.float64).sum() / max(len(res["e"]), 1)))


def expected_bundle(case):
    """The nine outputs of the call as uint32 arrays of exactly the stated sizes (poison where the call writes nothing),
    and the restatement's own dict under 'res'."""
    res = adjust(case, f32)
    P = res["problem"]
    n, mt, T = P.n, case["max_tracks"], P.T
    cam_out = P.cam_in.view(np.uint32).copy()
    own = np.isin(P.state, (ADJUSTED, FEW_OBS))
    cam_out[own] = res["cams"][own].astype(f32).view(np.uint32)
    with np.errstate(all="ignore"):
        rms = np.full((n, 2), PC.ONE_NAN, f32)
        has = P.icount > 0
        cnt = P.icount[has].astype(f32)
        rms[has, 0] = np.sqrt(res["ci0"][has] / cnt)
        rms[has, 1] = np.sqrt(res["ci1"][has] / cnt)
        rms = np.where(np.isnan(rms), PC.ONE_NAN, rms).astype(f32)
        points_out = np.full((mt, 4), POISON_WORD, np.uint32)
        points_out[:T] = np.ascontiguousarray(P.pts_in[:T]).view(np.uint32)
        act = np.nonzero(P.active)[0]
        ct = track_sum(np.asarray(res["e"], f32).reshape(-1, 1), P.trk, max(T, 1), f32)[:, 0]
        trms = np.sqrt(ct[act] / P.tcount[act].astype(f32))
        trms = np.where(np.isnan(trms), PC.ONE_NAN, trms).astype(f32)
        points_out[act, :3] = res["pts"][act].astype(f32).view(np.uint32)
        points_out[act, 3] = trms.view(np.uint32)
    point_obs = np.full(mt, POISON_WORD, np.uint32)
    point_obs[:T] = P.tcount[:T].astype(np.int32).view(np.uint32)
    L = case["num_loops"]
    history = np.full(max(4 * L, 1), POISON_WORD, np.uint32)
    for k, (c2, lam, kept, iters) in enumerate(res["history"]):
        history[4 * k:4 * k + 2] = np.array([c2, lam], f32).view(np.uint32)
        history[4 * k + 2:4 * k + 4] = [kept, iters]
    cost = np.array(res["cost"], f32)
    cost = np.where(np.isnan(cost), PC.ONE_NAN, cost).astype(f32)
    summary = np.array([T, (P.state == ADJUSTED).sum(), len(P.slot), (P.state == FEW_OBS).sum(), P.active.sum(),
                        (P.state == HELD).sum(), res["kept"], (P.state == NO_CAMERA).sum()], np.int32)
    return dict(cam_out=cam_out.reshape(-1), points_out=points_out.reshape(-1),
                cam_obs=P.icount.astype(np.int32).view(np.uint32), cam_status=P.state.astype(np.int32).view(np.uint32),
                cam_rms=rms.reshape(-1).view(np.uint32), point_obs=point_obs, history=history,
                cost=cost.view(np.uint32), summary=summary.view(np.uint32), res=res)


def sizes(case):
    n, mt = case["nimages"], case["max_tracks"]
    return dict(cam_out=12 * n, points_out=4 * mt, cam_obs=n, cam_status=n, cam_rms=2 * n, point_obs=mt,
                history=max(4 * case["num_loops"], 1), cost=2, summary=8)


# ---- the hook

def hook_bundle(case, in_place=False):
    """misift_test_adjust_bundle on poisoned outputs of exactly the stated sizes, as uint32 arrays."""
    from cudasift_amd import capi
    mt, mo, n = case["max_tracks"], case["max_obs"], case["nimages"]
    offs = np.ascontiguousarray(case["track_offsets"][:mt + 1], np.int32)
    obs = np.ascontiguousarray(case["obs"][:mo])
    summ = np.ascontiguousarray(case["export_summary"], np.int32)
    pts = np.ascontiguousarray(case["points"], f32).reshape(-1, 4).copy()
    st = np.ascontiguousarray(case["point_status"], np.int32)
    cam = np.ascontiguousarray(case["cam"], f32).reshape(-1, 12).copy()
    pair = np.ascontiguousarray(case["cam_pair"], np.int32)
    K = np.ascontiguousarray(case["intrinsics"], f32).reshape(-1, 4)
    hold = np.ascontiguousarray(case["hold"], np.int32).reshape(-1)
    out = {k: np.full(m, POISON_WORD, np.uint32) for k, m in sizes(case).items()}
    if in_place:
        out["cam_out"], out["points_out"] = cam.reshape(-1).view(np.uint32), pts.reshape(-1).view(np.uint32)
    rc = capi.lib().misift_test_adjust_bundle(
        mt, mo, offs.ctypes.data, obs.ctypes.data, summ.ctypes.data, pts.ctypes.data, st.ctypes.data, n, cam.ctypes.data,
        pair.ctypes.data, K.ctypes.data, len(hold), hold.ctypes.data if len(hold) else None, case["min_views"],
        case["min_obs"], case["num_loops"], case["cg_iters"], float(case["max_error"]), float(case["lambda0"]),
        int(case["orthonormalise"]), *[out[k].ctypes.data for k in OUTPUTS])
    assert rc == 0, rc
    return out


def compare(got, e, what):
    for k in OUTPUTS:
        bad = np.nonzero(got[k] != e[k])[0]
        view = np.int32 if k in INT_OUTPUTS else f32
        assert len(bad) == 0, (what, k, "%d words differ, first %s" % (len(bad), bad[:8]), got[k][bad[:4]].view(view),
                               e[k][bad[:4]].view(view))


# ---- cases

def bundle_case(refine, min_views=2, cg_iters=10, lambda0=1e-3, **kw):
    """A case of this call from a refine case; kw overrides its arguments (hold, min_obs, num_loops, ...)."""
    return dict(refine, min_views=min_views, cg_iters=cg_iters, lambda0=lambda0, **kw)


def planted(ntracks, nimages, seed, lengths=(2, 3, 4), noise=0.5, angle=0.02, shift=0.05, point_noise=0.05, hold=(1,),
            **kw):
    """A planted scene (refine_cases.scene) of runs of neighbouring images, the cameras drifted, the points perturbed,
    the root and image 1 (the seed partner) held, image 1 at its planted pose so that the planted state can be reached:
    dict(case, true, X)."""
    sc = RC.scene(RC.runs(ntracks, nimages, seed, lengths), nimages, seed, noise=noise, angle=angle, shift=shift,
                  point_noise=point_noise, hold=tuple(hold))
    cam = np.array(sc["case"]["cam"], f32)
    if nimages > 1:
        cam[1] = sc["true"][1]
    return dict(sc, case=bundle_case(sc["case"], cam=cam, **kw))


def frames_case(frames_of, nimages, seed, **kw):
    """A planted scene from explicit frame lists."""
    scene_kw = {k: kw.pop(k) for k in ("noise", "angle", "shift", "point_noise", "step") if k in kw}
    hold = tuple(kw.pop("hold", ()))
    sc = RC.scene(frames_of, nimages, seed, hold=hold, **scene_kw)
    return bundle_case(sc["case"], **kw)


def member_counts_case(min_obs=6, seed=81, **kw):
    """Tracks of three views, the root, the held image 1 and one of images 2..8, which so get min_obs - 1, min_obs,
    min_obs + 1, 255, 256, 257 and 513 members: either side of one row of the position rule and the wrap into a third."""
    want = [min_obs - 1, min_obs, min_obs + 1, 255, 256, 257, 513]
    frames = [(0, 1, 2 + j) for j, n in enumerate(want) for _ in range(n)]
    order = np.random.default_rng(seed).permutation(len(frames))
    return frames_case([frames[i] for i in order], 9, seed, hold=(1,), noise=0.5, angle=0.01, shift=0.02,
                       point_noise=0.02, step=0.15, min_obs=min_obs, **kw), want


def views_case(seed=82, **kw):
    """Tracks of 2, 3 and 7 views over 8 images and one of 301 (an inconsistent track: it cycles through the images)."""
    frames_of = list(RC.runs(90, 8, seed, lengths=(2, 3, 7)))
    frames_of.insert(40, [i % 8 for i in range(301)])
    return frames_case(frames_of, 8, seed, hold=(1,), noise=0.5, angle=0.01, shift=0.02, point_noise=0.02, **kw)


def hostile_case(**kw):
    """refine_cases.hostile_case (the root, a held and an unset image, a NaN and an inf in a camera, points of every failed
    status, a NaN and an inf in a point, frames outside the images, non-finite positions, points behind a camera)."""
    return bundle_case(RC.hostile_case(), **kw)


def rejected_then_kept_case(**kw):
    """8 cameras far from the optimum: the third step at a damping lowered twice is worse and turned away, the fourth at
    ten times the damping is kept."""
    return planted(120, 8, 6, num_loops=5, **kw)["case"]


def behind_trial_case(**kw):
    """Image 2 is 0.3 rad and 2 units off and the damping next to nothing: the first trial state has a member behind."""
    return frames_case([(0, 1, 2)] * 8, 3, 128, hold=(1,), noise=0.0, angle=0.3, shift=2.0, lambda0=1e-7, num_loops=5,
                       **kw)


# the shapes test_gpu_bundle.py runs on the device and test_bundle_cpu.py through the hook
IMAGE_SHAPES = ((2, 30, 5, 10), (3, 60, 5, 6), (4, 40, 5, 10), (8, 120, 5, 10), (65, 400, 2, 4), (257, 1300, 2, 3))
TRACK_COUNTS = (0, 1, 63, 64, 65, 257)
DEVICE_COUNTS = ((63, 513), (171, 200), (300, 10 ** 9), (2 ** 31 - 1, 2 ** 31 - 1), (-1, 513), (171, -5), (171, 256),
                 (-2 ** 31, -2 ** 31))
# num_loops, cg_iters, lambda0, max_error, orthonormalise
SETTINGS = ((0, 10, 1e-3, RC.INF, 0), (1, 0, 1e-3, RC.INF, 1), (5, 1, 1e-3, 8.0, 0), (5, 6, 1e-7, RC.INF, 1),
            (1, 10, 1e-3, 8.0, 1), (5, 10, 3e38, RC.INF, 0), (0, 0, 1e-3, 8.0, 1))


def image_count_case(nimages, ntracks, loops, cg):
    """Root plus held and no free camera, one free camera, and up to 257 images from tracks of two and three views."""
    return planted(ntracks, nimages, 40 + nimages, lengths=(2, 3) if nimages > 3 else (2, 3, 4), num_loops=loops,
                   cg_iters=cg)["case"]


def track_count_case(ntracks):
    return planted(ntracks, 4, 50 + ntracks, num_loops=3, cg_iters=6)["case"] if ntracks else frames_case([], 3, 83)


def device_counts_case(T, O):
    """171 tracks and 513 slots with T and O as the device would report them."""
    base = bundle_case(RC.spread_case(513), hold=(1,), num_loops=2, cg_iters=4)
    assert (base["max_tracks"], base["max_obs"]) == (171, 513)
    return RC.with_counts(base, T, O)


def settings_cases(num_loops, cg_iters, lambda0, max_error, orth):
    """A planted scene (near enough for an 8 px gate to leave members) and the hostile one under the settings."""
    kw = dict(num_loops=num_loops, cg_iters=cg_iters, lambda0=lambda0, max_error=max_error, orthonormalise=orth)
    return (("planted", planted(40, 4, 1, angle=0.003, shift=0.005, point_noise=0.005, **kw)["case"]),
            ("hostile", hostile_case(**kw)))


def cpu_cases():
    """name -> case: what test_bundle_cpu.py holds the hook to; test_gpu_bundle.py runs these and more on the device."""
    out = {"2 images": planted(30, 2, 4)["case"], "3 images": planted(60, 3, 3, cg_iters=6, orthonormalise=1)["case"],
           "4 images": planted(40, 4, 1)["case"], "rejected then kept": rejected_then_kept_case(),
           "behind": behind_trial_case(), "members": member_counts_case(num_loops=2, cg_iters=3)[0],
           "views": views_case(num_loops=2, cg_iters=4), "min_views 3": views_case(num_loops=2, cg_iters=4, min_views=3),
           "hostile": hostile_case(num_loops=3, cg_iters=5), "hostile gated": hostile_case(max_error=8.0, orthonormalise=1),
           "bad offsets": bundle_case(RC.bad_offsets_case(), hold=(1,)), "no track": frames_case([], 3, 83),
           "no loop": planted(40, 4, 1, num_loops=0, orthonormalise=0)["case"],
           "cg 0": planted(40, 4, 1, cg_iters=0)["case"], "cg 1": planted(40, 4, 1, cg_iters=1)["case"],
           "cg 40": planted(60, 3, 3, cg_iters=40, num_loops=3)["case"],
           "huge lambda": planted(40, 4, 1, lambda0=3e38, num_loops=3)["case"]}
    return out

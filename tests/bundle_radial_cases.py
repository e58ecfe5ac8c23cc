"""misift_adjust_bundle_radial_batch and misift_undistort_obs_batch: the numpy restatement of the definitions in
include/misift.h.  The first is that of misift_adjust_bundle_focal_batch (bundle_focal_cases.py) with one radial
coefficient k_g per camera group among the unknowns, applied to the observation.  The sets, the sums, the solves, the
linearisation, the loss and the groups are bundle_cases', bundle_robust_cases' and bundle_focal_cases' own; lm_step and
adjust are restated here with the radial column, and so are the expected outputs: the twelve shared ones and d_radial.
A case is a case of bundle_focal_cases with `radial` and `k0` (None and None: all zero).  test_bundle_radial_cpu.py pins
the restatement to the library's host hooks, to float64 and to dense linear algebra, test_gpu_bundle_radial.py holds the
device to it byte for byte.  No GPU in here, and cudasift_amd.capi is imported inside functions only."""
import numpy as np

import bundle_cases as BC
import bundle_focal_cases as BFC
import bundle_robust_cases as BRC
import pose_cases as PC
import refine_cases as RC
from bundle_cases import (LAMBDA_FLOOR, NO_CAMERA, POISON_WORD, Problem, cross_sum, dot6, linearise, pos_sum, solve3,
                          solve6, track_sum, w3, wt6)
from bundle_focal_cases import Groups, grouped, wf3
from bundle_robust_cases import NONE, HUBER, GEMAN_MCCLURE, loss_terms, scale_of
from test_fundamental_cpu import f32

MAX_GROUPS = BFC.MAX_GROUPS                                        # MISIFT_MAX_RADIAL_GROUPS
REFINED, NO_MEMBER, NOT_REFINED, HELD = 0, 1, 2, 3                 # MISIFT_RADIAL_*
OUTPUTS = BFC.OUTPUTS + ("radial_out",)                            # in the order of the call's arguments
INT_OUTPUTS = BFC.INT_OUTPUTS
LOSSES = BFC.LOSSES


def radial(case, flags=None, k0=None):
    """A case of this call from a case of bundle_focal_cases: the flag and the start of every group's coefficient.
    flags True: every group's coefficient is an unknown."""
    G = case["ngroups"]
    if flags is True:
        flags = np.ones(G, np.int32)
    if flags is not None and k0 is None:
        k0 = np.zeros(G, f32)
    if k0 is not None and flags is None:
        flags = np.zeros(G, np.int32)
    if flags is not None:
        flags, k0 = np.asarray(flags, np.int32).reshape(-1), np.asarray(k0, f32).reshape(-1)
        assert len(flags) == G and len(k0) == G
    return dict(case, radial=flags, k0=k0)


def flags_of(case):
    """(flags, k0) padded to one entry at the least."""
    G = max(case["ngroups"], 1)
    fl, k0 = np.zeros(G, np.int64), np.zeros(G, f32)
    if case.get("radial") is not None:
        fl[:case["ngroups"]] = case["radial"]
        k0[:case["ngroups"]] = case["k0"]
    return fl, k0


def radial_on(case):
    """The RADIAL instances run: an image has a group and some coefficient is an unknown or starts off zero."""
    fl, k0 = flags_of(case)
    return grouped(case) and bool((fl != 0).any() or (k0 != 0).any())


def model(K, k, x, y):
    """THE RADIAL MODEL on arrays, every operation rounded in the arrays' format: (x', y', dx*rho2, dy*rho2)."""
    dx, dy = x - K[:, 2], y - K[:, 3]
    nx, ny = dx / K[:, 0], dy / K[:, 1]
    rho2 = nx * nx + ny * ny
    e = k * rho2
    return x + dx * e, y + dy * e, dx * rho2, dy * rho2


def undistort(case, obs, kg, dt=f32):
    """misift_undistort_obs_batch restated: a copy of obs[:max_obs] with the slots below O under the coefficients kg."""
    n, G = case["nimages"], case["ngroups"]
    _, O = RC.counts(case)
    out = np.array(obs[:case["max_obs"]])
    if G == 0 or O == 0:
        return out
    K = np.asarray(case["intrinsics"], f32).reshape(-1, 4).astype(dt)
    grp = np.asarray(case["group"], np.int64)
    fr = out["frame"][:O].astype(np.int64)
    ok = (fr >= 0) & (fr < n)
    g = np.where(ok, grp[np.where(ok, fr, 0)], -1)
    sel = np.nonzero(g >= 0)[0]
    with np.errstate(all="ignore"):
        xd, yd, _, _ = model(K[fr[sel]], np.asarray(kg, dt)[g[sel]], out["xpos"][sel].astype(dt), out["ypos"][sel].astype(dt))
    out["xpos"][sel], out["ypos"][sel] = xd.astype(f32), yd.astype(f32)
    return out


class RGroups(Groups):
    """Groups with the flag of every group and member and the radial-live groups."""

    def __init__(self, case, P):
        super().__init__(case, P)
        self.rad, self.k0 = flags_of(case)
        self.mrad = (self.mg >= 0) & (self.rad[np.maximum(self.mg, 0)] != 0)
        self.klive = [g for g in self.live if self.rad[g]]

    def observe(self, P, k):
        """(x', y', Juk, Jvk) per member under the coefficients k: the column is zero where k_g is no unknown."""
        dt = P.dt
        x, y = P.x.copy(), P.y.copy()
        rk = np.zeros((len(x), 2), dt)
        m = np.nonzero(self.mg >= 0)[0]
        xd, yd, qu, qv = model(P.K[P.img[m]], k[self.mg[m]].astype(dt), P.x[m], P.y[m])
        x[m], y[m] = xd, yd
        on = self.mrad[m]
        rk[m[on], 0], rk[m[on], 1] = -qu[on], -qv[on]
        return x, y, rk


def problem(case, dt):
    """The sets under the start state: bundle_cases.Problem on the observations under k0, with the observations as given
    put back (P.x, P.y) for the states to come."""
    _, k0 = flags_of(case)
    T, O = RC.counts(case)
    P = Problem(dict(case, obs=undistort(case, case["obs"], k0, dt)) if radial_on(case) else case, dt)
    obs = case["obs"][:O]
    P.x, P.y = obs["xpos"][P.slot].astype(dt), obs["ypos"][P.slot].astype(dt)
    return P


def costs(P, Gr, cams, pts, s, k, loss, c, c2):
    """(in front (m,), s per member, rho per member, c_i per image, c) of a state."""
    dt = P.dt
    x, y, _ = Gr.observe(P, k)
    _, _, zc, _, _, _, ru, rv = RC.view(cams[P.img].T, Gr.intrinsics(P, s).T, pts[P.trk], x, y, dt)
    sq = ru * ru + rv * rv
    rho = loss_terms(sq, loss, c, c2, dt)[0]
    ci = np.array([pos_sum(rho[m].reshape(-1, 1), dt)[0] for m in P.of_image], dt)
    return zc > 0, sq, rho, ci, cross_sum(ci, np.arange(P.n), dt)


def jacobian(P, Gr, cams, pts, s, k, loss, c, c2):
    """Step 1: (lin (m, 20), f (m, 2), rk (m, 2), and the three before the loss, w)."""
    dt = P.dt
    Kf = Gr.intrinsics(P, s)
    x, y, rk0 = Gr.observe(P, k)
    front, l0 = linearise(cams[P.img], Kf, pts[P.trk], x, y, dt)
    assert front.all()
    _, _, _, _, a, b, _, _ = RC.view(cams[P.img].T, Kf.T, pts[P.trk], x, y, dt)
    Kg = P.K[P.img]
    f0 = np.stack([Kg[:, 0] * a, Kg[:, 1] * b], 1).astype(dt) if len(a) else np.zeros((0, 2), dt)
    wgt = np.ones(len(l0), dt)
    l, f, rk = l0, f0, rk0
    if loss != NONE:
        _, wgt, sw = loss_terms(l0[:, 18] * l0[:, 18] + l0[:, 19] * l0[:, 19], loss, c, c2, dt)
        l = (sw[:, None] * l0).astype(dt)
        f = (sw[:, None] * f0).astype(dt)
        rk = (sw[:, None] * rk0).astype(dt)
    return l, f, rk, l0, f0, rk0, wgt


def wcol(f, l):
    """wf or wk of every member: (m, 3)."""
    return np.stack([f[:, 0] * l[:, 12 + q] + f[:, 1] * l[:, 15 + q] for q in range(3)], 1) if len(l) else np.zeros((0, 3), l.dtype)


def lm_step(P, Gr, cams, pts, s, k, lam, cg_iters, dt, loss=NONE, c=None, c2=None, block=False):
    """Steps 1-5 at damping lam with the focal and the radial columns: dict(fail, cams, pts, s, k (the trial state), ...).
    block: not the call, a variant to measure against: the two scalars of a group preconditioned by their 2 x 2 Schur
    block [[S_gg, S_fk], [S_fk, S_kk]] in place of the two diagonals."""
    n, T, G = P.n, len(P.pts0), Gr.G
    G1 = max(G, 1)
    lam1 = dt(1) + lam
    l, f, rk, l0, f0, rk0, wgt = jacobian(P, Gr, cams, pts, s, k, loss, c, c2)
    mg = Gr.mg
    wf, wk = wcol(f, l), wcol(rk, l)
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
    tfd, tkd, tfk = np.zeros((T, G1), dt), np.zeros((T, G1), dt), np.zeros((T, G1), dt)
    for g in Gr.live:
        sel = mg == g
        wgt_t = track_sum(wf[sel], P.trk[sel], T, dt)
        xs, _ = solve3(V[act], wgt_t[act])
        tfd[act, g] = wf3(wgt_t[act], xs)
        if g in Gr.klive:
            wkt = track_sum(wk[sel], P.trk[sel], T, dt)
            tfk[act, g] = wf3(wkt[act], xs)
    for g in Gr.klive:
        sel = mg == g
        wkt = track_sum(wk[sel], P.trk[sel], T, dt)
        xs, _ = solve3(V[act], wkt[act])
        tkd[act, g] = wf3(wkt[act], xs)
    nf = len(P.free)
    U = np.zeros((nf, 6, 6), dt)
    b = np.zeros((nf, 6), dt)
    ucf, uck = np.zeros((n, 6), dt), np.zeros((n, 6), dt)
    foc, rad4 = np.zeros((n, 3), dt), np.zeros((n, 4), dt)
    for i in range(n):
        g = Gr.grp[i]
        if g < 0 or P.state[i] == NO_CAMERA:
            continue
        m = P.of_image[i]
        fm, lm, km = f[m], l[m], rk[m]
        yy = yt[P.trk[m]]
        cols = [fm[:, 0] * fm[:, 0] + fm[:, 1] * fm[:, 1], fm[:, 0] * lm[:, 18] + fm[:, 1] * lm[:, 19], wf3(wf[m], yy)]
        foc[i] = pos_sum(np.stack(cols, 1), dt)
        if P.state[i] == BC.ADJUSTED:
            ucf[i] = pos_sum(np.stack([lm[:, r] * fm[:, 0] + lm[:, 6 + r] * fm[:, 1] for r in range(6)], 1), dt)
        if not Gr.rad[g]:
            continue
        cols = [km[:, 0] * km[:, 0] + km[:, 1] * km[:, 1], km[:, 0] * lm[:, 18] + km[:, 1] * lm[:, 19], wf3(wk[m], yy),
                fm[:, 0] * km[:, 0] + fm[:, 1] * km[:, 1]]
        rad4[i] = pos_sum(np.stack(cols, 1), dt)
        if P.state[i] == BC.ADJUSTED:
            uck[i] = pos_sum(np.stack([lm[:, r] * km[:, 0] + lm[:, 6 + r] * km[:, 1] for r in range(6)], 1), dt)
    for fi, i in enumerate(P.free):
        m = P.of_image[i]
        lm = l[m]
        cols = [lm[:, r] * lm[:, q] + lm[:, 6 + r] * lm[:, 6 + q] for r in range(6) for q in range(r, 6)]
        cols += [lm[:, r] * lm[:, 18] + lm[:, 6 + r] * lm[:, 19] for r in range(6)]
        sm = pos_sum(np.concatenate([np.stack(cols, 1), w3(lm, yt[P.trk[m]])], 1), dt)
        j = 0
        for r in range(6):
            for q in range(r, 6):
                U[fi, r, q] = U[fi, q, r] = sm[j] * lam1 if r == q else sm[j]
                j += 1
        b[fi] = sm[21:27] - sm[27:33]
    _, ok = solve6(U, b)
    fail = fail or not ok.all()
    out = dict(fail=fail, iters=0, x=np.zeros((nf, 6), dt), xg=np.zeros(G1, dt), xk=np.zeros(G1, dt), cams=cams, pts=pts,
               s=s, k=k, lin=l, f=f, rk=rk, lin0=l0, f0=f0, rk0=rk0, w=wgt, U=U, b=b, V=V, gp=gp, ucf=ucf, uck=uck,
               foc=foc, rad4=rad4, tfd=tfd, tkd=tkd)
    if fail:
        return out
    UL, S, bg = np.zeros(G1, dt), np.ones(G1, dt), np.zeros(G1, dt)
    ULk, Sk, bk, Ufk = np.zeros(G1, dt), np.ones(G1, dt), np.zeros(G1, dt), np.zeros(G1, dt)
    for g in Gr.live:
        u = RC.slot_sum(foc[Gr.images[g]], Gr.images[g], dt)
        Dg = RC.slot_sum(tfd[act, g].reshape(-1, 1), act, dt)[0]
        UL[g] = u[0] * lam1
        S[g] = UL[g] - Dg
        bg[g] = u[1] - u[2]
        if not (np.isfinite(S[g]) and S[g] > 0):
            fail = True
    for g in Gr.klive:
        u = RC.slot_sum(rad4[Gr.images[g]], Gr.images[g], dt)
        Dg = RC.slot_sum(tkd[act, g].reshape(-1, 1), act, dt)[0]
        ULk[g] = u[0] * lam1
        Sk[g] = ULk[g] - Dg
        bk[g] = u[1] - u[2]
        Ufk[g] = u[3]
        if not (np.isfinite(Sk[g]) and Sk[g] > 0):
            fail = True
    out.update(UL=UL, S=S, bg=bg, ULk=ULk, Sk=Sk, bk=bk, Ufk=Ufk)
    if fail:
        return dict(out, fail=True)

    def precondition(rg, rr):
        zg, zk = (rg / S).astype(dt), (rr / Sk).astype(dt)
        for g in Gr.klive if block else ():
            sfk = Ufk[g] - RC.slot_sum(tfk[act, g].reshape(-1, 1), act, dt)[0]
            det = S[g] * Sk[g] - sfk * sfk
            zg[g], zk[g] = (Sk[g] * rg[g] - sfk * rr[g]) / det, (S[g] * rr[g] - sfk * rg[g]) / det
        return zg, zk
    fpos = np.full(n, -1, np.int64)
    fpos[P.free] = np.arange(nf)

    def dot(a, ag, ak, bb, bbg, bbk):
        acc = cross_sum(dot6(a, bb), P.free, dt)
        for g in Gr.live:
            acc = acc + ag[g] * bbg[g]
        for g in Gr.klive:
            acc = acc + ak[g] * bbk[g]
        return acc

    def gather(v, vg, vk):
        """Per track, per member in ascending slot: (W^T v_i) if its image is free, wf * v_g if it has a group, then
        wk * v_k if that group's coefficient is an unknown."""
        terms = np.zeros((len(l), 3, 3), dt)
        valid = np.stack([P.in_free, mg >= 0, Gr.mrad], 1) if len(l) else np.zeros((0, 3), bool)
        mf = np.nonzero(P.in_free)[0]
        terms[mf, 0] = wt6(l[mf], v[fpos[P.img[mf]]])
        mgr = np.nonzero(mg >= 0)[0]
        terms[mgr, 1] = wf[mgr] * vg[mg[mgr]][:, None]
        mk = np.nonzero(Gr.mrad)[0]
        terms[mk, 2] = wk[mk] * vk[mg[mk]][:, None]
        return track_sum(terms.reshape(-1, 3)[valid.reshape(-1)], np.repeat(P.trk, 3)[valid.reshape(-1)], T, dt)

    x, xg, xk = np.zeros((nf, 6), dt), np.zeros(G1, dt), np.zeros(G1, dt)
    r, rg, rr = b.copy(), bg.copy(), bk.copy()
    z, _ = solve6(U, r)
    zg, zk = precondition(rg, rr)
    p, pg, pk = z.copy(), zg.copy(), zk.copy()
    rho = dot(r, rg, rr, z, zg, zk)
    alive = bool(np.isfinite(rho))
    iters = 0
    for _ in range(cg_iters):
        if not alive:
            break
        st = gather(p, pg, pk)
        q = np.zeros((T, 3), dt)
        q[act], _ = solve3(V[act], st[act])
        yv = np.zeros((nf, 6), dt)
        ci, wq, cki, wqk = np.zeros(n, dt), np.zeros(n, dt), np.zeros(n, dt), np.zeros(n, dt)
        for i in range(n):
            if P.state[i] == NO_CAMERA or (Gr.grp[i] < 0 and P.state[i] != BC.ADJUSTED):
                continue
            m, g = P.of_image[i], Gr.grp[i]
            israd = g >= 0 and bool(Gr.rad[g])
            if g >= 0:
                wq[i] = pos_sum(wf3(wf[m], q[P.trk[m]]).reshape(-1, 1), dt)[0]
            if israd:
                wqk[i] = pos_sum(wf3(wk[m], q[P.trk[m]]).reshape(-1, 1), dt)[0]
            if P.state[i] != BC.ADJUSTED:
                continue
            fi = fpos[i]
            sm = pos_sum(w3(l[m], q[P.trk[m]]), dt)
            Up = np.array([dot6(U[fi, j], p[fi]) for j in range(6)], dt)
            if israd:
                yv[fi] = ((Up + ucf[i] * pg[g]) + uck[i] * pk[g]) - sm
                ci[i] = dot6(ucf[i], p[fi])
                cki[i] = dot6(uck[i], p[fi])
            elif g >= 0:
                yv[fi] = (Up + ucf[i] * pg[g]) - sm
                ci[i] = dot6(ucf[i], p[fi])
            else:
                yv[fi] = Up - sm
        yg, yk = np.zeros(G1, dt), np.zeros(G1, dt)
        for g in Gr.live:
            im = Gr.images[g]
            v = RC.slot_sum(np.stack([ci[im], wq[im]], 1), im, dt)
            diag = UL[g] * pg[g]
            if g in Gr.klive:
                w = RC.slot_sum(np.stack([cki[im], wqk[im]], 1), im, dt)
                yk[g] = ((ULk[g] * pk[g] + Ufk[g] * pg[g]) + w[0]) - w[1]
                diag = diag + Ufk[g] * pk[g]
            yg[g] = (diag + v[0]) - v[1]
        sigma = dot(p, pg, pk, yv, yg, yk)
        if not (np.isfinite(sigma) and sigma > 0):
            break
        alpha = rho / sigma
        x = x + alpha * p
        r = r - alpha * yv
        z, _ = solve6(U, r)
        for g in Gr.live:
            xg[g] = xg[g] + alpha * pg[g]
            rg[g] = rg[g] - alpha * yg[g]
            zg[g] = rg[g] / S[g]
        for g in Gr.klive:
            xk[g] = xk[g] + alpha * pk[g]
            rr[g] = rr[g] - alpha * yk[g]
            zk[g] = rr[g] / Sk[g]
        if block:
            zg, zk = precondition(rg, rr)
        rho2 = dot(r, rg, rr, z, zg, zk)
        iters += 1
        if not np.isfinite(rho2):
            break
        beta = rho2 / rho
        p = z + beta * p
        for g in Gr.live:
            pg[g] = zg[g] + beta * pg[g]
        for g in Gr.klive:
            pk[g] = zk[g] + beta * pk[g]
        rho = rho2
    st = gather(x, xg, xk)
    delta = np.zeros((T, 3), dt)
    delta[act], _ = solve3(V[act], gp[act] - st[act])
    pts2 = pts.copy()
    pts2[act] = pts[act] + delta[act]
    cams2 = cams.copy()
    for fi, i in enumerate(P.free):
        cams2[i] = RC.update(cams[i], x[fi], dt)
    s2, k2 = s.copy(), k.copy()
    for g in Gr.live:
        s2[g] = s[g] + xg[g]
    for g in Gr.klive:
        k2[g] = k[g] + xk[g]
    return dict(out, fail=False, iters=iters, x=x, xg=xg, xk=xk, delta=delta, cams=cams2, pts=pts2, s=s2, k=k2)


def adjust(case, dt=f32, steps=None, block=False):
    """The call restated, as bundle_focal_cases.adjust, with coef (the final k_g) and ktrace: the trial coefficients of
    every step that got as far.  steps: a list that takes the lm_step dict of every step."""
    G1 = max(case["ngroups"], 1)
    fl, k0 = flags_of(case)
    if not radial_on(case):
        res = BFC.adjust(case, dt)
        return dict(res, coef=k0.astype(dt), ktrace=[])
    P = problem(case, dt)
    Gr = RGroups(case, P)
    loss = case["loss"]
    c, c2 = scale_of(case, dt) if loss != NONE else (None, None)
    nan = PC.ONE_NAN if dt is f32 else dt(np.nan)
    with np.errstate(all="ignore"):
        cams, pts, s, k = P.cams0.copy(), P.pts0.copy(), np.ones(G1, dt), k0.astype(dt)
        front, sq, e, ci, cost = costs(P, Gr, cams, pts, s, k, loss, c, c2)
        ci0, c0 = ci, cost
        lam = dt(f32(case["lambda0"]))
        floor = dt(f32(LAMBDA_FLOOR))
        history, trace, strace, ktrace, kept_steps = [], [], [], [], 0
        for _ in range(case["num_loops"]):
            st = lm_step(P, Gr, cams, pts, s, k, lam, case["cg_iters"], dt, loss, c, c2, block)
            if steps is not None:
                steps.append(st)
            kept, cc2, why = False, nan, "singular"
            if not st["fail"]:
                act = np.nonzero(P.active)[0]
                strace.append(st["s"].copy())
                ktrace.append(st["k"].copy())
                sl, kl = st["s"][Gr.live], st["k"][Gr.klive]
                finite = (np.isfinite(st["cams"][P.free]).all() and np.isfinite(st["pts"][act]).all() and
                          bool((np.isfinite(sl) & (sl > 0)).all()) and bool(np.isfinite(kl).all()))
                front2, sq2, e2, ci2, cc = costs(P, Gr, st["cams"], st["pts"], st["s"], st["k"], loss, c, c2)
                why = "not finite" if not finite else "behind"
                if finite and front2.all():
                    cc2 = nan if np.isnan(cc) else cc
                    kept = bool(cc < cost)
                    why = "kept" if kept else "worse"
            trace.append(why)
            history.append((cc2, lam, int(kept), st["iters"]))
            if kept:
                cams, pts, s, k, front, sq, e, ci, cost = st["cams"], st["pts"], st["s"], st["k"], front2, sq2, e2, ci2, cc
                kept_steps += 1
                lo = lam / dt(10)
                lam = lo if lo > floor else floor
            else:
                lam = lam * dt(10)
        wgt = loss_terms(sq, loss, c, c2, dt)[1]
    return dict(problem=P, groups=Gr, cams=cams, pts=pts, scale=s, coef=k, cost=(c0, cost), history=history, ci0=ci0,
                ci1=ci, e=e, s=sq, front=front, w=wgt, kept=kept_steps, trace=trace, strace=strace, ktrace=ktrace)


pooled_rms = BRC.pooled_rms


def radial_words(case, res):
    """d_radial: k_g, M_g and the status of every group."""
    G, loops = case["ngroups"], case["num_loops"]
    fl, _ = flags_of(case)
    Gr = res["groups"]
    out = np.full(max(3 * G, 1), POISON_WORD, np.uint32)
    for g in range(G):
        members = int(Gr.count[g]) if grouped(case) else 0
        status = HELD
        if fl[g]:
            status = NOT_REFINED if loops == 0 else (REFINED if radial_on(case) and members > 0 else NO_MEMBER)
        out[3 * g] = np.array([res["coef"][g]], f32).view(np.uint32)[0]
        out[3 * g + 1] = members
        out[3 * g + 2] = status
    return out


def expected_radial(case):
    """The thirteen outputs of the call as uint32 arrays of exactly the stated sizes (poison where the call writes
    nothing), and the restatement's own dict under 'res'.  Where the RADIAL instances do not run the twelve shared ones
    are bundle_focal_cases.expected_focal's own."""
    if not radial_on(case):
        e = BFC.expected_focal(case)
        res = dict(e["res"], coef=flags_of(case)[1])
        return dict(e, res=res, radial_out=radial_words(case, res))
    res = adjust(case, f32)
    e = BFC.shared_outputs(case, res)
    P, Gr = res["problem"], res["groups"]
    G, loops = case["ngroups"], case["num_loops"]
    K = np.ascontiguousarray(case["intrinsics"], f32).reshape(-1, 4)
    kout = K.view(np.uint32).copy()
    foc = np.full(max(3 * G, 1), POISON_WORD, np.uint32)
    for g in range(G):
        status = BFC.NOT_REFINED if loops == 0 else (BFC.REFINED if Gr.count[g] > 0 else BFC.NO_MEMBER)
        foc[3 * g] = np.array([res["scale"][g]], f32).view(np.uint32)[0]
        foc[3 * g + 1] = int(Gr.count[g])
        foc[3 * g + 2] = status
        if status == BFC.REFINED:
            for i in np.nonzero((Gr.grp == g) & (P.state != NO_CAMERA))[0]:
                kout[i, :2] = (K[i, :2] * f32(res["scale"][g])).astype(f32).view(np.uint32)
    return dict(e, res=res, intrinsics_out=kout.reshape(-1), focal=foc, radial_out=radial_words(case, res))


def sizes(case):
    return dict(BFC.sizes(case), radial_out=max(3 * case["ngroups"], 1))


def compare_all(got, e, what, keys=OUTPUTS):
    for k in keys:
        bad = np.nonzero(got[k] != e[k])[0]
        view = np.int32 if k in INT_OUTPUTS else f32
        assert len(bad) == 0, (what, k, "%d words differ, first %s" % (len(bad), bad[:8]), got[k][bad[:4]].view(view),
                               e[k][bad[:4]].view(view))


# ---- the hooks

def host_lists(case):
    """(group, radial, k0) as the contiguous host arrays the calls take; radial and k0 None where the case has none."""
    group = np.ascontiguousarray(case["group"], np.int32).reshape(-1)
    if case.get("radial") is None:
        return group, None, None
    return group, np.ascontiguousarray(case["radial"], np.int32), np.ascontiguousarray(case["k0"], f32)


def hook_bundle_radial(case, in_place=False, weights=True):
    """misift_test_adjust_bundle_radial on poisoned outputs of exactly the stated sizes, as uint32 arrays."""
    from cudasift_amd import capi
    a = BRC.hook_args(case)
    out = {k: np.full(m, POISON_WORD, np.uint32) for k, m in sizes(case).items()}
    if in_place:
        out["cam_out"], out["points_out"] = a["cam"].reshape(-1).view(np.uint32), a["pts"].reshape(-1).view(np.uint32)
    ptr = {k: out[k].ctypes.data for k in OUTPUTS}
    if not weights:
        ptr["obs_weight"] = None
    group, flags, k0 = host_lists(case)
    G = case["ngroups"]
    rc = capi.lib().misift_test_adjust_bundle_radial(
        case["max_tracks"], case["max_obs"], a["offs"].ctypes.data, a["obs"].ctypes.data, a["summ"].ctypes.data,
        a["pts"].ctypes.data, a["st"].ctypes.data, case["nimages"], a["cam"].ctypes.data, a["pair"].ctypes.data,
        a["K"].ctypes.data, len(a["hold"]), a["hold"].ctypes.data if len(a["hold"]) else None, case["min_views"],
        case["min_obs"], case["num_loops"], case["cg_iters"], float(case["max_error"]), float(case["lambda0"]),
        int(case["orthonormalise"]), int(case["loss"]), float(case["loss_scale"]), int(G),
        group.ctypes.data if G > 0 else None, flags.ctypes.data if flags is not None and G > 0 else None,
        k0.ctypes.data if k0 is not None and G > 0 else None, *[ptr[k] for k in OUTPUTS])
    assert rc == 0, rc
    return out


def hook_undistort(case, obs, words, in_place=False):
    """misift_test_undistort_obs: obs (max_obs records) under the d_radial words; the output starts poisoned."""
    from cudasift_amd import capi
    src = np.ascontiguousarray(obs[:case["max_obs"]]).copy()
    dst = src if in_place else np.frombuffer(np.full(4 * len(src), POISON_WORD, np.uint32).tobytes(), src.dtype).copy()
    summ = np.ascontiguousarray(case["export_summary"], np.int32)
    K = np.ascontiguousarray(case["intrinsics"], f32).reshape(-1, 4)
    group = np.ascontiguousarray(case["group"], np.int32).reshape(-1)
    words = np.ascontiguousarray(words, np.uint32)
    G = case["ngroups"]
    rc = capi.lib().misift_test_undistort_obs(case["max_obs"], src.ctypes.data, summ.ctypes.data, case["nimages"],
                                              K.ctypes.data, int(G), group.ctypes.data if G > 0 else None,
                                              words.ctypes.data if G > 0 else None, dst.ctypes.data)
    assert rc == 0, rc
    return dst


def expected_undistort(case, obs, words, in_place=False):
    """What hook_undistort and the device call leave: the slots below O under the model, the rest as they were."""
    _, O = RC.counts(case)
    src = np.ascontiguousarray(obs[:case["max_obs"]])
    out = src.copy() if in_place else np.frombuffer(np.full(4 * len(src), POISON_WORD, np.uint32).tobytes(), src.dtype).copy()
    kg = np.ascontiguousarray(words, np.uint32).reshape(-1, 3)[:, 0].copy().view(f32) if case["ngroups"] else np.zeros(1, f32)
    out[:O] = undistort(case, src, kg)[:O]
    return out


# ---- cases

def distort_obs(case, kg, forward=False):
    """The observations of a case displaced so that THE RADIAL MODEL with kg undoes it (float64 fixed point), or by the
    forward model x_d = x_u * (1 + k r_u^2) in normalised coordinates; kg per group, relative to the case's own fx, fy."""
    obs = np.array(case["obs"])
    n = case["nimages"]
    K = np.asarray(case["intrinsics"], np.float64).reshape(-1, 4)
    grp = np.asarray(case["group"], np.int64)
    fr = obs["frame"].astype(np.int64)
    ok = (fr >= 0) & (fr < n)
    g = np.where(ok, grp[np.where(ok, fr, 0)], -1)
    sel = np.nonzero(g >= 0)[0]
    Ks, k = K[fr[sel]], np.asarray(kg, np.float64)[g[sel]]
    xu, yu = obs["xpos"][sel].astype(np.float64), obs["ypos"][sel].astype(np.float64)
    if forward:
        nx, ny = (xu - Ks[:, 2]) / Ks[:, 0], (yu - Ks[:, 3]) / Ks[:, 1]
        sc = 1 + k * (nx * nx + ny * ny)
        xd, yd = Ks[:, 2] + (xu - Ks[:, 2]) * sc, Ks[:, 3] + (yu - Ks[:, 3]) * sc
    else:
        xd, yd = xu.copy(), yu.copy()
        for _ in range(60):                                        # x = xu - dx*e(x): a contraction for the k in use
            x2, y2, _, _ = model(Ks, k, xd, yd)
            xd, yd = xd - (x2 - xu), yd - (y2 - yu)
    obs["xpos"][sel], obs["ypos"][sel] = xd.astype(f32), yd.astype(f32)
    return dict(case, obs=obs)


def corner_k(case, rel):
    """The coefficient that displaces the image corner (taken as 2*cx, 2*cy of image 0) by the share `rel`."""
    K = np.asarray(case["intrinsics"], np.float64).reshape(-1, 4)[0]
    return rel / ((K[2] / K[0]) ** 2 + (K[3] / K[1]) ** 2)


def one_group(case, k=-0.15, fscale=1.05, k0=None, flags=True, **kw):
    """Every image in one group, the observations planted with the coefficient of corner share k."""
    c = BFC.one_group(case, fscale, **kw)
    c = distort_obs(c, [corner_k(c, k)]) if k else c
    return radial(c, flags, k0)


def alternating(case, k=(-0.15, 0.08), fscale=(0.97, 1.03), flags=True, k0=None, **kw):
    c = BFC.alternating(case, fscale, **kw)
    c = distort_obs(c, [corner_k(c, v) for v in k])
    return radial(c, flags, k0)


def recovery_scene(ntracks, nimages, seed, groups=1, forward=False, noise=0.5, num_loops=8, **kw):
    """bundle_focal_cases.recovery_scene planted with k = -0.15 (one group) or -0.15 / +0.08 (two taking turns) at the
    image corner, relative to the focal length as given: dict(case, focal_case (the same input for the focal call), k:
    the planted coefficients relative to the given fx, fy)."""
    sc = BFC.recovery_scene(ntracks, nimages, seed, groups=groups, noise=noise, num_loops=num_loops, **kw)
    rel = (-0.15,) if groups == 1 else (-0.15, 0.08)
    c = sc["case"]
    # the planted lens is relative to the true focal length, fx / fscale; relative to the given one k grows by fscale^2
    ktrue = np.array([corner_k(c, r) / sc["fscale"][g] ** 2 for g, r in enumerate(rel)])
    Ktrue = np.array(c["intrinsics"], np.float64).reshape(-1, 4)
    for i, g in enumerate(c["group"]):
        Ktrue[i, :2] /= sc["fscale"][g]
    d = distort_obs(dict(c, intrinsics=Ktrue), ktrue, forward=forward)
    c = dict(c, obs=d["obs"])
    return dict(sc, case=radial(c, True), focal_case=c, k=ktrue * sc["fscale"] ** 2)


def hostile_obs_case(**kw):
    """8 images in two groups: one observation exactly at the principal point, one at 1e20 (rho2 stays finite, dx*rho2
    and dx*e overflow), one at 3e38 (rho2 itself overflows: x' is NaN whatever k is), one NaN."""
    c = alternating(BC.planted(120, 8, 6, num_loops=3, max_error=2000.0, **kw)["case"])
    obs = np.array(c["obs"])
    K = np.asarray(c["intrinsics"], f32).reshape(-1, 4)
    f = int(obs["frame"][5])
    obs["xpos"][5], obs["ypos"][5] = K[f, 2], K[f, 3]
    obs["xpos"][40] = 1e20
    obs["ypos"][120] = 3e38
    obs["ypos"][77] = np.nan
    return dict(c, obs=obs)


def behind_trial_case():
    """bundle_cases.behind_trial_case at lambda0 1e-5 with image 2, the one far off, alone in a group whose coefficient
    is an unknown: the first step is kept, the next three trial states have a member behind a trial camera, the fifth at
    10^3 times the damping is kept (so this is the rejected-then-kept case too)."""
    return radial(BFC.focal(dict(BC.behind_trial_case(), lambda0=1e-5), [-1, -1, 0], 1), True)


def not_finite_k_case(ntracks=6, k0=3.0e38, F=1.8e19, U=2e18, depth=1e6, baseline=1e5):
    """A trial coefficient that overflows.  Two images, the root and a held one, so that only the points, s and k move;
    image 1 alone in a group with k0 = 3.0e38, a focal length of 1.8e19 and its principal point at 0, both cameras
    looking down z, the points at depth 1e6.  A point projects to u (|u| about 1e18 px) in image 1, and its observation
    there is placed so that the model at k0 puts it at x' = u / 2 (|x| about 1e6 px, rho2 about 3e-27, e about 1e12): the
    residual -u / 2 lies along both the focal and the radial column, s_g and k_g share it, and k_g's share, about a
    tenth of k0, carries k0 + x_k past FLT_MAX while s_g + x_g stays near 0.9.  Juk is about 1.6e-21, so U_kk and S_kk
    are sums of fp32 denormals.  The steps: not finite, not finite, kept (at 100 times the damping), not finite, kept,
    not finite."""
    base = BC.planted(ntracks, 2, 5, lengths=(2,), num_loops=6, cg_iters=1, lambda0=0.1)["case"]
    offs, obs = np.asarray(base["track_offsets"]), np.array(base["obs"])
    cam = np.zeros((2, 12), f32)
    cam[:, [0, 4, 8]] = 1
    cam[0, 9] = -baseline
    K = np.array([[500, 500, 320, 240], [F, F, 0, 0]], f32)
    pts = np.array(base["points"], f32).reshape(-1, 4).copy()
    angle = np.linspace(0.3, 2 * np.pi + 0.3, ntracks, endpoint=False)
    for t in range(ntracks):
        u = np.array([np.cos(angle[t]), np.sin(angle[t])]) * U * (0.6 + 0.4 * t / ntracks)
        X = np.array([u[0] / F * depth, u[1] / F * depth, depth])
        pts[t, :3] = X
        want = np.linalg.norm(u / 2)                               # m + k0 m^3 / F^2 = |x'| for m = |x|, by Newton
        m = (want * F * F / k0) ** (1 / 3)
        for _ in range(50):
            m -= (m + k0 * m ** 3 / F ** 2 - want) / (1 + 3 * k0 * m ** 2 / F ** 2)
        for o in range(offs[t], offs[t + 1]):
            if obs["frame"][o] == 1:
                obs["xpos"][o], obs["ypos"][o] = u / np.linalg.norm(u) * m
            else:
                obs["xpos"][o], obs["ypos"][o] = 500 * (X[0] + baseline) / depth + 320, 500 * X[1] / depth + 240
    case = dict(base, obs=obs, cam=cam, intrinsics=K, points=pts, max_error=RC.INF, orthonormalise=0)
    return radial(BFC.focal(case, [-1, 0], 1), [1], [k0])


def held_group_case(**kw):
    """Two groups: the coefficient of group 0 is held at the planted value, that of group 1 is an unknown."""
    c = alternating(BC.planted(60, 4, 1, lengths=(3, 4), **kw)["case"], flags=None)
    return radial(c, [0, 1], [corner_k(c, -0.15), 0.0])


def all_held_case(**kw):
    """No unknown coefficient, but a start that is not zero: the RADIAL instances run for the observations alone."""
    c = one_group(BC.planted(40, 4, 1, **kw)["case"], flags=None)
    return radial(c, [0], [corner_k(c, -0.15)])


def empty_groups_case(**kw):
    c = BFC.empty_groups_case(**kw)
    c = distort_obs(c, [corner_k(c, -0.1), 0.0, 0.0, corner_k(c, 0.05)])
    return radial(c, [1, 1, 1, 0], [0.0, 0.01, 0.0, 0.02])


def max_groups_case(**kw):
    c = BFC.max_groups_case(**kw)
    c = distort_obs(c, [corner_k(c, v) for v in np.linspace(-0.12, 0.08, 8)])
    return radial(c, [1, 0, 1, 1, 0, 1, 1, 1], np.zeros(8, f32))


def undistort_case(O):
    """300 slots over five images in three groups and one image in none, a frame of -1 and one of nimages, a NaN and a
    position at the principal point, with O as the device would report it (300 is the capacity)."""
    base = BFC.focal(BC.bundle_case(RC.spread_case(300, nimages=5)), [0, 1, -1, 2, 0], 3)
    assert base["max_obs"] == 300
    obs = np.array(base["obs"])
    K = np.asarray(base["intrinsics"], f32).reshape(-1, 4)
    obs["frame"][0], obs["frame"][2] = -1, 5
    obs["xpos"][1] = np.nan
    f = int(obs["frame"][4])
    obs["xpos"][4], obs["ypos"][4] = K[f, 2], K[f, 3]
    return RC.with_counts(dict(base, obs=obs), None, O)


IMAGE_SHAPES = BFC.IMAGE_SHAPES
TRACK_COUNTS = BFC.TRACK_COUNTS
DEVICE_COUNTS = BFC.DEVICE_COUNTS


def image_count_case(nimages, ntracks, loops, cg):
    return one_group(BC.image_count_case(nimages, ntracks, loops, cg), -0.1)


def track_count_case(ntracks):
    return one_group(BC.track_count_case(ntracks), -0.1)


def device_counts_case(T, O):
    return radial(BFC.device_counts_case(T, O), True)


def identity_cases():
    """name -> case: those in which the call is the focal call."""
    base = BC.planted(40, 4, 1)["case"]
    return {"ngroups 0": radial(BFC.focal(base, [], 0)), "all -1": radial(BFC.focal(base, [-1] * 4, 2, loss=HUBER), True),
            "nothing radial": radial(BFC.one_group(base), [0], [0.0]), "no lists": radial(BFC.alternating(base))}


def cpu_cases():
    """name -> case: every case test_bundle_radial_cpu.py holds the hook to; test_gpu_bundle_radial.py runs these and
    the larger shapes on the device."""
    out = {"2 images": one_group(BC.planted(30, 2, 4)["case"]), "3 images": one_group(BC.planted(60, 3, 3, cg_iters=6)["case"]),
           "8 images": one_group(BC.planted(120, 8, 6, num_loops=3)["case"]),
           "two groups": alternating(BC.planted(40, 4, 1, lengths=(3, 4))["case"]),
           "some ungrouped": distort_obs(radial(BFC.ungrouped_track_case(), True), [corner_k(BFC.ungrouped_track_case(), -0.1)]),
           "empty groups": empty_groups_case(), "8 groups, mixed": max_groups_case(num_loops=2, cg_iters=4),
           "held group": held_group_case(), "all held": all_held_case(),
           "members": one_group(BC.member_counts_case(num_loops=2, cg_iters=3)[0], -0.1, 1.03),
           "views": alternating(BC.views_case(num_loops=2, cg_iters=4)),
           "hostile": radial(BFC.focal(BC.hostile_case(num_loops=3, cg_iters=5), np.arange(BC.hostile_case()["nimages"]) % 2, 2),
                             [1, 1], [0.01, -0.02]),
           "hostile observations": hostile_obs_case(),
           "no track": radial(BFC.one_group(BC.frames_case([], 3, 83)), True),
           "no loop": one_group(BC.planted(40, 4, 1, num_loops=0)["case"]),
           "cg 0": one_group(BC.planted(40, 4, 1, cg_iters=0)["case"]), "cg 1": one_group(BC.planted(40, 4, 1, cg_iters=1)["case"]),
           "huge lambda": one_group(BC.planted(40, 4, 1, lambda0=3e38, num_loops=3)["case"]),
           "far off": one_group(BC.rejected_then_kept_case()), "behind, rejected then kept": behind_trial_case(),
           "k not finite": not_finite_k_case()}
    for loss, c in LOSSES[1:]:
        tag = "huber" if loss == HUBER else "geman-mcclure"
        out["two groups, " + tag] = alternating(BC.planted(40, 4, 1, lengths=(3, 4))["case"], loss=loss, loss_scale=c)
        out["outlier scene, " + tag] = one_group(BRC.outlier_case(loss, c)[0], -0.1)
    out.update(identity_cases())
    return out

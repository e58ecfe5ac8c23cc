"""misift_adjust_bundle_focal_batch: the numpy restatement of the definition in include/misift.h, which is that of
misift_adjust_bundle_robust_batch (bundle_robust_cases.py) with one focal scale s_g per camera group among the unknowns.
The sets, the sums, the solves, the linearisation and the loss are bundle_cases' and bundle_robust_cases' own; lm_step and
adjust are restated here with the focal columns, and so are the expected outputs: the ten shared ones and the two
new ones.  A case is a case of bundle_robust_cases with `ngroups` and `group`.  test_bundle_focal_cpu.py pins the
restatement to the library's host hook, to float64 and to dense linear algebra, test_gpu_bundle_focal.py holds the device
to it byte for byte.  No GPU in here, and cudasift_amd.capi is imported inside functions only."""
import numpy as np

import bundle_cases as BC
import bundle_robust_cases as BRC
import pose_cases as PC
import refine_cases as RC
from bundle_cases import (LAMBDA_FLOOR, NO_CAMERA, POISON_WORD, Problem, cross_sum, dot6, linearise, pos_sum, solve3,
                          solve6, track_sum, w3, wt6)
from bundle_robust_cases import NONE, HUBER, GEMAN_MCCLURE, loss_terms, scale_of
from test_fundamental_cpu import f32

MAX_GROUPS = 8                                                     # MISIFT_MAX_FOCAL_GROUPS
REFINED, NO_MEMBER, NOT_REFINED = 0, 1, 2                          # MISIFT_FOCAL_*
OUTPUTS = BRC.OUTPUTS + ("intrinsics_out", "focal")                # in the order of the call's arguments
INT_OUTPUTS = BRC.INT_OUTPUTS


def focal(case, group, ngroups=None, loss=NONE, loss_scale=2.0, fscale=None):
    """A case of this call from a case of bundle_cases: the group of every image, the loss, and with fscale the given fx,
    fy multiplied by it (a scalar, or one factor per group; an image with group -1 keeps its own)."""
    group = np.asarray(group, np.int32).reshape(-1)
    if ngroups is None:
        ngroups = int(group.max()) + 1 if len(group) else 0
    out = dict(case, group=group, ngroups=ngroups, loss=case.get("loss", loss), loss_scale=case.get("loss_scale", loss_scale))
    if fscale is not None:
        K = np.array(case["intrinsics"], f32).reshape(-1, 4)
        fs = np.broadcast_to(np.asarray(fscale, np.float64), (max(ngroups, 1),))
        for i, g in enumerate(group):
            if g >= 0:
                K[i, :2] = (K[i, :2].astype(np.float64) * fs[g]).astype(f32)
        out["intrinsics"] = K
    return out


def grouped(case):
    return case["ngroups"] > 0 and bool((np.asarray(case["group"]) >= 0).any())


class Groups:
    """The groups of a Problem: the group of every image and member, the members M_g, the live groups."""

    def __init__(self, case, P):
        self.G = case["ngroups"]
        self.grp = np.asarray(case["group"], np.int64) if self.G > 0 else np.full(P.n, -1, np.int64)
        assert len(self.grp) == P.n and ((self.grp >= -1) & (self.grp < max(self.G, 1))).all()
        self.mg = self.grp[P.img]
        self.count = np.bincount(self.mg[self.mg >= 0], minlength=max(self.G, 1))[:max(self.G, 1)]
        self.live = [g for g in range(self.G) if self.count[g] > 0]
        self.images = {g: np.nonzero((self.grp == g) & (P.state != NO_CAMERA))[0] for g in self.live}

    def intrinsics(self, P, s):
        """fx*s_g, fy*s_g, cx, cy per member, each product rounded; s = 1 for a member of an image without a group."""
        K = P.K[P.img].copy()
        sc = np.where(self.mg >= 0, s[np.maximum(self.mg, 0)], P.dt(1)).astype(P.dt)
        K[:, 0] = K[:, 0] * sc
        K[:, 1] = K[:, 1] * sc
        return K


def costs(P, Gr, cams, pts, s, loss, c, c2):
    """(in front (m,), s per member, rho per member, c_i per image, c) of a state."""
    dt = P.dt
    _, _, zc, _, _, _, ru, rv = RC.view(cams[P.img].T, Gr.intrinsics(P, s).T, pts[P.trk], P.x, P.y, dt)
    sq = ru * ru + rv * rv
    rho = loss_terms(sq, loss, c, c2, dt)[0]
    ci = np.array([pos_sum(rho[m].reshape(-1, 1), dt)[0] for m in P.of_image], dt)
    return zc > 0, sq, rho, ci, cross_sum(ci, np.arange(P.n), dt)


def wf3(wf, v):
    return (wf[:, 0] * v[:, 0] + wf[:, 1] * v[:, 1]) + wf[:, 2] * v[:, 2]


def jacobian(P, Gr, cams, pts, s, loss, c, c2):
    """Step 1: (lin (m, 20), f (m, 2), lin0, f0 before the loss, w)."""
    dt = P.dt
    Kf = Gr.intrinsics(P, s)
    front, l0 = linearise(cams[P.img], Kf, pts[P.trk], P.x, P.y, dt)
    assert front.all()
    _, _, _, _, a, b, _, _ = RC.view(cams[P.img].T, Kf.T, pts[P.trk], P.x, P.y, dt)
    Kg = P.K[P.img]
    f0 = np.stack([Kg[:, 0] * a, Kg[:, 1] * b], 1).astype(dt) if len(a) else np.zeros((0, 2), dt)
    wgt = np.ones(len(l0), dt)
    l, f = l0, f0
    if loss != NONE:
        _, wgt, sw = loss_terms(l0[:, 18] * l0[:, 18] + l0[:, 19] * l0[:, 19], loss, c, c2, dt)
        l = (sw[:, None] * l0).astype(dt)
        f = (sw[:, None] * f0).astype(dt)
    return l, f, l0, f0, wgt


def lm_step(P, Gr, cams, pts, s, lam, cg_iters, dt, loss=NONE, c=None, c2=None):
    """Steps 1-5 at damping lam with the focal columns: dict(fail, cams, pts, s (the trial state), iters, x, xg, ...)."""
    n, T, G = P.n, len(P.pts0), Gr.G
    lam1 = dt(1) + lam
    l, f, l0, f0, wgt = jacobian(P, Gr, cams, pts, s, loss, c, c2)
    mg = Gr.mg
    wf = np.stack([f[:, 0] * l[:, 12 + q] + f[:, 1] * l[:, 15 + q] for q in range(3)], 1) if len(l) else np.zeros((0, 3), dt)
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
    tfd = np.zeros((T, max(G, 1)), dt)
    for g in Gr.live:
        sel = mg == g
        wgt_t = track_sum(wf[sel], P.trk[sel], T, dt)
        xs, _ = solve3(V[act], wgt_t[act])
        tfd[act, g] = wf3(wgt_t[act], xs)
    nf = len(P.free)
    U = np.zeros((nf, 6, 6), dt)
    b = np.zeros((nf, 6), dt)
    ucf = np.zeros((n, 6), dt)
    foc = np.zeros((n, 3), dt)
    for i in range(n):
        if Gr.grp[i] < 0 or P.state[i] == NO_CAMERA:
            continue
        m = P.of_image[i]
        fm, lm = f[m], l[m]
        cols = [fm[:, 0] * fm[:, 0] + fm[:, 1] * fm[:, 1], fm[:, 0] * lm[:, 18] + fm[:, 1] * lm[:, 19],
                wf3(wf[m], yt[P.trk[m]])]
        foc[i] = pos_sum(np.stack(cols, 1), dt)
        if P.state[i] == BC.ADJUSTED:
            ucf[i] = pos_sum(np.stack([lm[:, r] * fm[:, 0] + lm[:, 6 + r] * fm[:, 1] for r in range(6)], 1), dt)
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
    out = dict(fail=fail, iters=0, x=np.zeros((nf, 6), dt), xg=np.zeros(max(G, 1), dt), cams=cams, pts=pts, s=s, lin=l,
               f=f, lin0=l0, f0=f0, w=wgt, U=U, b=b, V=V, gp=gp, ucf=ucf, foc=foc, tfd=tfd)
    if fail:
        return out
    UL, S, bg = np.zeros(max(G, 1), dt), np.ones(max(G, 1), dt), np.zeros(max(G, 1), dt)
    for g in Gr.live:
        u = RC.slot_sum(foc[Gr.images[g]], Gr.images[g], dt)
        Dg = RC.slot_sum(tfd[act, g].reshape(-1, 1), act, dt)[0]
        UL[g] = u[0] * lam1
        S[g] = UL[g] - Dg
        bg[g] = u[1] - u[2]
        if not (np.isfinite(S[g]) and S[g] > 0):
            fail = True
    out.update(UL=UL, S=S, bg=bg)
    if fail:
        return dict(out, fail=True)
    fpos = np.full(n, -1, np.int64)
    fpos[P.free] = np.arange(nf)

    def dot(a, ag, bb, bbg):
        acc = cross_sum(dot6(a, bb), P.free, dt)
        for g in Gr.live:
            acc = acc + ag[g] * bbg[g]
        return acc

    def gather(v, vg):
        """Per track, per member in ascending slot: (W^T v_i) if its image is free, then wf * v_g if it has a group."""
        terms = np.zeros((len(l), 2, 3), dt)
        valid = np.stack([P.in_free, mg >= 0], 1) if len(l) else np.zeros((0, 2), bool)
        mf = np.nonzero(P.in_free)[0]
        terms[mf, 0] = wt6(l[mf], v[fpos[P.img[mf]]])
        mgr = np.nonzero(mg >= 0)[0]
        terms[mgr, 1] = wf[mgr] * vg[mg[mgr]][:, None]
        return track_sum(terms.reshape(-1, 3)[valid.reshape(-1)], np.repeat(P.trk, 2)[valid.reshape(-1)], T, dt)

    x, xg = np.zeros((nf, 6), dt), np.zeros(max(G, 1), dt)
    r, rg = b.copy(), bg.copy()
    z, _ = solve6(U, r)
    zg = (rg / S).astype(dt)
    p, pg = z.copy(), zg.copy()
    rho = dot(r, rg, z, zg)
    alive = bool(np.isfinite(rho))
    iters = 0
    for _ in range(cg_iters):
        if not alive:
            break
        st = gather(p, pg)
        q = np.zeros((T, 3), dt)
        q[act], _ = solve3(V[act], st[act])
        yv = np.zeros((nf, 6), dt)
        ci, wq = np.zeros(n, dt), np.zeros(n, dt)
        for i in range(n):
            if P.state[i] == NO_CAMERA or (Gr.grp[i] < 0 and P.state[i] != BC.ADJUSTED):
                continue
            m, g = P.of_image[i], Gr.grp[i]
            if g >= 0:
                wq[i] = pos_sum(wf3(wf[m], q[P.trk[m]]).reshape(-1, 1), dt)[0]
            if P.state[i] != BC.ADJUSTED:
                continue
            fi = fpos[i]
            sm = pos_sum(w3(l[m], q[P.trk[m]]), dt)
            Up = np.array([dot6(U[fi, rr], p[fi]) for rr in range(6)], dt)
            if g >= 0:
                yv[fi] = (Up + ucf[i] * pg[g]) - sm
                ci[i] = dot6(ucf[i], p[fi])
            else:
                yv[fi] = Up - sm
        yg = np.zeros(max(G, 1), dt)
        for g in Gr.live:
            im = Gr.images[g]
            v = RC.slot_sum(np.stack([ci[im], wq[im]], 1), im, dt)
            yg[g] = (UL[g] * pg[g] + v[0]) - v[1]
        sigma = dot(p, pg, yv, yg)
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
        rho2 = dot(r, rg, z, zg)
        iters += 1
        if not np.isfinite(rho2):
            break
        beta = rho2 / rho
        p = z + beta * p
        for g in Gr.live:
            pg[g] = zg[g] + beta * pg[g]
        rho = rho2
    st = gather(x, xg)
    delta = np.zeros((T, 3), dt)
    delta[act], _ = solve3(V[act], gp[act] - st[act])
    pts2 = pts.copy()
    pts2[act] = pts[act] + delta[act]
    cams2 = cams.copy()
    for fi, i in enumerate(P.free):
        cams2[i] = RC.update(cams[i], x[fi], dt)
    s2 = s.copy()
    for g in Gr.live:
        s2[g] = s[g] + xg[g]
    return dict(out, fail=False, iters=iters, x=x, xg=xg, delta=delta, cams=cams2, pts=pts2, s=s2)


def adjust(case, dt=f32):
    """The call restated, as bundle_robust_cases.adjust, with scale (the final s_g), groups and strace: the trial scale of
    every step that got as far."""
    if not grouped(case):
        res = BRC.adjust(case, dt)
        Gr = Groups(dict(case, group=np.full(case["nimages"], -1), ngroups=case["ngroups"]), res["problem"])
        return dict(res, scale=np.ones(max(case["ngroups"], 1), dt), groups=Gr, strace=[])
    P = Problem(case, dt)
    Gr = Groups(case, P)
    loss = case["loss"]
    c, c2 = scale_of(case, dt) if loss != NONE else (None, None)
    nan = PC.ONE_NAN if dt is f32 else dt(np.nan)
    with np.errstate(all="ignore"):
        cams, pts, s = P.cams0.copy(), P.pts0.copy(), np.ones(max(Gr.G, 1), dt)
        front, sq, e, ci, cost = costs(P, Gr, cams, pts, s, loss, c, c2)
        ci0, c0 = ci, cost
        lam = dt(f32(case["lambda0"]))
        floor = dt(f32(LAMBDA_FLOOR))
        history, trace, strace, kept_steps = [], [], [], 0
        for _ in range(case["num_loops"]):
            st = lm_step(P, Gr, cams, pts, s, lam, case["cg_iters"], dt, loss, c, c2)
            kept, cc2, why = False, nan, "singular"
            if not st["fail"]:
                act = np.nonzero(P.active)[0]
                strace.append(st["s"].copy())
                sl = st["s"][Gr.live]
                finite = (np.isfinite(st["cams"][P.free]).all() and np.isfinite(st["pts"][act]).all() and
                          bool((np.isfinite(sl) & (sl > 0)).all()))
                front2, sq2, e2, ci2, cc = costs(P, Gr, st["cams"], st["pts"], st["s"], loss, c, c2)
                why = "not finite" if not finite else "behind"
                if finite and front2.all():
                    cc2 = nan if np.isnan(cc) else cc
                    kept = bool(cc < cost)
                    why = "kept" if kept else "worse"
            trace.append(why)
            history.append((cc2, lam, int(kept), st["iters"]))
            if kept:
                cams, pts, s, front, sq, e, ci, cost = st["cams"], st["pts"], st["s"], front2, sq2, e2, ci2, cc
                kept_steps += 1
                lo = lam / dt(10)
                lam = lo if lo > floor else floor
            else:
                lam = lam * dt(10)
        wgt = loss_terms(sq, loss, c, c2, dt)[1]
    return dict(problem=P, groups=Gr, cams=cams, pts=pts, scale=s, cost=(c0, cost), history=history, ci0=ci0, ci1=ci, e=e,
                s=sq, front=front, w=wgt, kept=kept_steps, trace=trace, strace=strace)


pooled_rms = BRC.pooled_rms


def shared_outputs(case, res):
    """The ten outputs the call shares with the robust call, from the result of `adjust`: as
    bundle_robust_cases.expected_bundle builds them from its own."""
    P = res["problem"]
    n, mt, mo, T, O = P.n, case["max_tracks"], case["max_obs"], P.T, P.O
    cam_out = P.cam_in.view(np.uint32).copy()
    own = np.isin(P.state, (BC.ADJUSTED, BC.FEW_OBS))
    cam_out[own] = res["cams"][own].astype(f32).view(np.uint32)
    one_nan = lambda v: np.where(np.isnan(v), PC.ONE_NAN, v).astype(f32)
    with np.errstate(all="ignore"):
        rms = np.full((n, 2), PC.ONE_NAN, f32)
        has = P.icount > 0
        cnt = P.icount[has].astype(f32)
        rms[has, 0] = np.sqrt(res["ci0"][has] / cnt)
        rms[has, 1] = np.sqrt(res["ci1"][has] / cnt)
        points_out = np.full((mt, 4), POISON_WORD, np.uint32)
        points_out[:T] = np.ascontiguousarray(P.pts_in[:T]).view(np.uint32)
        act = np.nonzero(P.active)[0]
        ct = track_sum(np.asarray(res["e"], f32).reshape(-1, 1), P.trk, max(T, 1), f32)[:, 0]
        points_out[act, :3] = res["pts"][act].astype(f32).view(np.uint32)
        points_out[act, 3] = one_nan(np.sqrt(ct[act] / P.tcount[act].astype(f32))).view(np.uint32)
    point_obs = np.full(mt, POISON_WORD, np.uint32)
    point_obs[:T] = P.tcount[:T].astype(np.int32).view(np.uint32)
    history = np.full(max(4 * case["num_loops"], 1), POISON_WORD, np.uint32)
    for k, (c2, lam, kept, iters) in enumerate(res["history"]):
        history[4 * k:4 * k + 2] = np.array([c2, lam], f32).view(np.uint32)
        history[4 * k + 2:4 * k + 4] = [kept, iters]
    weight = np.full(mo, POISON_WORD, np.uint32)
    wo = np.full(O, -1.0, f32)
    wo[P.slot] = one_nan(np.where(res["front"], res["w"], PC.ONE_NAN).astype(f32))
    weight[:O] = wo.view(np.uint32)
    summary = np.array([T, (P.state == BC.ADJUSTED).sum(), len(P.slot), (P.state == BC.FEW_OBS).sum(), P.active.sum(),
                        (P.state == BC.HELD).sum(), res["kept"], (P.state == NO_CAMERA).sum()], np.int32)
    return dict(cam_out=cam_out.reshape(-1), points_out=points_out.reshape(-1),
                cam_obs=P.icount.astype(np.int32).view(np.uint32), cam_status=P.state.astype(np.int32).view(np.uint32),
                cam_rms=one_nan(rms).reshape(-1).view(np.uint32), point_obs=point_obs, history=history,
                cost=one_nan(np.array(res["cost"], f32)).view(np.uint32), obs_weight=weight,
                summary=summary.view(np.uint32))


def expected_focal(case):
    """The twelve outputs of the call as uint32 arrays of exactly the stated sizes (poison where the call writes nothing),
    and the restatement's own dict under 'res'.  Without a grouped image the ten shared ones are
    bundle_robust_cases.expected_bundle's own, from its own adjust."""
    if grouped(case):
        res = adjust(case, f32)
        e = shared_outputs(case, res)
    else:
        e = BRC.expected_bundle(case)
        res = adjust(case, f32)
    P, Gr = res["problem"], res["groups"]
    G, loops = case["ngroups"], case["num_loops"]
    K = np.ascontiguousarray(case["intrinsics"], f32).reshape(-1, 4)
    kout = K.view(np.uint32).copy()
    foc = np.full(max(3 * G, 1), POISON_WORD, np.uint32)
    for g in range(G):
        live = grouped(case) and Gr.count[g] > 0
        status = NOT_REFINED if loops == 0 else (REFINED if live else NO_MEMBER)
        foc[3 * g] = np.array([res["scale"][g]], f32).view(np.uint32)[0]
        foc[3 * g + 1] = int(Gr.count[g]) if grouped(case) else 0
        foc[3 * g + 2] = status
        if status == REFINED:
            for i in np.nonzero((Gr.grp == g) & (P.state != NO_CAMERA))[0]:
                kout[i, :2] = (K[i, :2] * f32(res["scale"][g])).astype(f32).view(np.uint32)
    return dict(e, res=res, intrinsics_out=kout.reshape(-1), focal=foc)


def sizes(case):
    return dict(BRC.sizes(case), intrinsics_out=4 * case["nimages"], focal=max(3 * case["ngroups"], 1))


def compare_all(got, e, what, keys=OUTPUTS):
    for k in keys:
        bad = np.nonzero(got[k] != e[k])[0]
        view = np.int32 if k in INT_OUTPUTS else f32
        assert len(bad) == 0, (what, k, "%d words differ, first %s" % (len(bad), bad[:8]), got[k][bad[:4]].view(view),
                               e[k][bad[:4]].view(view))


# ---- the hook

def hook_bundle_focal(case, in_place=False, weights=True):
    """misift_test_adjust_bundle_focal on poisoned outputs of exactly the stated sizes, as uint32 arrays; weights=False
    passes NULL for obs_weight, whose array then comes back as it was poisoned."""
    from cudasift_amd import capi
    a = BRC.hook_args(case)
    out = {k: np.full(m, POISON_WORD, np.uint32) for k, m in sizes(case).items()}
    if in_place:
        out["cam_out"], out["points_out"] = a["cam"].reshape(-1).view(np.uint32), a["pts"].reshape(-1).view(np.uint32)
    ptr = {k: out[k].ctypes.data for k in OUTPUTS}
    if not weights:
        ptr["obs_weight"] = None
    group = np.ascontiguousarray(case["group"], np.int32).reshape(-1)
    rc = capi.lib().misift_test_adjust_bundle_focal(
        case["max_tracks"], case["max_obs"], a["offs"].ctypes.data, a["obs"].ctypes.data, a["summ"].ctypes.data,
        a["pts"].ctypes.data, a["st"].ctypes.data, case["nimages"], a["cam"].ctypes.data, a["pair"].ctypes.data,
        a["K"].ctypes.data, len(a["hold"]), a["hold"].ctypes.data if len(a["hold"]) else None, case["min_views"],
        case["min_obs"], case["num_loops"], case["cg_iters"], float(case["max_error"]), float(case["lambda0"]),
        int(case["orthonormalise"]), int(case["loss"]), float(case["loss_scale"]), int(case["ngroups"]),
        group.ctypes.data if case["ngroups"] > 0 else None, *[ptr[k] for k in OUTPUTS])
    assert rc == 0, rc
    return out


# ---- cases

def one_group(case, fscale=1.1, **kw):
    return focal(case, np.zeros(case["nimages"], np.int32), 1, fscale=fscale, **kw)


def alternating(case, fscale=(0.9, 1.1), **kw):
    """Two cameras taking turns."""
    return focal(case, np.arange(case["nimages"]) % 2, 2, fscale=fscale, **kw)


def recovery_scene(ntracks, nimages, seed, groups=1, noise=0.5, num_loops=8, **kw):
    """planted(ntracks, nimages, seed) with fx, fy 10 % off (one group) or 0.9 / 1.1 (two alternating): dict(case, true,
    X, fscale: the factor the given focal is off by, so that 1 / fscale is the planted s_g)."""
    sc = BC.planted(ntracks, nimages, seed, noise=noise, num_loops=num_loops, **kw)
    fs = (1.1,) if groups == 1 else (0.9, 1.1)
    case = one_group(sc["case"], fs[0]) if groups == 1 else alternating(sc["case"], fs)
    return dict(sc, case=case, fscale=np.array(fs))


def non_positive_scale_case(**kw):
    """bundle_cases.behind_trial_case with image 2, the one far off, alone in a group: the first step is kept, the second
    overshoots to a trial scale near -10, which is not > 0, and is turned away like every step after it."""
    return focal(BC.behind_trial_case(**kw), [-1, -1, 0], 1)


def behind_trial_case(**kw):
    """The same scene with the held image 1 alone in a group: the first three trial states have a member behind, the
    fourth is worse, the fifth at 10^4 times the damping is kept (so this is the rejected-then-kept case too)."""
    return focal(BC.behind_trial_case(**kw), [-1, 0, -1], 1, fscale=1.02)


def two_group_track_case(**kw):
    """Tracks over four images whose cameras alternate: every track of three views has members in both groups."""
    return alternating(BC.planted(40, 4, 1, lengths=(3, 4), **kw)["case"])


def ungrouped_track_case(**kw):
    """Images 0 and 1 without a group, 2 and 3 in group 0: the tracks over (0, 1) have no grouped member."""
    return focal(BC.planted(40, 4, 1, lengths=(2, 3), **kw)["case"], [-1, -1, 0, 0], 1, fscale=1.05)


def empty_groups_case(**kw):
    """Four groups: 0 the images 0 and 2, 1 no image, 2 the image 3 which no track sees, 3 the image 1."""
    frames = [(0, 1, 2)] * 20 + [(0, 2)] * 6 + [(1, 2)] * 6
    base = BC.frames_case(frames, 4, 132, hold=(1,), noise=0.3, angle=0.01, shift=0.02, point_noise=0.02, **kw)
    return focal(base, [0, 3, 0, 2], 4, fscale=(1.05, 1.0, 1.0, 0.95))


def max_groups_case(**kw):
    return focal(BC.planted(120, 8, 6, **kw)["case"], np.arange(8), MAX_GROUPS, fscale=np.linspace(0.93, 1.07, 8))


IMAGE_SHAPES = ((2, 30, 5, 10), (3, 60, 5, 6), (8, 120, 5, 10), (65, 400, 2, 4), (257, 1300, 2, 3))
TRACK_COUNTS = BC.TRACK_COUNTS
DEVICE_COUNTS = BC.DEVICE_COUNTS
LOSSES = ((NONE, 0.0), (HUBER, 2.0), (GEMAN_MCCLURE, 4.0))


def image_count_case(nimages, ntracks, loops, cg):
    return one_group(BC.image_count_case(nimages, ntracks, loops, cg), 1.05)


def track_count_case(ntracks):
    return one_group(BC.track_count_case(ntracks), 1.05)


def device_counts_case(T, O):
    return one_group(BC.device_counts_case(T, O), 1.05)


def cpu_cases():
    """name -> case: every case test_bundle_focal_cpu.py holds the hook to; test_gpu_bundle_focal.py runs these and the
    larger shapes on the device."""
    out = {"2 images": one_group(BC.planted(30, 2, 4)["case"]), "3 images": one_group(BC.planted(60, 3, 3, cg_iters=6)["case"]),
           "8 images": one_group(BC.planted(120, 8, 6, num_loops=3)["case"]),
           "two groups": two_group_track_case(), "some ungrouped": ungrouped_track_case(),
           "empty groups": empty_groups_case(), "8 groups": max_groups_case(num_loops=2, cg_iters=4),
           "members": one_group(BC.member_counts_case(num_loops=2, cg_iters=3)[0], 1.03),
           "views": alternating(BC.views_case(num_loops=2, cg_iters=4), (0.97, 1.03)),
           "hostile": focal(BC.hostile_case(num_loops=3, cg_iters=5), np.arange(BC.hostile_case()["nimages"]) % 2, 2),
           "no track": one_group(BC.frames_case([], 3, 83)), "no loop": one_group(BC.planted(40, 4, 1, num_loops=0)["case"]),
           "cg 0": one_group(BC.planted(40, 4, 1, cg_iters=0)["case"]), "cg 1": one_group(BC.planted(40, 4, 1, cg_iters=1)["case"]),
           "huge lambda": one_group(BC.planted(40, 4, 1, lambda0=3e38, num_loops=3)["case"]),
           "far off": one_group(BC.rejected_then_kept_case()), "behind, rejected then kept": behind_trial_case(),
           "scale not positive": non_positive_scale_case(),
           "all -1": focal(BC.planted(40, 4, 1)["case"], [-1] * 4, 2, loss=HUBER),
           "ngroups 0": focal(BC.planted(40, 4, 1)["case"], [], 0)}
    for loss, c in LOSSES[1:]:
        tag = "huber" if loss == HUBER else "geman-mcclure"
        out["two groups, " + tag] = two_group_track_case(loss=loss, loss_scale=c)
        out["outlier scene, " + tag] = one_group(BRC.outlier_case(loss, c)[0], 1.05)
    return out

"""misift_adjust_bundle_robust_batch: the numpy restatement of the definition in include/misift.h, which is that of
misift_adjust_bundle_batch (bundle_cases.py) with three amendments: a member's 20 linearised values are scaled by sw, the
cost sums rho, and the weights of the final state are an output.  The sets, the sums, the solves and the linearisation
are bundle_cases' own; lm_step, adjust and the expected outputs are restated here with the loss.  A case is a case of
bundle_cases with `loss` and `loss_scale`.  test_bundle_robust_cpu.py pins the restatement to the library's host hook
and to float64, test_gpu_bundle_robust.py holds the device to it byte for byte.  No GPU in here, and cudasift_amd.capi
is imported inside functions only."""
import numpy as np

import bundle_cases as BC
import filter_cases as FC
import pose_cases as PC
import refine_cases as RC
from bundle_cases import (ADJUSTED, DEVICE_COUNTS, FEW_OBS, HELD, IMAGE_SHAPES, LAMBDA_FLOOR, NO_CAMERA, POISON_WORD,
                          TRACK_COUNTS, Problem, behind_trial_case, bundle_case, compare, cross_sum, device_counts_case,
                          dot6, image_count_case, linearise, member_counts_case, planted, pos_sum, rejected_then_kept_case,
                          solve3, solve6, track_count_case, track_sum, views_case, w3, wt6)
from test_fundamental_cpu import f32

NONE, HUBER, GEMAN_MCCLURE = 0, 1, 2
LOSSES = ((HUBER, 2.0), (GEMAN_MCCLURE, 4.0))
OUTPUTS = BC.OUTPUTS[:8] + ("obs_weight", "summary")               # in the order of the call's arguments
INT_OUTPUTS = BC.INT_OUTPUTS


def robust(case, loss, loss_scale):
    return dict(case, loss=loss, loss_scale=loss_scale)


# ---- the loss

def scale_of(case, dt):
    """(c, c2): c2 is rounded once, in the format of the run."""
    c = f32(case["loss_scale"])
    return (c, c * c) if dt is f32 else (dt(c), dt(c) * dt(c))


def loss_terms(s, loss, c, c2, dt):
    """(rho, w, sw) of the squared residuals s (m,)."""
    s = np.asarray(s, dt)
    one = np.ones(len(s), dt)
    with np.errstate(all="ignore"):
        if loss == NONE:
            return s, one, one
        if loss == HUBER:
            inl = s <= c2                                            # false for a NaN
            n = np.sqrt(s)
            w = c / n
            return (np.where(inl, s, (c + c) * n - c2).astype(dt), np.where(inl, one, w).astype(dt),
                    np.where(inl, one, np.sqrt(w)).astype(dt))
        assert loss == GEMAN_MCCLURE
        d = c2 + s
        q = c2 / d
        return ((s * c2) / d).astype(dt), (q * q).astype(dt), q.astype(dt)


def costs(P, cams, pts, loss, c, c2):
    """(in front (m,), s per member, rho per member, c_i per image, c) of a state."""
    dt = P.dt
    _, _, zc, _, _, _, ru, rv = RC.view(cams[P.img].T, P.K[P.img].T, pts[P.trk], P.x, P.y, dt)
    s = ru * ru + rv * rv
    rho = loss_terms(s, loss, c, c2, dt)[0]
    ci = np.array([pos_sum(rho[m].reshape(-1, 1), dt)[0] for m in P.of_image], dt)
    return zc > 0, s, rho, ci, cross_sum(ci, np.arange(P.n), dt)


# ---- one step

def lm_step(P, cams, pts, lam, cg_iters, dt, loss=NONE, c=None, c2=None):
    """Steps 1-5 at damping lam, as bundle_cases.lm_step, the members' values scaled by sw first: dict(fail, cams, pts
    (the trial state), iters, x, delta, lin (scaled), lin0 (as linearised), w)."""
    n, T = P.n, len(P.pts0)
    lam1 = dt(1) + lam
    front, l0 = linearise(cams[P.img], P.K[P.img], pts[P.trk], P.x, P.y, dt)
    assert front.all()
    wgt = np.ones(len(l0), dt)
    l = l0
    if loss != NONE:
        _, wgt, sw = loss_terms(l0[:, 18] * l0[:, 18] + l0[:, 19] * l0[:, 19], loss, c, c2, dt)
        l = (sw[:, None] * l0).astype(dt)
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
        cols = [lm[:, r] * lm[:, q] + lm[:, 6 + r] * lm[:, 6 + q] for r in range(6) for q in range(r, 6)]
        cols += [lm[:, r] * lm[:, 18] + lm[:, 6 + r] * lm[:, 19] for r in range(6)]
        s = pos_sum(np.concatenate([np.stack(cols, 1), w3(lm, yt[P.trk[m]])], 1), dt)
        j = 0
        for r in range(6):
            for q in range(r, 6):
                U[f, r, q] = U[f, q, r] = s[j] * lam1 if r == q else s[j]
                j += 1
        b[f] = s[21:27] - s[27:33]
    _, ok = solve6(U, b)
    fail = fail or not ok.all()
    out = dict(fail=fail, iters=0, x=np.zeros((nf, 6), dt), cams=cams, pts=pts, lin=l, lin0=l0, w=wgt)
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
    return dict(out, fail=False, iters=iters, x=x, delta=delta, cams=cams2, pts=pts2, U=U, b=b, V=V, gp=gp)


def adjust(case, dt=f32):
    """The call restated, as bundle_cases.adjust: dict(problem, cams, pts, cost (2, sums of rho), history, ci0, ci1, e
    (rho per member under the final state), s (the squared residual there), front, w (the weights there), kept, trace,
    visited: the largest s and whether every s was <= c2, over every state and trial state evaluated)."""
    P = Problem(case, dt)
    loss = case["loss"]
    c, c2 = scale_of(case, dt) if loss != NONE else (None, None)
    nan = PC.ONE_NAN if dt is f32 else dt(np.nan)
    with np.errstate(all="ignore"):
        cams, pts = P.cams0.copy(), P.pts0.copy()
        front, s, e, ci, cost = costs(P, cams, pts, loss, c, c2)
        seen = [s]
        ci0, c0 = ci, cost
        lam = dt(f32(case["lambda0"]))
        floor = dt(f32(LAMBDA_FLOOR))
        history, trace, kept_steps = [], [], 0
        for _ in range(case["num_loops"]):
            st = lm_step(P, cams, pts, lam, case["cg_iters"], dt, loss, c, c2)
            kept, cc2, why = False, nan, "singular"
            if not st["fail"]:
                act = np.nonzero(P.active)[0]
                finite = np.isfinite(st["cams"][P.free]).all() and np.isfinite(st["pts"][act]).all()
                front2, s2, e2, ci2, cc = costs(P, st["cams"], st["pts"], loss, c, c2)
                why = "not finite" if not finite else "behind"
                if finite and front2.all():
                    seen.append(s2)
                    cc2 = nan if np.isnan(cc) else cc
                    kept = bool(cc < cost)
                    why = "kept" if kept else "worse"
            trace.append(why)
            history.append((cc2, lam, int(kept), st["iters"]))
            if kept:
                cams, pts, front, s, e, ci, cost = st["cams"], st["pts"], front2, s2, e2, ci2, cc
                kept_steps += 1
                lo = lam / dt(10)
                lam = lo if lo > floor else floor
            else:
                lam = lam * dt(10)
        wgt = loss_terms(s, loss, c, c2, dt)[1]
        every = np.concatenate(seen) if seen else np.zeros(0, dt)
        inliers = bool((every <= c2).all()) if loss != NONE else True
    return dict(problem=P, cams=cams, pts=pts, cost=(c0, cost), history=history, ci0=ci0, ci1=ci, e=e, s=s, front=front,
                w=wgt, kept=kept_steps, trace=trace, visited=dict(largest=every.max() if len(every) else dt(0),
                                                                  inliers=inliers))


def pooled_rms(res):
    """The rms reprojection error over all members under the final state, in float64."""
    return float(np.sqrt(np.asarray(res["s"], np.float64).sum() / max(len(res["s"]), 1)))


def expected_bundle(case):
    """The ten outputs of the call as uint32 arrays of exactly the stated sizes (poison where the call writes nothing),
    and the restatement's own dict under 'res'."""
    res = adjust(case, f32)
    P = res["problem"]
    n, mt, mo, T, O = P.n, case["max_tracks"], case["max_obs"], P.T, P.O
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
    weight = np.full(mo, POISON_WORD, np.uint32)
    wo = np.full(O, -1.0, f32)
    wm = np.where(res["front"], res["w"], PC.ONE_NAN).astype(f32)
    wo[P.slot] = np.where(np.isnan(wm), PC.ONE_NAN, wm)
    weight[:O] = wo.view(np.uint32)
    summary = np.array([T, (P.state == ADJUSTED).sum(), len(P.slot), (P.state == FEW_OBS).sum(), P.active.sum(),
                        (P.state == HELD).sum(), res["kept"], (P.state == NO_CAMERA).sum()], np.int32)
    return dict(cam_out=cam_out.reshape(-1), points_out=points_out.reshape(-1),
                cam_obs=P.icount.astype(np.int32).view(np.uint32), cam_status=P.state.astype(np.int32).view(np.uint32),
                cam_rms=rms.reshape(-1).view(np.uint32), point_obs=point_obs, history=history,
                cost=cost.view(np.uint32), obs_weight=weight, summary=summary.view(np.uint32), res=res)


def expected_plain_with_weights(case):
    """Loss 0 from the OLD restatement (bundle_cases.expected_bundle): its nine outputs, and the weights: 1 for a member,
    -1 for any other slot below O."""
    e = BC.expected_bundle(case)
    P = e["res"]["problem"]
    weight = np.full(case["max_obs"], POISON_WORD, np.uint32)
    wo = np.full(P.O, -1.0, f32)
    wo[P.slot] = 1.0
    weight[:P.O] = wo.view(np.uint32)
    return dict(e, obs_weight=weight)


def in_place(e, case):
    """The expected outputs when d_points_out is d_points: beyond T the input stays, which is no poison."""
    T = e["res"]["problem"].T
    pts = e["points_out"].copy()
    pts[4 * T:] = np.ascontiguousarray(case["points"], f32).view(np.uint32).reshape(-1)[4 * T:]
    return dict(e, points_out=pts)


def sizes(case):
    return dict(BC.sizes(case), obs_weight=case["max_obs"])


def compare_all(got, e, what, keys=OUTPUTS):
    for k in keys:
        bad = np.nonzero(got[k] != e[k])[0]
        view = np.int32 if k in INT_OUTPUTS else f32
        assert len(bad) == 0, (what, k, "%d words differ, first %s" % (len(bad), bad[:8]), got[k][bad[:4]].view(view),
                               e[k][bad[:4]].view(view))


# ---- the hook

def hook_args(case):
    """The input arrays of a hook call, at exactly the stated sizes."""
    mt, mo = case["max_tracks"], case["max_obs"]
    return dict(offs=np.ascontiguousarray(case["track_offsets"][:mt + 1], np.int32),
                obs=np.ascontiguousarray(case["obs"][:mo]), summ=np.ascontiguousarray(case["export_summary"], np.int32),
                pts=np.ascontiguousarray(case["points"], f32).reshape(-1, 4).copy(),
                st=np.ascontiguousarray(case["point_status"], np.int32),
                cam=np.ascontiguousarray(case["cam"], f32).reshape(-1, 12).copy(),
                pair=np.ascontiguousarray(case["cam_pair"], np.int32),
                K=np.ascontiguousarray(case["intrinsics"], f32).reshape(-1, 4),
                hold=np.ascontiguousarray(case["hold"], np.int32).reshape(-1))


def hook_bundle_robust(case, in_place=False, weights=True):
    """misift_test_adjust_bundle_robust on poisoned outputs of exactly the stated sizes, as uint32 arrays; weights=False
    passes NULL for obs_weight, whose array then comes back as it was poisoned."""
    from cudasift_amd import capi
    a = hook_args(case)
    out = {k: np.full(m, POISON_WORD, np.uint32) for k, m in sizes(case).items()}
    if in_place:
        out["cam_out"], out["points_out"] = a["cam"].reshape(-1).view(np.uint32), a["pts"].reshape(-1).view(np.uint32)
    ptr = {k: out[k].ctypes.data for k in OUTPUTS}
    if not weights:
        ptr["obs_weight"] = None
    rc = capi.lib().misift_test_adjust_bundle_robust(
        case["max_tracks"], case["max_obs"], a["offs"].ctypes.data, a["obs"].ctypes.data, a["summ"].ctypes.data,
        a["pts"].ctypes.data, a["st"].ctypes.data, case["nimages"], a["cam"].ctypes.data, a["pair"].ctypes.data,
        a["K"].ctypes.data, len(a["hold"]), a["hold"].ctypes.data if len(a["hold"]) else None, case["min_views"],
        case["min_obs"], case["num_loops"], case["cg_iters"], float(case["max_error"]), float(case["lambda0"]),
        int(case["orthonormalise"]), int(case["loss"]), float(case["loss_scale"]), *[ptr[k] for k in OUTPUTS])
    assert rc == 0, rc
    return out


# ---- cases

def member_s(case):
    """The squared residual of every member under the starting state, in float32, and the Problem."""
    P = Problem(case, f32)
    with np.errstate(all="ignore"):
        return costs(P, P.cams0, P.pts0, NONE, None, None)[1], P


def huber_tie_cases(**kw):
    """A planted case and one of its members with fl(fl(sqrtf(s))^2) == s under the starting state: with c = sqrtf(s),
    c2 == s exactly, the edge of the Huber test.  dict(member, s, cases: c one ulp down, c, c one ulp up)."""
    base = planted(60, 4, 1, num_loops=3, **kw)["case"]
    s, _ = member_s(base)
    root = np.sqrt(s)
    hit = np.nonzero((root * root == s) & (s > 0))[0]
    assert len(hit), "no member with an exactly representable root"
    m = int(hit[0])
    c = root[m]
    scales = (np.nextafter(c, f32(0)), c, np.nextafter(c, f32(np.inf)))
    return dict(member=m, s=s[m], cases=[robust(base, HUBER, float(v)) for v in scales])


def every_member_an_outlier_case(loss=HUBER):
    return robust(planted(40, 4, 1, num_loops=3)["case"], loss, 1e-3)


def every_member_an_inlier_case():
    """c = 1e6: no residual of any state visited comes near it, so the call is the plain one (the second identity)."""
    return robust(planted(40, 4, 1)["case"], HUBER, 1e6)


def overflow_case(loss):
    """One observation at 1e20 px: its s overflows to +inf."""
    base = planted(40, 4, 1, num_loops=3)["case"]
    _, P = member_s(base)
    obs = base["obs"].copy()
    obs["xpos"][P.slot[len(P.slot) // 2]] = 1e20
    return robust(dict(base, obs=obs), loss, 2.0)


def displaced(case, seed, share=0.05, by=30.0):
    """`share` of the observations of a case moved by `by` px in a random direction: (case, displaced (O,))."""
    rng = np.random.default_rng(seed)
    O = RC.counts(case)[1]
    obs = case["obs"].copy()
    hit = rng.random(O) < share
    ang = rng.uniform(0, 2 * np.pi, O)
    obs["xpos"][:O] += np.where(hit, by * np.cos(ang), 0).astype(f32)
    obs["ypos"][:O] += np.where(hit, by * np.sin(ang), 0).astype(f32)
    return dict(case, obs=obs), hit


def noisy_scene(ntracks, nimages, seed, loss, loss_scale):
    """A planted scene with 0.5 px noise and 5 % of the observations displaced by 30 px, 6 steps."""
    base = planted(ntracks, nimages, seed, lengths=(3, 4, 5), noise=0.5, num_loops=6, orthonormalise=1)["case"]
    case, hit = displaced(base, seed + 1000)
    return robust(case, loss, loss_scale), hit


SCENE_KW = dict(hold=(1,), min_views=2, min_obs=6, cg_iters=10, lambda0=1e-3, orthonormalise=0, max_error=RC.INF)


def outlier_case(loss, loss_scale, num_loops=3):
    """filter_cases.outlier_scene at a size that restates in about a second: 48 tracks over 4 images, 5 % of the
    observations displaced by 30 px, 3 tracks merged with another point's: (case, the scene)."""
    sc = FC.outlier_scene(ntracks=48, nimages=4, seed=107, merged=3, drift=(0.004, 0.01), point_noise=0.01)
    return robust(dict(sc["case"], num_loops=num_loops, **SCENE_KW), loss, loss_scale), sc


def cpu_cases():
    """name -> case: every new case, which test_bundle_robust_cpu.py holds the hook to and test_gpu_bundle_robust.py the
    device."""
    out = {}
    for name, case in zip(("tie, c down", "tie", "tie, c up"), huber_tie_cases()["cases"]):
        out[name] = case
    out["inliers"] = every_member_an_inlier_case()
    for loss, c in LOSSES:
        tag = "huber" if loss == HUBER else "geman-mcclure"
        out["outliers only, " + tag] = every_member_an_outlier_case(loss)
        out["overflow, " + tag] = overflow_case(loss)
        out["rejected then kept, " + tag] = robust(rejected_then_kept_case(), loss, c)
        out["behind, " + tag] = robust(behind_trial_case(), loss, c)
        out["outlier scene, " + tag] = outlier_case(loss, c)[0]
    return out

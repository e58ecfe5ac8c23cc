"""misift_filter_tracks_batch: expected_filter, the numpy restatement of the definition in include/misift.h rule by rule,
the wrapper of the library's host hook, and the cases of its tests (test_filter_cpu.py pins the restatement to the hook
and to float64, test_gpu_filter.py holds the device to it byte for byte).  A case is a refine case (refine_cases) with
the call's further arguments: max_error, max_cos, min_views, unique_frames.  The restatement takes its number format as
an argument: with float32 every operation is rounded as the library rounds it, with float64 the same rules are the
yardstick.  No GPU in here, and cudasift_amd.capi is imported inside functions only."""
import numpy as np

import refine_cases as RC
import triangulate_cases as TC
from test_fundamental_cpu import f32

NO_OWNER, BAD_POINT, NOT_USABLE, BEHIND, ERROR, DUPLICATE, FEW_VIEWS, NARROW = -1, -2, -3, -4, -5, -6, -7, -8
INF = float("inf")
POISON_WORD = TC.POISON_WORD
OUTPUTS = ("track_offsets_out", "obs_out", "export_summary_out", "points_out", "point_views_out", "point_status_out",
           "track_map", "obs_map", "summary")
FLOAT_OUTPUTS = ("points_out",)
ARGS = ("max_error", "max_cos", "min_views", "unique_frames")


# ---- the definition restated

def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def slots(case, dt=f32):
    """Rule 1 for every slot o < O: dict(code (0 for a survivor), owner, e2, ray (O, 3), p, q (the projections))."""
    T, O = RC.counts(case)
    _, owner = RC.candidate_keys(case)
    n = case["nimages"]
    obs = case["obs"][:O]
    pts = np.asarray(case["points"], f32).reshape(-1, 4)
    st = np.asarray(case["point_status"], np.int32)
    cam = np.ascontiguousarray(case["cam"], f32).reshape(-1, 12)
    pair = np.asarray(case["cam_pair"], np.int32)
    K = np.asarray(case["intrinsics"], f32).reshape(-1, 4)
    oc = np.maximum(owner, 0)
    X32 = pts[oc, :3]
    bad = (st[oc] != 0) | ~np.isfinite(X32).all(1)
    frame = obs["frame"].astype(np.int64)
    inr = (frame >= 0) & (frame < n)
    fc = np.where(inr, frame, 0)
    x32, y32 = obs["xpos"], obs["ypos"]
    usable = inr & (pair[fc] != RC.UNSET) & np.isfinite(cam[fc]).all(1) & np.isfinite(x32) & np.isfinite(y32)
    me = f32(case["max_error"])
    E2 = me * me if dt is f32 else dt(me) * dt(me)
    with np.errstate(all="ignore"):
        c, k, X = cam[fc].astype(dt).T, K[fc].astype(dt).T, X32.astype(dt)
        _, _, zc, _, a, b, ru, rv = RC.view(c, k, X, x32.astype(dt), y32.astype(dt), dt)
        e2 = ru * ru + rv * rv
        centre = [-((c[j] * c[9] + c[3 + j] * c[10]) + c[6 + j] * c[11]) for j in range(3)]
        d = [X[:, j] - centre[j] for j in range(3)]
        nrm = np.sqrt(dot3(d, d))
        ray = np.stack([d[j] / nrm for j in range(3)], 1)
        code = np.zeros(O, np.int64)
        for reason, hit in ((ERROR, ~(e2 < E2)), (BEHIND, ~(zc > 0)), (NOT_USABLE, ~usable), (BAD_POINT, bad),
                            (NO_OWNER, owner < 0)):
            code[hit] = reason                                   # the last one written is the first that applies
        p, q = k[0] * a + k[2], k[1] * b + k[3]
    return dict(code=code, owner=owner, e2=e2, ray=ray, frame=frame, p=p, q=q, E2=E2)


def decide(case, dt=f32):
    """Rules 1-4 as decisions: dict(code (O: the reason, or 0 for a kept view of a surviving track), track (T: the
    reason, or 0), kept [(t, slots, m, s)] for the surviving tracks in ascending t, slots (rule 1's dict))."""
    T, O = RC.counts(case)
    S = slots(case, dt)
    code, owner, e2, ray, frame = S["code"].copy(), S["owner"], S["e2"], S["ray"], S["frame"]
    offs = np.asarray(case["track_offsets"], np.int64)
    pts = np.asarray(case["points"], f32).reshape(-1, 4)
    st = np.asarray(case["point_status"], np.int32)
    max_cos = dt(f32(case["max_cos"]))
    track = np.zeros(T, np.int64)
    kept = []
    with np.errstate(all="ignore"):
        for t in range(T):
            off, end = offs[t], offs[t + 1]
            if not 0 <= off <= end <= O:
                track[t] = NO_OWNER
                continue
            if st[t] != 0 or not np.isfinite(pts[t, :3]).all():
                track[t] = BAD_POINT
                continue
            o = np.arange(off, end)
            o = o[(owner[o] == t) & (code[o] == 0)]
            if case["unique_frames"] and len(o) > 1:
                same = (frame[o][:, None] == frame[o][None, :]) & (o[:, None] != o[None, :])
                better = (e2[o][None, :] < e2[o][:, None]) | ((e2[o][None, :] == e2[o][:, None]) & (o[None, :] < o[:, None]))
                loses = (same & better).any(1)
                code[o[loses]] = DUPLICATE
                o = o[~loses]
            m = len(o)
            if m < case["min_views"]:
                track[t] = FEW_VIEWS
            elif max_cos < np.inf:
                u = ray[o].T
                G = (u[0][:, None] * u[0][None, :] + u[1][:, None] * u[1][None, :]) + u[2][:, None] * u[2][None, :]
                if not (G[np.triu_indices(m, 1)] < max_cos).any():
                    track[t] = NARROW
            if track[t]:
                code[o] = track[t]
                continue
            s = np.add.accumulate(e2[o], dtype=dt)[-1]           # from +0, one term at a time, in ascending slot
            kept.append((t, o, m, s))
    return dict(code=code, track=track, kept=kept, slots=S)


def sizes(case):
    mt, mo = case["max_tracks"], case["max_obs"]
    return dict(track_offsets_out=mt + 1, obs_out=4 * mo, export_summary_out=8, points_out=4 * mt, point_views_out=mt,
                point_status_out=mt, track_map=mt, obs_map=mo, summary=8)


def expected_filter(case):
    """The nine outputs of the call as uint32 arrays of exactly the stated sizes (poison where the call writes nothing),
    and the decisions under 'res'."""
    res = decide(case, f32)
    T, O = RC.counts(case)
    out = {k: np.full(m, POISON_WORD, np.uint32) for k, m in sizes(case).items()}
    obs = np.ascontiguousarray(case["obs"][:case["max_obs"]]).view(np.uint32).reshape(-1, 4)
    pts = np.ascontiguousarray(case["points"], f32).reshape(-1, 4).view(np.uint32)
    obs_out, points_out = out["obs_out"].reshape(-1, 4), out["points_out"].reshape(-1, 4)
    code = res["code"].copy()
    track = res["track"].copy()
    at = 0
    out["track_offsets_out"][0] = 0
    with np.errstate(all="ignore"):
        for tn, (t, o, m, s) in enumerate(res["kept"]):
            obs_out[at:at + m] = obs[o]
            code[o] = at + np.arange(m)
            points_out[tn, :3] = pts[t, :3]
            points_out[tn, 3] = np.array([np.sqrt(s / f32(m))], f32).view(np.uint32)[0]
            out["point_views_out"][tn] = m
            out["point_status_out"][tn] = 0
            track[t] = tn
            at += m
            out["track_offsets_out"][tn + 1] = at
    Tn = len(res["kept"])
    out["track_map"][:T] = track.astype(np.int32).view(np.uint32)
    out["obs_map"][:O] = code.astype(np.int32).view(np.uint32)
    longest = max([m for _, _, m, _ in res["kept"]] + [0])
    out["export_summary_out"][:] = np.array([Tn, at, Tn, at, longest, 0, 0, 0], np.int32).view(np.uint32)
    c1 = res["slots"]["code"]                                    # -4 and -5 are rule 1's; -6 is rule 2's
    out["summary"][:] = np.array([Tn, at, (c1 == BEHIND).sum(), (c1 == ERROR).sum(), (res["code"] == DUPLICATE).sum(),
                                  (res["track"] == FEW_VIEWS).sum(), (res["track"] == NARROW).sum(),
                                  ((c1 < 0) & (c1 >= NOT_USABLE)).sum()], np.int32).view(np.uint32)
    return dict(out, res=res)


def compare(got, e, what, keys=OUTPUTS):
    for k in keys:
        bad = np.nonzero(got[k] != e[k])[0]
        view = f32 if k in FLOAT_OUTPUTS else np.int32
        assert len(bad) == 0, (what, k, "%d words differ, first %s" % (len(bad), bad[:8]), got[k][bad[:4]].view(view),
                               e[k][bad[:4]].view(view))


def reasons(e):
    """The reason codes a case gives rise to, of slots and of tracks."""
    res = e["res"]
    return set(int(c) for c in np.unique(res["code"]) if c < 0), set(int(c) for c in np.unique(res["track"]) if c < 0)


def filtered_case(case, out):
    """The case a later call sees: the filter's outputs (uint32 arrays, as expected_filter or the device give them) in
    place of the lists, the points and their status; capacities, cameras and arguments stay."""
    mt, mo = case["max_tracks"], case["max_obs"]
    return dict(case, track_offsets=out["track_offsets_out"].view(np.int32).copy(),
                obs=out["obs_out"].view(TC.OBS_DTYPE).copy(), export_summary=out["export_summary_out"].view(np.int32).copy(),
                points=out["points_out"].view(f32).reshape(mt, 4).copy(),
                point_status=out["point_status_out"].view(np.int32).copy())


# ---- the hook

def stage():
    from cudasift_amd import capi
    return int(capi.lib().misift_test_filter_stage())


def inputs(case):
    """The inputs at exactly the sizes the call states."""
    mt, mo = case["max_tracks"], case["max_obs"]
    ins = dict(track_offsets=np.ascontiguousarray(case["track_offsets"][:mt + 1], np.int32),
               obs=np.ascontiguousarray(case["obs"][:mo]), export_summary=np.ascontiguousarray(case["export_summary"], np.int32),
               points=np.ascontiguousarray(case["points"], f32).reshape(-1, 4),
               point_status=np.ascontiguousarray(case["point_status"], np.int32),
               cam=np.ascontiguousarray(case["cam"], f32).reshape(-1, 12),
               cam_pair=np.ascontiguousarray(case["cam_pair"], np.int32))
    assert len(ins["track_offsets"]) == mt + 1 and len(ins["obs"]) == mo and len(ins["cam"]) == case["nimages"]
    assert len(ins["points"]) == mt == len(ins["point_status"])
    return ins


def hook_filter(case, obs_map=True):
    """misift_test_filter_tracks on poisoned outputs of exactly the stated sizes, as uint32 arrays."""
    from cudasift_amd import capi
    ins = inputs(case)
    K = np.ascontiguousarray(case["intrinsics"], f32).reshape(-1, 4)
    out = {k: np.full(m, POISON_WORD, np.uint32) for k, m in sizes(case).items()}
    ptr = {k: out[k].ctypes.data for k in OUTPUTS}
    if not obs_map:
        ptr["obs_map"] = None
    rc = capi.lib().misift_test_filter_tracks(
        case["max_tracks"], case["max_obs"], ins["track_offsets"].ctypes.data, ins["obs"].ctypes.data,
        ins["export_summary"].ctypes.data, ins["points"].ctypes.data, ins["point_status"].ctypes.data, case["nimages"],
        ins["cam"].ctypes.data, ins["cam_pair"].ctypes.data, K.ctypes.data, float(case["max_error"]),
        float(case["max_cos"]), int(case["min_views"]), int(case["unique_frames"]), *[ptr[k] for k in OUTPUTS])
    assert rc == 0, rc
    return out


# ---- cases

def filter_case(refine, max_error=INF, max_cos=INF, min_views=2, unique_frames=1):
    return dict(refine, max_error=max_error, max_cos=max_cos, min_views=min_views, unique_frames=unique_frames)


def variant(case, **kw):
    return dict(case, **kw)


def cycled(m, nimages, first=0):
    """The frames of a track of m views that cycles through the images: beyond nimages views it holds duplicates."""
    return [(first + i) % nimages for i in range(m)]


def lengths_case(lengths, nimages=8, seed=90, noise=0.5, **kw):
    """One track per entry of `lengths` with that many views, cycling through the images; the cameras as planted."""
    frames_of = [cycled(m, nimages, t) for t, m in enumerate(lengths)]
    sc = RC.scene(frames_of, nimages, seed, noise=noise, angle=0.0, shift=0.0, step=min(0.4, 3.2 / nimages))
    return filter_case(sc["case"], **kw)


def two_view_case(T, seed=91, **kw):
    """T tracks of two views each over four images."""
    return lengths_case([2] * T, nimages=4, seed=seed, **kw)


def view_counts_case(**kw):
    """Tracks of 1, 2, 3, 63, 64, 65, 129 and 301 views and one longer than the staging, over 8 images (so the long ones
    hold up to 40 views of a frame), and the same lengths over 400 images (no duplicate at all)."""
    L = [1, 2, 3, 63, 64, 65, 129, 301, stage() + 70]
    return lengths_case(L, 8, 92, **kw), lengths_case(L, 400, 93, **kw)


def residual_at(case, o, du, dv):
    """The case with the position of slot o moved to its projection + (du, dv), added in fp32."""
    S = slots(case)
    obs = case["obs"].copy()
    obs["xpos"][o], obs["ypos"][o] = f32(S["p"][o]) + f32(du), f32(S["q"][o]) + f32(dv)
    return variant(case, obs=obs)


def duplicates_case(**kw):
    """Track 0: two views of frame 1; track 1: three of frame 2; track 2: two of frame 3 at identical positions (a tie,
    the lower slot stays); track 3: 70 views over 72 images with slots 63 and 64 of one frame; track 4: clean."""
    f3 = list(range(70))
    f3[64] = f3[63]
    frames_of = [[0, 1, 1, 2], [2, 0, 2, 1, 2], [3, 3, 0, 1], f3, [0, 1, 2, 3]]
    sc = RC.scene(frames_of, 72, 94, noise=0.5, angle=0.0, shift=0.0, step=0.1)
    case = filter_case(sc["case"], **kw)
    obs = case["obs"].copy()
    offs = case["track_offsets"]
    a = offs[2]
    obs["xpos"][a + 1], obs["ypos"][a + 1] = obs["xpos"][a], obs["ypos"][a]
    return variant(case, obs=obs)


def error_gate_case(max_error=2.0):
    """Slot 1 of track 0 sits exactly max_error px from its projection: e2 == E2, which is not below it."""
    case = lengths_case([3, 3, 4], 4, 95, noise=0.25, max_error=max_error)
    return residual_at(case, int(case["track_offsets"][0]) + 1, max_error, 0.0)


def angle_gate_case():
    """Two-view tracks; max_cos is exactly u_0 . u_1 of track 2, so that track is dropped and one ulp more keeps it."""
    case = lengths_case([2, 2, 2, 3], 4, 96)
    S = slots(case)
    o = int(case["track_offsets"][2])
    u = S["ray"][o:o + 2].T
    cos = f32(dot3(u[:, 0], u[:, 1]))
    return variant(case, max_cos=float(cos)), variant(case, max_cos=float(np.nextafter(cos, f32(2))))


def min_views_cases():
    """Tracks of 1 to 4 views under min_views 2 and 3: m at min_views - 1, equal to it and + 1."""
    return [lengths_case([1, 2, 3, 4, 2, 3], 6, 97, min_views=mv) for mv in (2, 3)]


def hostile_case(**kw):
    """refine_cases.hostile_case (hostile frames, NaN and inf in cameras, points and positions, points of every failed
    status, points behind a camera, an image without a camera) and a point on a camera centre."""
    case = dict(RC.hostile_case())
    pts = case["points"].copy()
    t = 30
    f = int(case["obs"]["frame"][case["track_offsets"][t]])
    c = np.asarray(case["cam"], f32)[f]
    pts[t, :3] = [-((c[j] * c[9] + c[3 + j] * c[10]) + c[6 + j] * c[11]) for j in range(3)]
    case["points"] = pts
    return filter_case(case, **kw)


def bad_offsets_case(**kw):
    return filter_case(RC.bad_offsets_case(), **kw)


def device_counts_case(T, O, **kw):
    base = filter_case(RC.spread_case(513), **kw)
    assert (base["max_tracks"], base["max_obs"]) == (171, 513)
    return RC.with_counts(base, T, O)


DEVICE_COUNTS = ((63, 513), (171, 200), (300, 10 ** 9), (2 ** 31 - 1, 2 ** 31 - 1), (-1, 513), (171, -5), (171, 256),
                 (-2 ** 31, -2 ** 31))
TRACK_COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 257)
TILE_COUNTS = (2047, 2048, 2049, 4097)


def track_count_case(T, **kw):
    """T tracks of two, three and four views over six images."""
    return lengths_case([(2, 3, 4)[t % 3] for t in range(T)], 6, 98, **kw)


_SCENES = {}


def outlier_scene(ntracks=240, nimages=8, seed=99, share=0.05, merged=12, noise=0.5, drift=(0.0, 0.0), point_noise=0.0,
                  **kw):
    """A planted scene with `noise` px on every position in which `share` of the observations is displaced by 30 px and
    `merged` tracks are each joined with their successor (another point), so that they hold duplicate frames.  The
    cameras are the planted ones, or drifted by up to drift[0] rad and drift[1] units; the points are the planted ones
    moved by point_noise units.  dict(case, clean (O: the observation is neither displaced nor foreign to its track),
    foreign, displaced)."""
    key = (ntracks, nimages, seed, share, merged, noise, drift, point_noise, tuple(sorted(kw.items())))
    if key in _SCENES:
        return _SCENES[key]
    rng = np.random.default_rng(seed)
    frames_of = list(RC.runs(ntracks, nimages, seed, lengths=(3, 4, 5, 6)))
    sc = RC.scene(frames_of, nimages, seed, noise=noise, angle=drift[0], shift=drift[1], point_noise=point_noise,
                  step=0.4)
    case = dict(sc["case"])
    T, O = RC.counts(case)
    obs = case["obs"].copy()
    displaced = rng.random(O) < share
    ang = rng.uniform(0, 2 * np.pi, O)
    obs["xpos"][:O] += np.where(displaced, 30 * np.cos(ang), 0).astype(f32)
    obs["ypos"][:O] += np.where(displaced, 30 * np.sin(ang), 0).astype(f32)
    offs = case["track_offsets"][:T + 1].astype(np.int64)
    join = np.sort(rng.choice(np.arange(0, T - 1, 2), merged, replace=False))
    foreign = np.zeros(O, bool)
    for t in join:
        foreign[offs[t + 1]:offs[t + 2]] = True
    keep = np.ones(T + 1, bool)
    keep[join + 1] = False                                       # the boundary between t and t + 1 goes
    new_offs = offs[keep]
    Tn = len(new_offs) - 1
    mt = case["max_tracks"]
    offs_out = np.full(mt + 1, POISON_WORD, np.uint32).view(np.int32)
    offs_out[:Tn + 1] = new_offs
    pts = np.zeros((mt, 4), f32)
    pts[:Tn] = case["points"][:T][keep[:T]]
    summ = case["export_summary"].copy()
    summ[0] = summ[2] = Tn
    case.update(obs=obs, track_offsets=offs_out, points=pts, export_summary=summ)
    out = dict(case=filter_case(case, **kw), clean=~displaced & ~foreign, foreign=foreign, displaced=displaced,
               true=sc["true"])
    _SCENES[key] = out
    return out


def cpu_cases():
    """name -> case: every case of test_gpu_filter.py, which test_filter_cpu.py holds the hook to."""
    out = {}
    for T in TRACK_COUNTS + TILE_COUNTS:
        out["T %d" % T] = two_view_case(T) if T in TILE_COUNTS else track_count_case(T, max_error=1.5)
    for T, O in DEVICE_COUNTS:
        out["counts %d %d" % (T, O)] = device_counts_case(T, O)
    for uf in (0, 1):
        few, many = view_counts_case(unique_frames=uf, max_error=1.2)
        out["views over 8 images, unique %d" % uf] = few
        out["views over 400 images, unique %d" % uf] = many
        out["duplicates, unique %d" % uf] = duplicates_case(unique_frames=uf)
    out["e2 == E2"] = error_gate_case()
    out["e2 < E2"] = variant(error_gate_case(), max_error=float(np.nextafter(f32(2), f32(3))))
    out["dot == max_cos"], out["dot < max_cos"] = angle_gate_case()
    out["max_cos 1"] = lengths_case([2, 3, 4], 4, 96, max_cos=1.0)
    out["max_cos finite"] = lengths_case([2, 3, 4, 8] * 6, 8, 100, max_cos=0.998, max_error=3.0)
    out["min_views 2"], out["min_views 3"] = min_views_cases()
    out["hostile"] = hostile_case()
    out["hostile gated"] = hostile_case(max_error=8.0, max_cos=0.99999, min_views=3)
    out["bad offsets"] = bad_offsets_case()
    out["bad offsets gated"] = bad_offsets_case(max_error=1.0, max_cos=0.9999)
    out["every track dropped"] = lengths_case([2, 3, 4, 5], 6, 101, max_error=1e-6)
    out["every track kept"] = lengths_case([2, 3, 4, 5], 6, 101, noise=0.0, max_error=0.5)
    out["outliers"] = outlier_scene(max_error=3.0)["case"]
    out["outliers, no gate"] = outlier_scene()["case"]
    out["outliers, angle"] = outlier_scene(max_error=3.0, max_cos=0.9985)["case"]
    return out

"""misift_filter_tracks_batch without a GPU: the numpy restatement of the header (filter_cases.py) against the library's
host hook, which compiles the rules the kernels compile (filter_core.hpp), byte for byte on every case the device test
runs; the restatement in float32 against itself in float64; what each case is built to hit; idempotence and the
"no gate" property; and the loop adjust -> filter -> adjust in the restatements."""
import numpy as np
import pytest

import bundle_cases as BC
import filter_cases as FC
import refine_cases as RC
from test_fundamental_cpu import f32

MISIFT_EINVAL = -1


def test_library_exports_the_call_and_the_hook():
    """Fails without the feature: the symbols, their rows in capi.SIGNATURES, the binding, and every argument error that
    needs no device."""
    from cudasift_amd import capi
    L = capi.lib()
    for name in ("misift_filter_tracks_batch", "misift_test_filter_tracks", "misift_test_filter_stage"):
        assert name in capi.SIGNATURES and hasattr(L, name), name
    assert callable(getattr(capi.Context, "filter_tracks_batch"))
    assert len(capi.SIGNATURES["misift_filter_tracks_batch"][1]) == 25
    assert FC.stage() >= 64 and FC.stage() % 64 == 0
    case = FC.lengths_case([2, 3], 4, 96)
    ins = FC.inputs(case)
    K = np.ascontiguousarray(case["intrinsics"], f32)
    out = {k: np.full(m, FC.POISON_WORD, np.uint32) for k, m in FC.sizes(case).items()}
    good = dict(max_tracks=case["max_tracks"], max_obs=case["max_obs"], track_offsets=ins["track_offsets"].ctypes.data,
                obs=ins["obs"].ctypes.data, export_summary=ins["export_summary"].ctypes.data,
                points=ins["points"].ctypes.data, point_status=ins["point_status"].ctypes.data, nimages=case["nimages"],
                cam=ins["cam"].ctypes.data, cam_pair=ins["cam_pair"].ctypes.data, intrinsics=K.ctypes.data,
                max_error=np.inf, max_cos=np.inf, min_views=2, unique_frames=1,
                **{k: out[k].ctypes.data for k in FC.OUTPUTS})
    # a NULL context is refused before anything else is looked at
    assert L.misift_filter_tracks_batch(None, *[good[k] for k in good]) == MISIFT_EINVAL

    def hook(**kw):
        a = dict(good, **kw)
        return L.misift_test_filter_tracks(*[a[k] for k in good])

    bad = [dict(max_tracks=0), dict(max_tracks=-1), dict(max_obs=0), dict(nimages=0), dict(min_views=1), dict(min_views=0),
           dict(unique_frames=2), dict(unique_frames=-1), dict(max_error=np.nan), dict(max_error=0.0),
           dict(max_error=-1.0), dict(max_cos=np.nan)]
    pointers = ("track_offsets", "obs", "export_summary", "points", "point_status", "cam", "cam_pair", "intrinsics")
    bad += [{k: None} for k in pointers + FC.OUTPUTS if k != "obs_map"]
    for kw in bad:
        assert hook(**kw) == MISIFT_EINVAL, kw
    for k in FC.OUTPUTS:
        assert (out[k] == FC.POISON_WORD).all(), k
    assert hook() == 0 and hook(obs_map=None) == 0 and hook(max_cos=-np.inf) == 0 and hook(max_error=np.inf) == 0


_CASES = {}


def _cases():
    if not _CASES:
        _CASES.update(FC.cpu_cases())
    return _CASES


CASE_NAMES = (["T %d" % T for T in FC.TRACK_COUNTS + FC.TILE_COUNTS] + ["counts %d %d" % c for c in FC.DEVICE_COUNTS] +
              ["%s, unique %d" % (n, u) for u in (0, 1) for n in ("views over 8 images", "views over 400 images",
                                                                  "duplicates")] +
              ["e2 == E2", "e2 < E2", "dot == max_cos", "dot < max_cos", "max_cos 1", "max_cos finite", "min_views 2",
               "min_views 3", "hostile", "hostile gated", "bad offsets", "bad offsets gated", "every track dropped",
               "every track kept", "outliers", "outliers, no gate", "outliers, angle"])


def test_case_names():
    assert sorted(CASE_NAMES) == sorted(_cases())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_equals_the_hook(name):
    case = _cases()[name]
    e = FC.expected_filter(case)
    FC.compare(FC.hook_filter(case), e, name)
    if name in ("hostile gated", "duplicates, unique 1"):
        got = FC.hook_filter(case, obs_map=False)
        assert (got["obs_map"] == FC.POISON_WORD).all()
        FC.compare(got, e, name + ", no obs_map", [k for k in FC.OUTPUTS if k != "obs_map"])


def _summary(name):
    e = FC.expected_filter(_cases()[name])
    return e, e["summary"].view(np.int32), FC.reasons(e)


def test_what_the_cases_are_built_to_hit():
    C = _cases()
    for T in FC.TRACK_COUNTS + FC.TILE_COUNTS:
        assert RC.counts(C["T %d" % T])[0] == T
        e, s, _ = _summary("T %d" % T)
        assert s[0] >= T - 1 and (T < 2 or s[0] > 0)
    for T in FC.TILE_COUNTS:
        assert _summary("T %d" % T)[1][:2].tolist() == [T, 2 * T]
    # counts from the device: clamped, cut, and a track that ends beyond O is not valid
    for (T, O), want in zip(FC.DEVICE_COUNTS, (63, 171, 171, 171, 0, 171, 171, 0)):
        case = C["counts %d %d" % (T, O)]
        assert RC.counts(case)[0] == want
    assert _summary("counts 63 513")[2][0] >= {FC.NO_OWNER} and FC.NO_OWNER in _summary("counts 171 200")[2][1]
    assert _summary("counts 300 1000000000")[1][0] > 100
    # the view counts: 1, 2, 3, 63, 64, 65, 129, 301 and one beyond the staging
    st = FC.stage()
    for name in ("views over 8 images", "views over 400 images"):
        for u in (0, 1):
            case = C["%s, unique %d" % (name, u)]
            assert np.diff(case["track_offsets"][:10]).tolist() == [1, 2, 3, 63, 64, 65, 129, 301, st + 70]
    e, s, (slots, tracks) = _summary("views over 8 images, unique 1")
    assert s[4] > 700 and FC.DUPLICATE in slots and e["export_summary_out"].view(np.int32)[4] == 8
    e, s, _ = _summary("views over 400 images, unique 1")
    assert s[4] == 0 and e["export_summary_out"].view(np.int32)[4] > st
    e, s, _ = _summary("views over 8 images, unique 0")
    assert s[4] == 0 and e["export_summary_out"].view(np.int32)[4] > st
    # duplicates: 2 and 3 views of a frame, a tie decided by the slot, slots 63 and 64
    case = C["duplicates, unique 1"]
    e, s, _ = _summary("duplicates, unique 1")
    code, offs = e["res"]["code"], case["track_offsets"]
    assert s[4] == 5 and _summary("duplicates, unique 0")[1][4] == 0
    assert (code[offs[0]:offs[1]] == FC.DUPLICATE).sum() == 1 and (code[offs[1]:offs[2]] == FC.DUPLICATE).sum() == 2
    S = e["res"]["slots"]
    assert S["e2"][offs[2]] == S["e2"][offs[2] + 1] and code[offs[2]] == 0 and code[offs[2] + 1] == FC.DUPLICATE
    assert sorted(code[offs[3] + 63:offs[3] + 65].tolist()) == [FC.DUPLICATE, 0]
    # the gates at equality
    case = C["e2 == E2"]
    e, s, _ = _summary("e2 == E2")
    o = int(case["track_offsets"][0]) + 1
    assert e["res"]["slots"]["e2"][o] == e["res"]["slots"]["E2"] == f32(4) and e["res"]["code"][o] == FC.ERROR
    assert s[3] == 1 and _summary("e2 < E2")[1][3] == 0
    e, s, _ = _summary("dot == max_cos")
    assert e["res"]["track"][2] == FC.NARROW and _summary("dot < max_cos")[0]["res"]["track"][2] == 0
    assert _summary("max_cos 1")[1][6] == 0
    e, s, (slots, tracks) = _summary("max_cos finite")
    assert s[6] > 0 and s[0] > 0 and FC.NARROW in slots
    assert _summary("min_views 2")[1][[0, 5]].tolist() == [5, 1] and _summary("min_views 3")[1][[0, 5]].tolist() == [3, 3]
    # hostile inputs: every reason of rule 1, a NaN ray from the point on a camera centre
    e, s, (slots, tracks) = _summary("hostile")
    assert {FC.BAD_POINT, FC.NOT_USABLE, FC.BEHIND, FC.FEW_VIEWS} <= slots and {FC.BAD_POINT, FC.FEW_VIEWS} <= tracks
    e, s, (slots, tracks) = _summary("hostile gated")
    assert FC.ERROR in slots and s[0] > 0
    case = C["hostile"]
    assert np.isnan(e["res"]["slots"]["ray"][case["track_offsets"][30]]).all()
    e, s, (slots, tracks) = _summary("bad offsets")
    assert FC.NO_OWNER in slots and FC.NO_OWNER in tracks and s[0] > 0
    assert _summary("every track dropped")[1][:2].tolist() == [0, 0] and _summary("every track dropped")[1][5] == 4
    assert _summary("every track kept")[1].tolist() == [4, 14, 0, 0, 0, 0, 0, 0]
    e, s, (slots, tracks) = _summary("outliers, no gate")
    assert FC.DUPLICATE in slots and s[3] == 0
    e, s, (slots, tracks) = _summary("outliers, angle")
    assert {FC.ERROR, FC.NARROW} <= slots and s[0] > 50


def test_float32_decisions_against_float64():
    """The planted scene with 0.5 px of noise, 5 % of the observations displaced by 30 px and 12 tracks merged with
    another point's.  Rule 1 decides alike in both formats but for observations whose float64 e2 lies within a
    relative 1e-3 of E2, and the whole call decides alike on every track that holds no such observation; that band holds
    under 1 % of the observations."""
    sc = FC.outlier_scene(max_error=3.0, max_cos=0.9985)
    case = sc["case"]
    T, O = RC.counts(case)
    d32, d64 = FC.decide(case, f32), FC.decide(case, np.float64)
    e2, E2 = d64["slots"]["e2"], d64["slots"]["E2"]
    band = np.abs(e2 - E2) <= 1e-3 * E2
    print("band: %d of %d observations" % (band.sum(), O))
    assert band.sum() < 0.01 * O
    assert (d32["slots"]["code"][~band] == d64["slots"]["code"][~band]).all()
    owner = d64["slots"]["owner"]
    touched = np.zeros(T, bool)
    touched[owner[band & (owner >= 0)]] = True
    clear = ~touched[np.maximum(owner, 0)]
    assert (d32["code"][clear] == d64["code"][clear]).all() and (d32["track"][~touched] == d64["track"][~touched]).all()
    # the scene does what it is meant to: the displaced and the foreign observations go, nearly all clean ones stay
    gone = d64["slots"]["code"] == FC.ERROR
    assert gone[sc["displaced"]].all() and gone[sc["foreign"]].mean() > 0.9 and gone[sc["clean"]].mean() < 0.01
    assert np.allclose(d32["slots"]["e2"][~gone], e2[~gone], rtol=1e-2, atol=1e-4)


@pytest.mark.parametrize("name", ["views over 8 images, unique 1", "duplicates, unique 1", "hostile gated", "bad offsets",
                                  "outliers, angle", "max_cos finite", "min_views 3", "T 257"])
def test_idempotent(name):
    """Run on its own outputs with the same arguments the call keeps everything, in the restatement and in the hook."""
    case = _cases()[name]
    e = FC.expected_filter(case)
    Tn, On = e["summary"].view(np.int32)[:2]
    again = FC.filtered_case(case, e)
    for got in (FC.expected_filter(again), FC.hook_filter(again)):
        assert got["summary"].view(np.int32).tolist() == [Tn, On, 0, 0, 0, 0, 0, 0]
        for k, n in (("track_offsets_out", Tn + 1), ("obs_out", 4 * On), ("points_out", 4 * Tn), ("point_views_out", Tn),
                     ("point_status_out", Tn)):
            assert got[k][:n].tobytes() == e[k][:n].tobytes(), k
        assert got["export_summary_out"].tobytes() == e["export_summary_out"].tobytes()
        assert (got["track_map"][:Tn].view(np.int32) == np.arange(Tn)).all()
        assert (got["obs_map"][:On].view(np.int32) == np.arange(On)).all()


def test_without_a_gate_it_drops_what_triangulate_did_not_use():
    """max_error = max_cos = +inf, unique_frames = 0, min_views = 2 on triangulate's own output: the tracks without
    status 0 go, and the views triangulate did not use (its d_obs_error is the NaN there)."""
    base = RC.hostile_case()
    pts, st, err = RC.triangulate_under(base, base["cam"])
    case = FC.filter_case(dict(base, points=pts, point_status=st), unique_frames=0)
    T, O = RC.counts(case)
    e = FC.expected_filter(case)
    FC.compare(FC.hook_filter(case), e, "no gate")
    track, code = e["res"]["track"], e["res"]["code"]
    assert ((track == 0) == (st[:T] == 0)).all() and 0 < (st[:T] != 0).sum() < T
    assert ((code == 0) == np.isfinite(err[:O])).all()
    s = e["summary"].view(np.int32)
    assert s[2:7].tolist() == [0, 0, 0, 0, 0] and s[7] == (code < 0).sum() > 0


# adjust -> filter -> adjust against adjust -> adjust, three loops each: the pooled rms in px over the planted-clean
# observations of the tracks the filter keeps (the same observations in both runs, whether the filter kept them or
# not), under each run's final cameras and points, and the share of clean observations the filter removed.  The scene:
# 152 tracks over 6 images, 0.5 px of noise, 5 % of the observations displaced by 30 px, 8 tracks merged with another
# point's, the gate at 10 px
MEASURED = {"adjust, adjust": 4.6235, "adjust, filter, adjust": 0.8214, "clean removed": 0.1068}


def _clean_rms(case, cam, pts, slots, owner):
    c = np.asarray(cam, np.float64).reshape(-1, 12)[case["obs"]["frame"][slots]].T
    k = np.asarray(case["intrinsics"], np.float64)[case["obs"]["frame"][slots]].T
    X = np.asarray(pts, np.float64).reshape(-1, 4)[owner, :3]
    _, _, zc, _, _, _, ru, rv = RC.view(c, k, X, case["obs"]["xpos"][slots].astype(np.float64),
                                        case["obs"]["ypos"][slots].astype(np.float64), np.float64)
    assert (zc > 0).all()
    return float(np.sqrt((ru * ru + rv * rv).mean()))


def test_adjust_filter_adjust_against_adjust_adjust():
    sc = FC.outlier_scene(ntracks=160, nimages=6, seed=103, merged=8, drift=(0.004, 0.01), point_noise=0.01,
                          max_error=10.0)
    case = sc["case"]
    T, O = RC.counts(case)
    mt = case["max_tracks"]
    kw = dict(hold=(1,), min_views=2, min_obs=6, cg_iters=10, lambda0=1e-3, orthonormalise=0, max_error=RC.INF)

    def adjusted(c, loops):
        e = BC.expected_bundle(dict(c, num_loops=loops, **kw))
        pts = e["points_out"].view(f32).reshape(mt, 4).copy()
        pts[RC.counts(c)[0]:] = 0
        return dict(c, cam=e["cam_out"].view(f32).reshape(-1, 12).copy(), points=pts), e

    both, _ = adjusted(case, 6)
    first, _ = adjusted(case, 3)
    f = FC.expected_filter(dict(first, **{k: case[k] for k in FC.ARGS}))
    second, _ = adjusted(FC.filtered_case(first, f), 3)
    # the clean observations of the surviving tracks, by their old slot and track and by their new ones
    code, track = f["obs_map"].view(np.int32)[:O], f["track_map"].view(np.int32)[:T]
    owner = f["res"]["slots"]["owner"]
    sel = np.nonzero(sc["clean"] & (owner >= 0) & (track[np.maximum(owner, 0)] >= 0))[0]
    got = {"adjust, adjust": _clean_rms(case, both["cam"], both["points"], sel, owner[sel]),
           "adjust, filter, adjust": _clean_rms(case, second["cam"], second["points"], sel, track[owner[sel]]),
           "clean removed": float((code[sc["clean"]] < 0).mean())}
    print("measured: %s; T %d -> %d, O %d -> %d" % (got, T, f["summary"].view(np.int32)[0], O,
                                                    f["summary"].view(np.int32)[1]))
    assert got["adjust, filter, adjust"] < got["adjust, adjust"]

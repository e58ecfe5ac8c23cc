"""misift_describe_points_batch and misift_localize_frames_batch without a GPU: the numpy restatements of
localize_cases against the library's host hooks (compiled from localize_core.hpp, the functions the kernels run) on every
case of test_gpu_localize.py, what each case is built to hit, the rounding of the mean by brute force, localise against
resect on the same candidates, the planted scenes of resect's own test, and the chain describe -> match -> localise ->
merge -> triangulate in numpy."""
import numpy as np
import pytest

import batch_util as BU
import localize_cases as L
import merge_cases as MC
import refine_cases as RC
import resect_cases as C
import triangulate_cases as TC
from test_fundamental_cpu import f32


def test_library_exports_the_calls():
    from cudasift_amd import capi
    lib = capi.lib()
    for name in ("misift_describe_points_batch", "misift_test_describe_points", "misift_localize_frames_batch",
                 "misift_test_localize_candidates"):
        assert hasattr(lib, name), name
    assert callable(capi.Context.describe_points_batch) and callable(capi.Context.localize_frames_batch)


# ---- describe

@pytest.mark.parametrize("name", L.DESCRIBE_GPU_CASES)
def test_describe_restatement_equals_the_hook(name):
    case = L.describe_gpu_cases()[name]
    e, h = L.expected_describe(case), L.hook_describe(case)
    for k in L.DESCRIBE_OUTPUTS:
        assert e[k].tobytes() == h[k].tobytes(), (name, k, np.nonzero(e[k] != h[k])[0][:8])


def test_describe_premises():
    cases = L.describe_gpu_cases()
    e = L.expected_describe(cases["lengths padded"])
    T = len(L.LENGTHS)
    assert e["point_members"].view(np.int32)[:T].tolist() == list(L.LENGTHS)
    assert e["summary"].view(np.int32).tolist()[:4] == [T, T - 1, sum(L.LENGTHS), 0]
    q = e["scene_q"].view(np.int8).reshape(-1, 128)
    assert (q[0] == 0).all() and (q[1:T] >= 0).all() and (q[T:].view(np.uint8) == L.POISON_BYTE).all()
    assert (e["scene_recs"].reshape(-1, 144)[:T, 3:] == 0).all()
    assert (e["scene_recs"].reshape(-1, 144)[T:] == L.POISON_WORD).all()
    # m = 1: the row itself
    c1 = cases["lengths padded"]
    lay = L.frame_layout(c1)
    o = int(c1["track_offsets"][1])
    row = lay[int(c1["obs"]["frame"][o])][1] + int(c1["obs"]["record"][o])
    assert (q[1] == c1["q"][row]).all()
    for packed in ("padded", "packed"):
        case = cases["hostile " + packed]
        h = L.expected_describe(case)
        T, O = RC.counts(case)
        m = h["point_members"].view(np.int32)[:T]
        first = len(L.LENGTHS)
        assert m[first:first + 2].tolist() == [2, 2]             # four bad frames, four bad records
        desc = (h["scene_q"].view(np.int8).reshape(-1, 128)[:T] != 0).any(1)
        assert not desc[first + 2:first + 7].any() and desc[first + 7]      # status, NaN, inf; the fourth word is free
        assert m[first + 8] == 0 and m[first + 9] == 15 and m[T - 1] == 0    # descending, overlapping, beyond O
        s = h["summary"].view(np.int32)
        assert s[3] == 8 and s[1] == desc.sum() and s[2] == m[desc].sum()
        b = L.expected_describe(cases["bad frames " + packed])
        assert b["summary"].view(np.int32)[3] > 0
        lay = L.frame_layout(cases["bad frames " + packed])
        assert [x[2] for x in lay] == [True, True, True, True, False] and lay[3][0] == 0
    for name, T in (("T -1", 0), ("T below", 9), ("T beyond", len(L.LENGTHS) + 2), ("T INT_MIN O INT_MIN", 0)):
        assert L.expected_describe(cases[name])["scene_count"].view(np.int32)[0] == T
    assert L.expected_describe(cases["O -5"])["summary"].view(np.int32).tolist()[:3] == [len(L.LENGTHS), 0, 0]
    low = L.expected_describe(cases["O below"])["point_members"].view(np.int32)[:len(L.LENGTHS)]
    assert (low > 0).any() and low[-1] == 0                      # the tracks that end beyond O = 100 are not valid


def test_mean_rounding_by_brute_force():
    """Python integers over rows with ties: the mean of (1, 2) is 2, of (1, 1, 2) is 1, of (1, 1, 3) is 2; 301 rows of
    127 give 127; a described point is all zero only if its rows are."""
    case = L.ties_case()
    h = L.hook_describe(case)
    q = h["scene_q"].view(np.int8).reshape(-1, 128)
    assert (q[0] == 2).all()
    a = np.arange(128) % 127
    assert (q[1] == a + 1).all()                                 # a tie in every byte
    assert (q[2] == 127).all()
    assert (q[3, :64] == 1).all() and (q[3, 64:] == 2).all()
    rng = np.random.default_rng(8)
    for m in (1, 2, 3, 5, 8):
        rows = rng.integers(0, 128, (m, 128))
        rows[:, :8] = 0
        rows[0, 8] = 1                                           # sum 1 over m rows: rounds to 0 from m = 3 on
        case = L.describe_case((m,), seed=1, frame_sizes=(m,), slack_tracks=0, slack_obs=0)
        qq = np.zeros((case["max_records"], 128), np.int8)
        qq[:m] = rows
        obs = case["obs"].copy()
        obs["frame"], obs["record"] = 0, np.arange(m)
        got = L.hook_describe(dict(case, q=qq, obs=obs))["scene_q"].view(np.int8)[:128]
        want = [(2 * int(rows[:, k].sum()) + m) // (2 * m) for k in range(128)]
        assert got.tolist() == want, m
        assert all(0 <= v <= 127 for v in want) and (got[:8] == 0).all()
        if m == 1:
            assert (got == rows[0]).all()


# ---- localise

@pytest.mark.parametrize("name", L.LOCALIZE_GPU_CASES)
def test_candidates_restatement_equals_the_hook(name):
    case = L.localize_gpu_cases()[name]
    T = RC.counts(dict(case, max_obs=1))[0]
    for e in range(len(case["frames"])):
        rows = L.frame_rows(case, int(case["frames"][e]))
        if rows is None:
            continue
        r, t, xy, X = L.candidates(rows, T, case["points"], case["point_status"], case["min_score"], case["max_ambiguity"])
        hr, ht, h5 = L.hook_candidates(rows, T, case["points"], case["point_status"], case["min_score"],
                                       case["max_ambiguity"])
        assert hr.tolist() == r.tolist() and ht.tolist() == t.tolist(), (name, e)
        assert h5.tobytes() == np.concatenate([xy, X], 1).astype(f32).tobytes(), (name, e)


@pytest.mark.parametrize("name", L.RESECT_TWINS)
def test_localize_agrees_with_resect(name):
    """The rows of a frame list exactly the candidates expected_resect gathers for the image, in the same order and with
    the same seed: resect's twelve floats, inliers and status, byte for byte (an image resect turns away for max_cand,
    which localise does not have, aside)."""
    case = L.localize_gpu_cases()["resect: " + name]
    rcase = case["resect"]
    er, el = C.expected_resect(rcase), L.expected_localize(case)
    n = len(rcase["images"])
    keep = np.array([x["status"] != C.OVER for x in er["entries"]], bool)
    for k in ("res_cand", "res_inliers", "res_status"):
        assert (er[k][keep] == el[k][keep]).all(), (name, k)
    assert (er["res_cam"].reshape(n, 12)[keep] == el["res_cam"].reshape(n, 12)[keep]).all()
    if keep.all():
        assert er["cam"].tobytes() == el["cam"].tobytes() and er["cam_pair"].tobytes() == el["cam_pair"].tobytes()
        assert er["summary"][:7].tobytes() == el["summary"][:7].tobytes()
    for x, y in zip(er["entries"], el["entries"]):
        if y["status"] == C.OK:
            assert len(y["finds"][0]) == y["inliers"]


def test_localize_premises():
    cases = L.localize_gpu_cases()
    st = [x["status"] for x in L.expected_localize(cases["all statuses"])["entries"]]
    assert sorted(set(st)) == [0, 1, 2, 3, 4], st
    for k in ("hostile padded", "hostile packed"):
        e, plain = L.expected_localize(cases[k]), L.expected_localize(L.from_resect(cases[k]["resect"]))
        assert e["res_cam"].tobytes() == plain["res_cam"].tobytes()         # the hostile rows are nobody's candidate
        assert e["res_cand"].tobytes() == plain["res_cand"].tobytes() and e["N"] == plain["N"] > 0
        rows_h = e["found_obs"].view(L.OBS_DTYPE)["record"][:e["N"]]
        rows_p = plain["found_obs"].view(L.OBS_DTYPE)["record"][:e["N"]]
        assert (rows_h >= rows_p).all() and (rows_h > rows_p).any()         # the row index is the frame's, not the list's
    assert [x["status"] for x in L.expected_localize(cases["max_pts one below n"])["entries"]] == [0, 0, 4]
    assert [x["status"] for x in L.expected_localize(cases["max_pts 1030"])["entries"]] == [0, 0, 0]
    assert [x["cand"] for x in L.expected_localize(cases["count -1"])["entries"]][1] == 0
    full = L.expected_localize(cases["max_found N"])
    N = full["N"]
    for name, Tp in (("N-1", N - 1), ("N", N), ("N+1", N), ("1", 1)):
        e = L.expected_localize(cases["max_found " + name])
        assert e["found_summary"].view(np.int32).tolist()[:5] == [N, N, Tp, Tp, 1] and e["summary"].view(np.int32)[7] == Tp
        assert e["found_map"][:Tp].tobytes() == full["found_map"][:Tp].tobytes()
    cut = L.expected_localize(cases["max_found cuts an entry"])
    ents = cut["entries"]
    assert ents[0]["inliers"] < cases["max_found cuts an entry"]["max_found"] < ents[0]["inliers"] + ents[1]["inliers"]
    many = L.expected_localize(cases["several rows to one point"])
    t = many["found_map"].view(np.int32)[:many["N"]]
    assert len(set(t.tolist())) < len(t)                         # two finds of one point: both emitted
    empty = L.expected_localize(cases["resect: nsel 0"])
    assert empty["N"] == 0 and empty["found_offsets"].view(np.int32)[0] == 0
    assert empty["found_summary"].view(np.int32).tolist() == [0] * 8


QUALITY_SEEDS = (91, 92, 93)
QUALITY_COUNTS = (40, 400, 2000)
# measured over these scenes (printed below): the float32 camera differs from the float64 twin of the algorithm by at most
# 4.9e-4 rad (the resolution of the angle of a float32 rotation matrix) and 6.9e-6 in the centre; against the planted
# camera the worst is 6.4e-3 rad and 5.6e-2 (seed 92 at 40 correspondences); at least 90.0 % of the planted inliers held
TWIN_ROTATION, TWIN_CENTRE = 4 * 4.9e-4, 4 * 6.9e-6
PLANTED_ROTATION, PLANTED_CENTRE = 4 * 6.4e-3, 4 * 5.6e-2


@pytest.mark.parametrize("seed", QUALITY_SEEDS)
def test_localize_quality_on_planted_scenes(seed):
    """Resect's planted scenes as match rows: 40, 400 and 2000 correspondences, a quarter wrong, 0.5 px noise, 1024
    hypotheses at 4 px.  The share of planted inliers held is resect's bound (0.9); the float32 camera stays within four
    times the measured worst of its float64 twin."""
    sc = C.planted(QUALITY_COUNTS, seed)
    rcase = C.resect_case(sc["case"], [0, 1, 2], seeds=[1000 + seed] * 3, num_loops=1024, thresh=4.0, max_cand=4096)
    case = L.from_resect(rcase, max_found=1)
    keys = RC.candidate_keys(rcase)
    for e, n in enumerate(QUALITY_COUNTS):
        slots = RC.image_candidates(rcase, e, keys)[0]
        good = np.isin(slots, sc["good"][e])
        cams = {}
        for dt in (f32, np.float64):
            x = L.expected_loc_entry(case, e, dt)
            assert x["status"] == C.OK
            held = np.isin(np.nonzero(good)[0], x["finds"][0]).mean()     # row r is candidate r here
            eR, eC = C.pose_error(x["cam"], sc["true"][e])
            print("seed %d, n %d, %s: %d inliers, %.1f %% of the planted ones, rotation %.2e rad, centre %.2e" % (
                seed, n, dt.__name__, x["inliers"], 100 * held, eR, eC))
            assert held >= 0.9, (seed, n, dt, held)
            cams[dt] = x["cam"]
        dR, dC = C.pose_error(cams[f32], cams[np.float64])
        print("seed %d, n %d: float32 against float64: rotation %.2e rad, centre %.2e" % (seed, n, dR, dC))
        assert dR < TWIN_ROTATION and dC < TWIN_CENTRE, (seed, n, dR, dC)


def test_describe_match_localize_merge_triangulate():
    """The chain in numpy on a planted window of eight cameras whose last image is not in the export: describe, the int8
    match of batch_util against the scene frame, localise, merge_cases.expected_merge, triangulate_cases."""
    w = L.window()
    d = w["describe"]
    ed = L.expected_describe(d)
    npts = w["npts"]
    assert ed["summary"].view(np.int32).tolist()[:4] == [npts, npts, 7 * npts, 0]
    recs2, q2 = L.scene_records(d, ed)
    assert len({r.tobytes() for r in d["q"]}) == len(d["q"])    # every view quantises to a row of its own
    rows = BU.match_np(w["query"][0], w["query_q"][0], recs2, q2)
    last = w["nimages"] - 1
    truth = w["perm"][last]                                      # the point record r of the new image shows
    assert (rows["match"] == truth).all()
    assert (rows["match_xpos"].view(np.uint32) == d["points"][truth, 0].view(np.uint32)).all()
    case = L.window_localize_case(w, rows)
    e = L.expected_localize(case)
    x = e["entries"][0]
    assert x["status"] == C.OK and x["inliers"] >= 0.9 * (npts - len(w["moved"][0]))
    eR, eC = C.pose_error(x["cam"], w["true"][last])
    print("window: %d of %d rows are finds, rotation %.2e rad, centre %.2e" % (x["inliers"], npts, eR, eC))
    assert eR < PLANTED_ROTATION and eC < PLANTED_CENTRE         # four times the worst of the planted scenes above
    assert e["cam_pair"].view(np.int32)[last] == C.RESECTED
    mc = L.window_merge_case(w, case, e)
    em = MC.expected_merge(mc)
    hm = MC.hook_merge(mc)
    MC.compare(hm, em, "window", keys=[k for k in MC.OUTPUTS if k != "record_obs_out"])
    merged = MC.merged_sets(em)
    by_point = {}
    for s in merged:
        for f, r in s:
            if f < last:
                by_point[int(w["perm"][f][r])] = s
    N = e["N"]
    fo = e["found_obs"].view(L.OBS_DTYPE)[:N]
    assert N == x["inliers"] and (fo["frame"] == last).all()
    for r, t in zip(fo["record"], e["found_map"].view(np.int32)[:N]):
        if int(r) not in w["moved"][0]:
            assert t == truth[r] and (last, int(r)) in by_point[int(t)]
    assert int(em["export_summary_out"].view(np.int32)[3]) == 7 * npts + N
    ms = MC.merged_scene(mc, em)
    tri = dict(ms, intrinsics=w["K"], min_views=2, num_loops=5, memo={})
    with np.errstate(all="ignore"):
        t3 = TC.expected_triangulate(tri)
    T = int(ms["export_summary"][2])
    assert (t3["point_status"].view(np.int32)[:T] == 0).all()
    views = t3["point_views"].view(np.int32)[:T]
    assert views.sum() == 7 * npts + N and views.max() == 8

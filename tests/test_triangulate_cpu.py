"""misift_triangulate_tracks_batch without a GPU: triangulate_cases.expected_triangulate, the numpy float32 restatement of
the definition in include/misift.h, which tests/test_gpu_triangulate.py holds the device to byte for byte.  Here the
restatement is pinned from both sides: the library's host-only hook misift_test_triangulate_track, compiled from the
function a lane of the kernel runs, must equal it byte for byte on every case of the GPU file, and on planted scenes its
answer is held to the same algorithm in float64 on the same inputs.  The premises of the cases are asserted here too."""
import numpy as np
import pytest

import triangulate_cases as TC
from test_fundamental_cpu import f32

CAPACITY = 512                                                   # asserted against the library's hook below


def same_as_hook(case, what, obs_error=True):
    """The hook equals the restatement byte for byte on every track of the case whose range is valid; returns the
    expected outputs."""
    e = TC.expected_triangulate(case)
    T = min(max(int(case["export_summary"][2]), 0), case["max_tracks"])
    for t in range(T):
        off, end = int(case["track_offsets"][t]), int(case["track_offsets"][t + 1])
        if not TC.range_ok(off, end, case["max_obs"]):
            assert e["point_status"][t] == TC.BAD_RANGE
            continue
        h = TC.hook_track(case["cam"], case["cam_pair"], case["intrinsics"], case["nimages"], case["obs"][off:end],
                          case["min_views"], case["num_loops"], obs_error)
        x = case["memo"][(off, end, case["min_views"], case["num_loops"])]
        assert (h["views"], h["status"], h["accepted"]) == (x["views"], x["status"], x["accepted"]), (what, t, h, x)
        assert h["point4"].tobytes() == x["point4"].tobytes(), (what, t, h["point4"], x["point4"])
        if obs_error:
            assert h["obs_error"].tobytes() == x["obs_error"].tobytes(), (what, t, h["obs_error"], x["obs_error"])
        else:
            assert (h["obs_error"] == f32(3.5)).all(), (what, t, "obs_error written through NULL")
    return e


def test_library_exports_the_call():
    """Fails without the feature: the symbols, their rows in capi.SIGNATURES, the binding, the argument checks that need
    no device."""
    from cudasift_amd import capi
    L = capi.lib()
    for name in ("misift_triangulate_tracks_batch", "misift_test_triangulate_track", "misift_test_triangulate_capacity"):
        assert name in capi.SIGNATURES and hasattr(L, name), name
    assert hasattr(capi.Context, "triangulate_tracks_batch")
    assert L.misift_triangulate_tracks_batch(None, 1, 1, None, None, None, 1, None, None, None, 2, 0, None, None, None,
                                             None, None) == -1  # MISIFT_EINVAL
    assert L.misift_test_triangulate_track(None, None, None, 1, None, 0, 2, 0, None, None, None, None, None) == -1
    assert TC.capacity() == CAPACITY
    assert capi.TRACK_OBS_DTYPE == TC.OBS_DTYPE


@pytest.mark.parametrize("num_loops,min_views", [(5, 2), (0, 2), (1, 3)])
def test_hostile_tracks_equal_the_hook(num_loops, min_views):
    case = TC.hostile_case(num_loops, min_views)
    e = same_as_hook(case, "hostile")
    status = dict(zip(case["names"], e["point_status"].view(np.int32).tolist()))
    views = dict(zip(case["names"], e["point_views"].view(np.int32).tolist()))
    assert len(status) == len(case["names"])                     # the names are distinct
    few = TC.FEW_VIEWS if min_views > 2 else TC.OK
    assert status["good"] == TC.OK and views["good"] == 4 and status["good again"] == TC.OK
    for name in ("frame -1", "frame nimages", "frame far out of range", "an unset camera", "a NaN in a camera",
                 "an inf in a camera"):
        assert (status[name], views[name]) == (few, 2), name     # the hostile view is left out, the others are used
    for name in ("a NaN x", "an inf y"):
        assert (status[name], views[name]) == (TC.OK, 3), name
    for name, m in (("only out-of-range frames", 0), ("an unset camera leaves one view", 1), ("one observation", 1),
                    ("a -inf x leaves one view", 1), ("no observation", 0)):
        assert (status[name], views[name]) == (TC.FEW_VIEWS, m), name
    assert status["behind one camera"] == TC.BEHIND and views["behind one camera"] == 4
    assert status["behind one of two"] == (TC.BEHIND if min_views == 2 else TC.FEW_VIEWS)
    assert status["identical cameras, identical positions"] == (TC.SINGULAR if min_views == 2 else TC.FEW_VIEWS)
    assert status["identical cameras, three times"] == TC.SINGULAR
    assert status["huge positions"] == TC.SINGULAR
    assert views["two observations from one frame"] == 4 and status["two observations from one frame"] == TC.OK
    # a failed track holds the one quiet NaN everywhere, its views all the same
    pts, err = e["points"].reshape(-1, 4), e["obs_error"]
    for t, name in enumerate(case["names"]):
        off, end = case["track_offsets"][t:t + 2]
        if status[name] != TC.OK:
            assert (pts[t] == TC.PC.NAN_BITS).all() and (err[off:end] == TC.PC.NAN_BITS).all(), name
        else:
            use = TC.usable_views(case["cam"], case["cam_pair"], case["nimages"], case["obs"][off:end])
            assert np.isfinite(pts[t].view(f32)).all(), name
            assert (np.isfinite(err[off:end].view(f32)) == use).all() and (err[off:end][~use] == TC.PC.NAN_BITS).all()
    assert (err[case["track_offsets"][len(case["names"])]:] == TC.POISON_WORD).all()        # behind the last track
    s = e["summary"].view(np.int32)
    assert s[0] == len(case["names"]) == s[1] + s[3] + s[4] + s[5] and s[7] == 0
    assert (s[6] > 0) == (num_loops > 0)


def test_bad_offsets():
    case = TC.bad_offsets_case()
    e = same_as_hook(case, "bad offsets")
    st = e["point_status"].view(np.int32)
    assert np.nonzero(st == TC.BAD_RANGE)[0].tolist() == case["bad"] and e["summary"].view(np.int32)[7] == len(case["bad"])
    assert (st[[0, 1, 4, 7, 10]] == TC.OK).all()
    assert (e["points"].reshape(-1, 4)[case["bad"]] == TC.PC.NAN_BITS).all()
    assert (e["point_views"].view(np.int32)[case["bad"]] == 0).all()


@pytest.mark.parametrize("num_loops,min_views", [(5, 2), (0, 2), (1, 3)])
def test_the_pool_equals_the_hook(num_loops, min_views):
    case = TC.pool_case(num_loops, min_views)
    e = same_as_hook(case, "pool", obs_error=num_loops != 1)
    lengths = np.diff(case["track_offsets"][:259])
    assert sorted(set(lengths.tolist())) == [1, 2, 3, 7, 301]
    s = e["summary"].view(np.int32)
    assert s[0] == 258 and s[3] == (lengths < min_views).sum() and s[1] == 258 - s[3]
    # a cut of the pool: T below, at and beyond max_tracks, and negative
    for T, mt, want in ((63, 258, 63), (300, 258, 258), (-5, 258, 0), (65, 64, 64), (0, 1, 0)):
        cut = TC.expected_triangulate(TC.with_T(case, T, mt))
        assert cut["summary"].view(np.int32)[0] == want
        assert (cut["points"][4 * want:] == TC.POISON_WORD).all() and (cut["point_status"][want:] == TC.POISON_WORD).all()
        assert cut["points"][:4 * want].tobytes() == e["points"][:4 * want].tobytes()
        assert (cut["obs_error"][case["track_offsets"][want]:] == TC.POISON_WORD).all()


@pytest.mark.parametrize("nimages", [CAPACITY - 1, CAPACITY, CAPACITY + 1, CAPACITY + 9])
def test_either_side_of_the_staging_capacity(nimages):
    case = TC.capacity_case(nimages)
    e = same_as_hook(case, "capacity")
    assert e["summary"].view(np.int32)[1] == 70 and case["obs"]["frame"].max() == nimages - 1


# ---- float64
#
# The same algorithm in float64 on the same inputs (triangulate_cases.triangulate64) is the yardstick; the figure is
# max over the tracks of |X32 - X64| / |X64|.  The scenes: 300 points 4 to 12 deep, seen by runs of 2 to 6 of six cameras
# whose neighbouring centres are `ratio` * 8 apart and which are turned by up to 0.05 rad; 0.5 px of noise or none.  All
# 300 tracks reach status 0 in both formats in every setting, which is asserted: no track is left out of a maximum.
# Measured at seed 51 with num_loops = 5, one figure per (ratio, noise); seeds 61 and 71 gave between a fifth and twice
# these.  The deviation stays orders of magnitude below what the noise itself does to the point (4e-3, 4e-2 and 1e-1 of
# |X| at the three ratios) and, without noise, is of the order of float64's own distance from the planted point.
MEASURED = {(0.5, 0.0): 3.76e-7, (0.5, 0.5): 2.86e-6, (0.05, 0.0): 1.68e-6, (0.05, 0.5): 5.42e-6, (0.02, 0.0): 4.41e-6,
            (0.02, 0.5): 3.02e-4}
# the linear start alone (num_loops = 0), the largest of the six settings (ratio 0.02 with noise); the Gauss-Newton steps
# do not only fit the noise better, they also repair the start's rounding
MEASURED_LINEAR = 6.97e-4


def deviation(case):
    e = TC.expected_triangulate(case)
    p32 = e["points"].view(f32).reshape(-1, 4).astype(np.float64)
    p64, s64, _ = TC.triangulate64(case)
    assert (e["point_status"].view(np.int32) == TC.OK).all() and (s64 == TC.OK).all()      # the share left out is 0
    return e, p32, p64, np.linalg.norm(p32[:, :3] - p64[:, :3], axis=1) / np.linalg.norm(p64[:, :3], axis=1)


@pytest.mark.parametrize("ratio,noise", sorted(MEASURED))
def test_planted_scenes_against_float64(ratio, noise):
    sc = TC.planted(ratio, noise)
    case = sc["case"]
    same_as_hook(case, "planted")
    e, p32, p64, rel = deviation(case)
    lengths = np.diff(case["track_offsets"])
    assert sorted(set(lengths.tolist())) == [2, 3, 4, 5, 6] and len(rel) == 300
    print("planted %s: max %.3g median %.3g" % ((ratio, noise), rel.max(), np.median(rel)))
    assert rel.max() <= 2 * MEASURED[(ratio, noise)], rel.max()
    # the linear start alone, and what the loops do to it
    start = TC.variant(case, num_loops=0)
    same_as_hook(start, "planted, linear start")
    e0, q32, _, rel0 = deviation(start)
    print("linear start %s: max %.3g median %.3g" % ((ratio, noise), rel0.max(), np.median(rel0)))
    assert rel0.max() <= 2 * MEASURED_LINEAR, rel0.max()
    assert (p32[:, 3] <= q32[:, 3]).all()                        # a kept step lowers c, so the rms error never rises
    steps = e["summary"].view(np.int32)[6]
    assert e0["summary"].view(np.int32)[6] == 0
    if noise:
        assert steps > 0 and (p32[:, :3] != q32[:, :3]).any(1).sum() >= 150 and (p32[:, 3] < q32[:, 3]).sum() >= 150
        truth = np.linalg.norm(p64[:, :3] - sc["X"], axis=1) / np.linalg.norm(sc["X"], axis=1)
        assert rel.max() < 0.1 * truth.max()                     # below the effect of the noise itself


# The 64-image chain of posegraph_cases under the cameras misift_link_poses_batch links: the last cameras sit 15 seed
# baselines from the root and the points up to 77 from it, so X and t no longer have their digits to themselves.
# Measured: fp32 within 2.54e-6 of float64 (median 1.7e-7), no worse at the far end of the chain than at the root; float64
# itself lies within 1.25e-5 of the planted points, which is the drift of the linked cameras; the rms reprojection error
# is 1.6e-4 px in both.
CHAIN_MEASURED = 2.54e-6


def test_chain_far_from_the_origin():
    sc = TC.chain_case()
    case = sc["case"]
    same_as_hook(case, "chain")
    e, p32, p64, rel = deviation(case)
    assert e["summary"].view(np.int32).tolist()[:3] == [244, 244, 976]
    far = np.linalg.norm(sc["X"], axis=1)
    print("chain: max %.3g median %.3g, last quarter %.3g, |X| up to %.3g, rms %.3g px" % (
        rel.max(), np.median(rel), rel[183:].max(), far.max(), p32[:, 3].max()))
    assert far.max() > 50 and rel.max() <= 2 * CHAIN_MEASURED
    truth = np.linalg.norm(p64[:, :3] - sc["X"], axis=1) / far
    assert truth.max() < 5e-5 and p32[:, 3].max() < 1e-3


def test_hook_arguments():
    from cudasift_amd import capi
    L = capi.lib()
    case = TC.planted(0.05, 0.5)["case"]
    cam, pair, K = case["cam"], case["cam_pair"], case["intrinsics"]
    obs = np.ascontiguousarray(case["obs"][:2])
    point, ints, err = np.zeros(4, f32), np.zeros(3, np.int32), np.zeros(2, f32)
    a = [cam.ctypes.data, pair.ctypes.data, K.ctypes.data, case["nimages"], obs.ctypes.data, 2, 2, 5, point.ctypes.data,
         ints.ctypes.data, ints.ctypes.data + 4, err.ctypes.data, ints.ctypes.data + 8]
    assert L.misift_test_triangulate_track(*a) == 0 and ints[1] == TC.OK
    for i, v in ((0, None), (1, None), (2, None), (3, 0), (4, None), (5, -1), (6, 1), (7, -1), (8, None), (9, None),
                 (10, None), (12, None)):
        b = list(a)
        b[i] = v
        assert L.misift_test_triangulate_track(*b) == -1, (i, v)

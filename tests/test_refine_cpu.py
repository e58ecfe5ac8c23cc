"""misift_refine_cameras_batch without a GPU: refine_cases.expected_refine, the numpy float32 restatement of the
definition in include/misift.h, which tests/test_gpu_refine.py holds the device to byte for byte.  Here the restatement
is pinned from both sides: the library's host-only hook misift_test_refine_camera, compiled from the function a
workgroup of the kernel runs, must equal it byte for byte on every case of the GPU file, and on planted scenes its answer
is held to the same algorithm in float64 on the same inputs.  The premises of the cases are asserted here too."""
import numpy as np
import pytest

import refine_cases as RC
from test_fundamental_cpu import f32


def same_as_hook(case, what):
    """The hook equals the restatement byte for byte on every image of the case; returns the expected outputs."""
    e = RC.expected_refine(case)
    keys = RC.candidate_keys(case)
    cam = np.ascontiguousarray(case["cam"], f32).reshape(-1, 12)
    for i, x in enumerate(e["images"]):
        slots, X, xy = RC.image_candidates(case, i, keys)
        for in_place in (False, True):
            h = RC.hook_camera(cam[i], case["cam_pair"][i], i in case["hold"], case["intrinsics"][i], slots, X, xy,
                               case["min_obs"], case["num_loops"], case["max_error"], case["orthonormalise"], in_place)
            assert (h["nobs"], h["steps"], h["status"]) == (x["nobs"], x["steps"], x["status"]), (what, i, h, x)
            assert h["cam"].tobytes() == e["cam_out"][12 * i:12 * i + 12].tobytes(), (what, i, h["cam"], x["cam"])
            assert h["rms"].tobytes() == e["cam_rms"][2 * i:2 * i + 2].tobytes(), (what, i, h["rms"], x["rms"])
    return e


def test_library_exports_the_call():
    """Fails without the feature: the symbols, their rows in capi.SIGNATURES, the binding, the argument checks that need
    no device."""
    from cudasift_amd import capi
    L = capi.lib()
    for name in ("misift_refine_cameras_batch", "misift_test_refine_camera"):
        assert name in capi.SIGNATURES and hasattr(L, name), name
    assert hasattr(capi.Context, "refine_cameras_batch")
    assert L.misift_refine_cameras_batch(None, 1, 1, None, None, None, None, None, 1, None, None, None, 0, None, 3, 0, 1.0,
                                         0, None, None, None, None, None, None) == -1  # MISIFT_EINVAL
    assert L.misift_test_refine_camera(None, 0, 0, None, 0, None, None, None, 3, 0, 1.0, 0, None, None, None, None,
                                       None) == -1


@pytest.mark.parametrize("O", [0, 1, 255, 256, 257, 513])
def test_every_slot_count_equals_the_hook(O):
    case = RC.spread_case(O)
    assert RC.counts(case)[1] == O
    e = same_as_hook(case, "O = %d" % O)
    assert (e["summary"].view(np.int32)[1] > 0) == (O >= 255)


def test_counts_from_the_device():
    base = RC.spread_case(513)
    full = same_as_hook(base, "spread")
    assert (base["max_tracks"], base["max_obs"]) == (171, 513)
    for T, O, wantT in ((63, 513, 63), (171, 200, 171), (300, 10 ** 9, 171), (-1, 513, 0), (171, -5, 171), (171, 256, 171)):
        case = RC.with_counts(base, T, O)
        e = same_as_hook(case, "T = %d, O = %d" % (T, O))
        assert e["summary"].view(np.int32)[0] == wantT
        cut = (T, O) not in ((300, 10 ** 9),)
        assert (e["cam_obs"].view(np.int32).sum() < full["cam_obs"].view(np.int32).sum()) == cut
    # a track that ends beyond O is not valid: its slots below O have no owner
    case = RC.with_counts(base, None, 200)
    key, owner = RC.candidate_keys(case)
    offs = base["track_offsets"]
    t = int(np.searchsorted(offs[:172], 200, side="right") - 1)
    if offs[t] < 200 < offs[t + 1]:
        assert (owner[offs[t]:200] == -1).all()


@pytest.mark.parametrize("nimages", [1, 2, 3, 64, 65])
def test_every_image_count_equals_the_hook(nimages):
    case = RC.scene(RC.runs(8 * nimages, nimages, 66), nimages, 66, orthonormalise=1)["case"]
    s = same_as_hook(case, "%d images" % nimages)["summary"].view(np.int32)
    assert s[5] == 1 and s[1] + s[3] == nimages - 1 and (nimages < 3 or s[1] >= nimages // 2)


def test_around_min_obs_and_one_lane_slot():
    e = same_as_hook(RC.member_counts_case(), "around min_obs")
    assert e["cam_obs"].view(np.int32).tolist() == [0, 5, 6, 7, 0, 40]
    assert e["cam_status"].view(np.int32).tolist() == [RC.HELD, RC.FEW_OBS, RC.OK, RC.OK, RC.FEW_OBS, RC.OK]
    case = RC.one_lane_case()
    key, _ = RC.candidate_keys(case)
    assert (np.nonzero(key == 1)[0] % 256 == 5).all() and (key == 1).sum() == 8
    e = same_as_hook(case, "one lane slot")
    assert e["cam_status"].view(np.int32).tolist() == [RC.HELD, RC.OK, RC.OK, RC.OK]


@pytest.mark.parametrize("max_error,num_loops,orth", [(RC.INF, 0, 0), (RC.INF, 1, 1), (8.0, 5, 0), (RC.INF, 5, 1),
                                                      (8.0, 0, 1)])
def test_gate_loops_and_orthonormalise(max_error, num_loops, orth):
    for name, base in (("spread", RC.spread_case(513)), ("hostile", RC.hostile_case())):
        case = RC.variant(base, max_error=max_error, num_loops=num_loops, orthonormalise=orth)
        e = same_as_hook(case, name)
        s = e["summary"].view(np.int32)
        assert (s[6] > 0) == (num_loops > 0) and s[1] > 0
        gated = sum(x["gated"] for x in e["images"])
        assert (gated > 0) == (max_error == 8.0) and s[2] > 100  # the gate really decides, and leaves members
        if num_loops == 0 and orth == 0:
            assert e["cam_out"].tobytes() == np.ascontiguousarray(case["cam"], f32).tobytes()
        if orth:
            moved = e["cam_out"].reshape(-1, 12) != np.ascontiguousarray(case["cam"], f32).view(np.uint32).reshape(-1, 12)
            assert moved[np.array(e["cam_status"].view(np.int32)) <= RC.SINGULAR, :9].any()


def test_hostile_premises():
    case = RC.hostile_case()
    e = same_as_hook(case, "hostile")
    st = e["cam_status"].view(np.int32).tolist()
    want = dict(root=RC.HELD, held=RC.HELD, good=RC.OK, unset=RC.NO_CAMERA, behind=RC.OK)
    want.update({"a NaN": RC.NO_CAMERA, "an inf": RC.NO_CAMERA})
    assert st == [want[n] for n in case["names"]]
    cam_in = np.ascontiguousarray(case["cam"], f32).view(np.uint32).reshape(-1, 12)
    for i in (0, 1, 3, 4, 5):                                    # copied as given, the NaN's bits included
        assert (e["cam_out"].reshape(-1, 12)[i] == cam_in[i]).all()
        assert (e["cam_rms"].reshape(-1, 2)[i] == RC.PC.NAN_BITS).all() and e["cam_obs"][i] == 0
    key, owner = RC.candidate_keys(case)
    T, O = RC.counts(case)
    offs = case["track_offsets"]
    for t in range(10, 17):                                      # failed and non-finite points give no candidate
        assert offs[t + 1] > offs[t] and (key[offs[t]:offs[t + 1]] == -1).all(), t
    for o in (20, 33, 47, 48, 60, 61, 62):                       # frames outside the images, non-finite positions
        assert key[o] == -1 and owner[o] >= 0, o
    # the three points behind image 7 are candidates and no members
    slots, X, xy = RC.image_candidates(case, 7, (key, owner))
    assert len(slots) == e["images"][7]["nobs"] + 3 and set(case["behind"]) <= set(owner[slots])


def test_bad_offsets_premises():
    case = RC.bad_offsets_case()
    same_as_hook(case, "bad offsets")
    key, owner = RC.candidate_keys(case)
    offs, good = case["track_offsets"], RC.scene(RC.runs(40, 4, 65, lengths=(3, 4)), 4, 65)["case"]["track_offsets"]
    T, O = RC.counts(case)
    assert (owner[good[4]:good[6]] == -1).all()                  # a negative end, a negative start
    assert (owner[good[7]:good[10]] == 9).all()                  # track 9 reaches back over 7 and 8 and owns them
    assert (owner[good[19]:good[21]] == -1).all() and offs[20] > O
    assert (owner[good[10]:good[19]] >= 10).all() and (owner[:good[4]] == np.repeat(np.arange(4), np.diff(good[:5]))).all()


def test_a_rejected_step_and_a_member_behind_a_trial_camera():
    e = same_as_hook(RC.rejected_step_case(), "rejected step")
    assert e["images"][1]["trace"] == ["kept", "worse"] and e["cam_steps"].view(np.int32)[1] == 1
    e = same_as_hook(RC.behind_trial_case(), "behind a trial camera")
    assert e["images"][1]["trace"] == ["behind"] and e["cam_status"].view(np.int32)[1] == RC.OK
    assert e["cam_out"].tobytes() == np.ascontiguousarray(RC.behind_trial_case()["cam"], f32).tobytes()


# ---- float64
#
# The same algorithm in float64 on the same inputs is the yardstick; the figure is max |fp32 - fp64| over the twelve
# entries of the refined camera of image 1.  The scenes (refine_cases.resection): n points 4 to 12 deep, fx about 1500,
# the start camera off by up to `err` rad and 5 * err units (Gaussian per axis), `noise` px on every position,
# num_loops = 5, the rotation re-orthonormalised first.  One figure per (n, noise): the worst over err = 0.001, 0.01 and
# 0.1 and the seeds 81, 82, 83.  Without noise both formats end at the planted camera and differ by a few fp32
# roundings of t; with noise the minimum is flatter the fewer the points, and the two formats stop at different places on it.
ERRS, SEEDS = (0.001, 0.01, 0.1), (81, 82, 83)
MEASURED = {(6, 0.0): 8.39e-7, (6, 0.5): 2.58e-5, (12, 0.0): 7.33e-7, (12, 0.5): 9.0e-6, (200, 0.0): 8.76e-7,
            (200, 0.5): 3.9e-6, (2000, 0.0): 5.45e-7, (2000, 0.5): 1.69e-6}
# |R^T R - I| (largest entry) of the refined fp32 rotation, the worst of all the scenes above; float64's is 1e-15
MEASURED_ORTHO = 4.32e-7


def _cam_error(c, true):
    return float(np.abs(np.asarray(c, np.float64) - true).max())


def _ortho(c):
    R = np.asarray(c, np.float64)[:9].reshape(3, 3)
    return float(np.abs(R.T @ R - np.eye(3)).max())


@pytest.mark.parametrize("n,noise", sorted(MEASURED))
def test_planted_scenes_against_float64(n, noise):
    worst, ortho, steps = 0.0, 0.0, 0
    for err in ERRS:
        for seed in SEEDS:
            sc = RC.resection(n, noise, err, seed, orthonormalise=1)
            case = sc["case"]
            if n <= 200:
                same_as_hook(case, "planted")
            x32, x64 = RC.per_image(case)[1], RC.per_image(case, np.float64)[1]
            assert x32["status"] == RC.OK == x64["status"] and x32["nobs"] == n == x64["nobs"]
            assert x32["steps"] >= 1 and x64["steps"] >= 1
            dev = float(np.abs(x32["cam"].astype(np.float64) - x64["cam"]).max())
            worst, ortho, steps = max(worst, dev), max(ortho, _ortho(x32["cam"])), max(steps, x32["steps"])
            assert _ortho(x64["cam"]) < 1e-14
            assert x32["rms"][1] <= x32["rms"][0]
            start, true = np.asarray(case["cam"], np.float64).reshape(-1, 12)[1], sc["true"][1]
            if noise == 0.0:                                     # planted recovery: closer than the start, every scene
                assert _cam_error(x32["cam"], true) < _cam_error(start, true), (err, seed)
                assert x32["rms"][1] < 0.01
            else:
                assert x32["rms"][1] < 2 * noise * np.sqrt(2)
    print("planted %s: max |fp32 - fp64| %.3g, |RtR - I| %.3g, steps up to %d" % ((n, noise), worst, ortho, steps))
    assert steps >= 3
    assert worst <= 2 * MEASURED[(n, noise)], worst
    assert ortho <= 2 * MEASURED_ORTHO, ortho


# The far end of the 64-image chain of posegraph_cases as misift_link_poses_batch links it: |R^T R - I| of camera 63 is
# 7.35e-6 as given (the worst of the last 16 cameras) and 2.75e-7, the rounding level, once re-orthonormalised.
CHAIN_ORTHO_BEFORE, CHAIN_ORTHO_AFTER = 7.35e-6, 2.75e-7


def test_orthonormalise_at_the_far_end_of_the_chain():
    sc = RC.chain_start(orthonormalise=1, num_loops=0)
    case = sc["case"]
    e = RC.expected_refine(case)
    before = max(_ortho(c) for c in np.asarray(case["cam"], f32).reshape(-1, 12)[48:])
    after = max(_ortho(c) for c in e["cam_out"].view(f32).reshape(-1, 12)[48:])
    print("chain: |RtR - I| of the last 16 cameras %.3g as given, %.3g re-orthonormalised" % (before, after))
    assert before > 20 * after
    assert after <= 2 * CHAIN_ORTHO_AFTER and before <= 2 * CHAIN_ORTHO_BEFORE
    slots, X, xy = RC.image_candidates(case, 63)
    cam = np.asarray(case["cam"], f32).reshape(-1, 12)[63]
    h = RC.hook_camera(cam, case["cam_pair"][63], False, case["intrinsics"][63], slots, X, xy, 3, 0, RC.INF, 1)
    assert h["cam"].tobytes() == e["cam_out"][12 * 63:].tobytes() and h["status"] in (RC.OK, RC.FEW_OBS)


def test_alternation_with_triangulate():
    """triangulate -> refine -> triangulate, four rounds, in the restatements alone: 6 drifted cameras and 150 points, the
    root and the seed partner held, no gate.  The pooled rms over the observations does not rise in any round and is
    below the start after the first."""
    sc = RC.scene(RC.runs(150, 6, 67, lengths=(3, 4, 5)), 6, 67, noise=0.5, angle=0.02, shift=0.05, hold=(1,),
                  orthonormalise=1)
    case = sc["case"]

    def pooled(err):
        e = err[np.isfinite(err)].astype(np.float64)
        assert len(e) > 500
        return float(np.sqrt((e ** 2).mean()))

    cam = np.asarray(case["cam"], f32)
    pts, st, err = RC.triangulate_under(case, cam)
    rms = [pooled(err)]
    for _ in range(4):
        e = RC.expected_refine(RC.variant(case, points=pts, point_status=st))
        assert e["summary"].view(np.int32)[5] == 2 and e["summary"].view(np.int32)[1] == 4
        cam = e["cam_out"].view(f32).reshape(-1, 12)
        assert cam[:2].tobytes() == np.asarray(case["cam"], f32)[:2].tobytes()       # the gauge stays
        pts, st, err = RC.triangulate_under(case, cam)
        rms.append(pooled(err))
    print("alternation: pooled rms %s px" % ["%.4g" % r for r in rms])
    assert all(b <= a for a, b in zip(rms, rms[1:])) and rms[1] < rms[0]


def test_hook_arguments():
    from cudasift_amd import capi
    L = capi.lib()
    case = RC.spread_case(257)
    slots, X, xy = RC.image_candidates(case, 1)
    slots, X, xy = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(X, f32), np.ascontiguousarray(xy, f32)
    cam, K = np.ascontiguousarray(case["cam"][1], f32), np.ascontiguousarray(case["intrinsics"][1], f32)
    out, ints, rms = np.zeros(12, f32), np.zeros(3, np.int32), np.zeros(2, f32)
    a = [cam.ctypes.data, 0, 0, K.ctypes.data, len(slots), slots.ctypes.data, X.ctypes.data, xy.ctypes.data, 6, 5, np.inf,
         1, out.ctypes.data, ints.ctypes.data, rms.ctypes.data, ints.ctypes.data + 4, ints.ctypes.data + 8]
    assert L.misift_test_refine_camera(*a) == 0 and ints[2] == RC.OK
    down = slots[::-1].copy()
    for i, v in ((0, None), (3, None), (4, -1), (5, None), (6, None), (7, None), (8, 2), (9, -1), (10, 0.0), (10, np.nan),
                 (11, 2), (12, None), (13, None), (14, None), (15, None), (16, None), (5, down.ctypes.data)):
        b = list(a)
        b[i] = v
        assert L.misift_test_refine_camera(*b) == -1, (i, v)

"""The host side of the track chain reads misift_track_obs where it lies: the three host hooks that take an
observation array give byte-identical outputs whether the array is 16-byte aligned, as the case modules build it, or
sits at an address that is 4 mod 16.  (The public calls reject such a d_obs; the kernels load an observation with one
16-byte load.  The hooks run on the CPU and may ask for no more than the alignment of the type, which is 4.)"""
import numpy as np

import bundle_cases as BC
import bundle_robust_cases as BR
import filter_cases as FC
import triangulate_cases as TC


def at_4_mod_16(obs):
    """The same bytes in a view at byte offset 4 into a buffer whose base is 16-byte aligned."""
    raw = np.zeros(obs.nbytes + 32, np.uint8)
    base = (-raw.ctypes.data) % 16
    view = raw[base + 4:base + 4 + obs.nbytes].view(obs.dtype)
    view[:] = obs
    assert view.ctypes.data % 16 == 4 and view.tobytes() == obs.tobytes()
    assert np.ascontiguousarray(view).ctypes.data == view.ctypes.data        # the hooks' wrappers pass it on as it is
    return view


def aligned(obs):
    obs = np.ascontiguousarray(obs)
    if obs.ctypes.data % 16:
        raw = np.zeros(obs.nbytes + 16, np.uint8)
        base = (-raw.ctypes.data) % 16
        view = raw[base:base + obs.nbytes].view(obs.dtype)
        view[:] = obs
        obs = view
    assert obs.ctypes.data % 16 == 0
    return obs


def same_bytes(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


def test_triangulate_track_hook_reads_obs_at_any_4_byte_address():
    case = TC.planted(0.05, 0.5, ntracks=6, ncams=4, lengths=(2, 3, 4))["case"]
    offs = case["track_offsets"]
    for name, obs in (("aligned", aligned(case["obs"])), ("4 mod 16", at_4_mod_16(case["obs"]))):
        for t in range(int(case["export_summary"][2])):
            track = obs[offs[t]:offs[t + 1]]
            assert track.ctypes.data % 16 == obs.ctypes.data % 16           # a slot is 16 bytes
            args = (case["cam"], case["cam_pair"], case["intrinsics"], case["nimages"])
            want = TC.hook_track(*args, case["obs"][offs[t]:offs[t + 1]], case["min_views"], case["num_loops"])
            got = TC.hook_track(*args, track, case["min_views"], case["num_loops"])
            assert want["status"] == 0
            same_bytes(got, want, (name, t))


def test_filter_tracks_hook_reads_obs_at_any_4_byte_address():
    case = FC.variant(FC.lengths_case([2, 3], 4, 96), max_error=4.0)
    moved = FC.variant(case, obs=at_4_mod_16(case["obs"]))
    assert FC.inputs(moved)["obs"].ctypes.data % 16 == 4
    want = FC.hook_filter(FC.variant(case, obs=aligned(case["obs"])))
    assert want["summary"][0] > 0                                             # tracks survive: obs_out is written
    same_bytes(FC.hook_filter(moved), want, "filter")


def test_adjust_bundle_robust_hook_reads_obs_at_any_4_byte_address():
    case = BR.robust(BC.planted(40, 4, 1)["case"], BR.HUBER, 2.0)
    moved = dict(case, obs=at_4_mod_16(case["obs"]))
    assert BR.hook_args(moved)["obs"].ctypes.data % 16 == 4
    want = BR.hook_bundle_robust(dict(case, obs=aligned(case["obs"])))
    assert want["summary"].view(np.int32)[1] > 0                              # cameras were adjusted
    same_bytes(BR.hook_bundle_robust(moved), want, "bundle")

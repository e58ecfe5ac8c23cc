"""The premises of test_gpu_used_context.py, checked without a GPU: every step of used_context.table() has an expected
answer at each of its sizes, a reused host list cannot pass for the original, and the temp each step asks for is ordered
as the sequences assume."""
import re

import numpy as np
import pytest

import used_context as U

NAMES = [s.name for s in U.table()]
CALLS = ("match_pairs_batch", "match_pairs_batch_i8", "match_guided_batch", "match_epipolar_batch", "link_tracks_batch",
         "export_tracks_batch", "link_poses_batch", "triangulate_tracks_batch", "refine_cameras_batch",
         "resect_cameras_batch", "recover_pose_batch", "improve_fundamental_batch", "find_fundamental_batch",
         "find_homography_batch")


def test_the_table_holds_every_call_once():
    from cudasift_amd import capi
    assert tuple(NAMES) == CALLS
    for n in NAMES:
        assert "misift_" + n in capi.SIGNATURES and hasattr(capi.Context, n), n
    assert "misift_test_ctx_state" in capi.SIGNATURES
    assert capi.lib().misift_test_ctx_state(None, 0) < 0 and capi.lib().misift_test_ctx_state(None, 3) < 0
    for s in U.table():                                          # a step has a huge case or says why it has none
        assert ("huge" in s.sizes) != bool(s.no_huge), s.name
    assert [s.name for s in U.table() if s.no_huge] == ["match_pairs_batch", "link_poses_batch", "recover_pose_batch",
                                                        "improve_fundamental_batch"]
    assert [s.name for s in U.table() if not s.temp] == ["recover_pose_batch", "improve_fundamental_batch"]
    assert [s.name for s in U.table() if not s.carries_lists] == ["export_tracks_batch"]


@pytest.mark.parametrize("name", NAMES)
def test_expected_is_well_formed_at_every_size(name):
    """expected() runs at every size; it names device buffers only, with exactly their bytes; every output is among
    them, and at least one output word is no longer poison."""
    s = U.step(name)
    for size in s.sizes:
        case = s.case(size)
        ups, outs = s.uploads(case), s.outputs(case)
        assert not set(ups) & set(outs)
        e = s.expected_for(size)
        assert set(outs) <= set(e) <= set(ups) | set(outs), (name, size, sorted(e))
        written = 0
        for k, v in e.items():
            have = np.ascontiguousarray((ups if k in ups else outs)[k])
            assert v.nbytes == have.nbytes, (name, size, k, v.nbytes, have.nbytes)
            written += int((v.reshape(-1).view(np.uint8) != have.reshape(-1).view(np.uint8)).sum())
        assert written > 0, (name, size)
        lists = s.lists(case)
        assert bool(lists) == s.carries_lists
        for k, v in lists.items():
            assert v.flags.c_contiguous and v.flags.writeable and v.dtype in (np.int32, np.uint32, np.float32), (name, k)


@pytest.mark.parametrize("name", [s.name for s in U.table() if s.carries_lists])
def test_other_lists_give_another_answer(name):
    """other_lists() has the shapes and types of lists(), differs from it, and its expected output differs in at least
    one word of an output: a call that read a reused list cannot pass."""
    s = U.step(name)
    for size in ("small", "large"):
        case = s.case(size)
        own, other = s.lists(case), s.other_lists(case)
        assert set(own) == set(other)
        for k in own:
            assert own[k].shape == other[k].shape and own[k].dtype == other[k].dtype, (name, k)
        assert any(own[k].tobytes() != other[k].tobytes() for k in own), name
        a, b = s.expected_for(size), s.expected_for(size, other)
        outs = s.outputs(case)
        assert any(a[k].tobytes() != b[k].tobytes() for k in outs), (name, size)


def test_other_lists_are_valid_arguments():
    """Frames, pairs, images, links and walk entries in range, no frame or image twice where the call forbids it, CHAIN
    and FAN links that still join their pairs, positive focal lengths: a reused list can give wrong bytes, never an
    access out of range."""
    for s in U.table():
        for size in ("small", "large"):
            case = s.case(size)
            o = s.other_lists(case)
            if "frames" in o:
                assert sorted(o["frames"].tolist()) == sorted(case["sel"].tolist())
            if "images" in o:
                assert sorted(o["images"].tolist()) == sorted(np.asarray(case["images"]).tolist())
            if "hold" in o:
                assert (o["hold"] >= 0).all() and (o["hold"] < case["nimages"]).all()
            if "intrinsics" in o:
                k = o["intrinsics"]
                assert np.isfinite(k).all() and (k.reshape(len(k), -1)[:, :2] > 0).all()
                assert k.shape[1] == 4 or (k[:, 4:6] > 0).all()
            if "links" in o:
                assert sorted(map(tuple, o["links"].tolist())) == sorted(map(tuple, np.asarray(case["links"]).tolist()))
                assert sorted(o["walk"].tolist()) == sorted(np.asarray(case["walk"]).tolist())
                assert o["pairs"].tobytes() == np.ascontiguousarray(case["pairs"], np.int32).tobytes()
            elif "pairs" in o:
                p = o["pairs"]
                assert sorted(map(tuple, p.tolist())) == sorted(map(tuple, case["pairs"].tolist()))
                if s.name.startswith(("match_guided", "match_epipolar")):
                    assert len(set(p[:, 0].tolist())) == len(p)          # the rows are written in place: one pair each


class _Recorder:
    """Stands in for the loaded library: every call returns 0 and leaves its arguments behind."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.mark.parametrize("name", [s.name for s in U.table() if s.carries_lists])
def test_the_wrappers_hand_the_library_the_callers_own_lists(name, monkeypatch):
    """The reuse test overwrites the arrays of lists() and relies on the library having been given those very arrays:
    with the library replaced by a recorder, the address of every list is among the arguments of the step's call."""
    from cudasift_amd import capi
    s = U.step(name)
    case = s.case("small")
    rec = _Recorder()
    monkeypatch.setattr(capi, "_lib", rec)
    ctx = object.__new__(capi.Context)
    ctx.h, ctx.device = 1, 0
    dev = {k: 4096 * (n + 1) for n, k in enumerate(list(s.uploads(case)) + list(s.outputs(case)))}
    lists = s.lists(case)
    s.enqueue(ctx, case, dev, lists)
    ctx.h = None
    (called, args), = rec.calls
    assert called == "misift_" + name
    for k, v in lists.items():
        assert v.ctypes.data in args, (name, k)


def _temp(size):
    return {s.name: s.tmp_bytes(s.case(size), U.CUS) for s in U.table() if size in s.sizes}


def test_temp_is_ordered_as_the_sequences_assume():
    """small < large for every step that uses temp, 0 for the two that do not; every huge step above every step at
    small and large, and no two of them equal.  The pair matchers' partials are the same at every size: only their keys
    grow."""
    small, large, huge = _temp("small"), _temp("large"), _temp("huge")
    for s in U.table():
        if s.temp:
            assert 0 < small[s.name] < large[s.name], (s.name, small[s.name], large[s.name])
        else:
            assert small[s.name] == large[s.name] == 0
    most = max(max(small.values()), max(large.values()))
    assert len(huge) == 10 and all(v > most for v in huge.values()), (huge, most)
    assert len(set(huge.values())) == len(huge)                  # in ascending order every one of them makes the temp grow
    for name in ("match_pairs_batch", "match_pairs_batch_i8"):
        s = U.step(name)
        assert s.part_bytes(s.case("small"), U.CUS) == s.part_bytes(s.case("large"), U.CUS) > 2 ** 20
    print("temp bytes:", {k: (small[k], large[k], huge.get(k)) for k in small})


def test_large_covers_every_region_of_small_with_another():
    """For the calls that carve several regions out of the temp, every region of the small layout but the first lies
    wholly in bytes the large layout of the same call uses for other regions.  (The first starts at 0 at any size: it
    lies in what the other calls wrote.)"""
    def regions(name, case):
        if name == "refine_cameras_batch":
            return [4 * case["max_obs"]] * 2
        if name == "resect_cameras_batch":
            n, cap, lp = len(case["images"]), U.align16(min(case["max_cand"], case["max_obs"])), U.align16(case["num_loops"])
            return [4 * case["max_obs"]] * 2 + [20 * cap * n, 24 * lp * n, 48 * lp * n, 4 * lp * n, 16 * n]
        if name == "link_tracks_batch":
            return [U.align16(4 * case["max_records"]), U.align16(16 * len(case["pairs"])), 16 * case["max_records"]]
        if name == "export_tracks_batch":
            return [U.align16(4 * case["max_records"])] * 4 + [8 * ((case["max_records"] + 2047) // 2048)]
        return [12 * len(case["links"]), 8 * len(case["pairs"]), 4 * len(case["walk"]), 4 * len(case["pairs"]) + 16]

    for name in ("refine_cameras_batch", "resect_cameras_batch", "link_tracks_batch", "export_tracks_batch",
                 "link_poses_batch"):
        s = U.step(name)
        a, b = regions(name, s.case("small")), regions(name, s.case("large"))
        assert sum(a) == s.tmp_bytes(s.case("small"), U.CUS) and sum(b) == s.tmp_bytes(s.case("large"), U.CUS), name
        sa, sb = np.concatenate([[0], np.cumsum(a)]), np.concatenate([[0], np.cumsum(b)])
        assert sa[-1] < sb[-1]
        for r in range(1, len(a)):                               # region 0 starts at 0 at any size: other calls cover it
            assert sa[r + 1] <= sb[r] or sa[r] >= sb[r + 1], (name, r, sa.tolist(), sb.tolist())


def test_the_gpu_file_holds_no_tolerance_and_no_literal_ring_size():
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_used_context.py")).read()
    assert not re.search(r"allclose|isclose|approx|rtol|atol|assert_almost", src)
    for line in src.split("\n"):                                # the ring's size comes from the hook, never from a literal
        if re.search(r"ring|slot|RING|SLOT", line):
            assert not re.search(r"(?<![\w.])4(?![\w.])", line), line

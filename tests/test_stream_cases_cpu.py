"""The premises of test_gpu_caller_stream.py, checked without a GPU.  A gated call whose kernels ran early would have
read zero-filled inputs: for every step of used_context.stream_table() the restatement takes such inputs and gives another
answer than for the real ones, so an early kernel cannot be told from a correct one by no buffer at all.  Every output the
call writes differs from its poison, the plans are padded to the ring, and the steps table() does not hold are library
calls only."""
import numpy as np
import pytest

import stream_util as SU
import used_context as U
from test_used_context_cpu import _Recorder

NAMES = [s.name for s in U.stream_table()]
NEW = [s.name for s in U.stream_table() if s not in U.table()]
REQUIRED = ("select_pairs_batch", "adjust_bundle_batch", "adjust_bundle_robust_batch", "adjust_bundle_focal_batch",
            "adjust_bundle_radial_batch", "filter_tracks_batch", "correspond_tracks_batch", "align_points_batch",
            "transform_scene_batch", "merge_scenes_batch", "recover_pose_planar_batch")
# misift_improve_homography_batch is not among them: its GPU file holds it to the device's own single-frame call, and no
# test pins a host restatement of it to the device bit for bit
OPTIONAL = ("match_batch", "quantize_batch", "match_batch_i8", "score_fundamental_batch", "undistort_obs_batch")


def _differ(a, b):
    return np.ascontiguousarray(a).tobytes() != np.ascontiguousarray(b).tobytes()


def test_the_stream_table_is_the_table_and_the_required_calls():
    from cudasift_amd import capi
    assert U.stream_table()[:len(U.table())] == U.table() and tuple(NEW) == REQUIRED + OPTIONAL
    assert len(set(NAMES)) == len(NAMES)
    for n in NEW:
        assert "misift_" + n in capi.SIGNATURES and hasattr(capi.Context, n), n
        assert "small" in U.step(n).sizes and not U.step(n).lists(U.step(n).case("small"))
    assert "misift_ctx_set_stream" in capi.SIGNATURES and hasattr(capi.Context, "set_stream")


@pytest.mark.parametrize("name", NAMES)
def test_zero_filled_inputs_give_another_answer(name):
    """The restatement runs on the case with every device input zero-filled (the host lists as they are), names the same
    buffers at the same sizes, and differs from the real answer in at least one buffer the call writes."""
    s = U.step(name)
    case = s.case("small")
    lists = s.lists(case)
    zero = s.zeroed(case)
    for k, v in s.uploads(zero).items():
        assert not np.ascontiguousarray(v).view(np.uint8).any(), (name, k)
        assert np.ascontiguousarray(v).nbytes == np.ascontiguousarray(s.uploads(case)[k]).nbytes, (name, k)
    with np.errstate(all="ignore"):
        early = s.expected(zero, lists)
    real = s.expected_for("small")
    assert set(early) == set(real), (name, set(early) ^ set(real))
    for k in real:
        assert np.ascontiguousarray(early[k]).nbytes == real[k].nbytes, (name, k)
    assert any(_differ(early[k], real[k]) for k in real), name


@pytest.mark.parametrize("name", NAMES)
def test_every_written_output_differs_from_its_poison(name):
    """An output the call left alone cannot pass for one it wrote; and what expected() names beyond the outputs is an
    input the call writes in place, which differs from what is staged."""
    s = U.step(name)
    case = s.case("small")
    ups, outs = s.uploads(case), s.outputs(case)
    assert not set(ups) & set(outs)
    e = s.expected_for("small")
    assert set(outs) <= set(e) <= set(ups) | set(outs), (name, sorted(e))
    for k in outs:
        assert e[k].nbytes == outs[k].nbytes and _differ(e[k], outs[k]), (name, k)


@pytest.mark.parametrize("ring", range(1, 9))
def test_the_padded_plan_is_a_multiple_of_the_ring(ring):
    plans = [[(s, "small") for s in U.stream_table()], [(s, "small") for s in U.stream_table()][::-1],
             [(U.step("triangulate_tracks_batch"), "small"), (U.step("refine_cameras_batch"), "small")],
             [(U.step("link_tracks_batch"), "small")] * (2 * ring + 1)]
    for plan in plans:
        p = SU.padded(plan, ring)
        assert SU.takers(p) % ring == 0 and 0 <= len(p) - len(plan) < ring and p[:len(plan)] == plan
        assert all(size == "small" and s.takes_slot for s, size in p[len(plan):])
        parts = SU.segments([s for s, _ in p], ring)             # the gates: every call once, at most `ring` slots each
        assert [a for a, _ in parts] == [0] + [b for _, b in parts[:-1]] and parts[-1][1] == len(p)
        assert all(0 < SU.takers(p[a:b]) <= ring for a, b in parts)
    assert [s.name for s in U.stream_table() if not s.takes_slot] == ["quantize_batch"]


@pytest.mark.parametrize("name", NEW)
def test_enqueue_is_one_library_call(name, monkeypatch):
    """With the library replaced by a recorder: enqueue() of a step that table() does not hold makes exactly the call it
    is named after, on the device buffers it was given (no allocation, no copy, no synchronisation besides)."""
    from cudasift_amd import capi
    s = U.step(name)
    case = s.case("small")
    rec = _Recorder()
    monkeypatch.setattr(capi, "_lib", rec)
    ctx = object.__new__(capi.Context)
    ctx.h, ctx.device = 1, 0
    dev = {k: 4096 * (n + 1) for n, k in enumerate(list(s.uploads(case)) + list(s.outputs(case)))}
    s.enqueue(ctx, case, dev, s.lists(case))
    ctx.h = None
    (called, args), = rec.calls
    assert called == "misift_" + name
    for k, p in dev.items():
        assert p in args, (name, k)


def test_the_gpu_file_holds_no_tolerance_and_no_literal_ring_size():
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    for f in ("test_gpu_caller_stream.py", "stream_util.py"):
        src = open(os.path.join(here, f)).read()
        assert not re.search(r"allclose|isclose|approx|rtol|atol|assert_almost", src), f
        assert "hipStreamCreateWithFlags" not in src or "NON_BLOCKING" in src

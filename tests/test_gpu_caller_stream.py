"""The device batch calls on a caller's own non-blocking stream, and across misift_ctx_set_stream.

include/misift.h promises of every batch call that it "runs on the context stream and returns before the GPU work is
done", with "no host synchronisation and no host read", and callers chain the calls on that promise with nothing read in
between.  Every other GPU file creates its contexts on the NULL stream, where legacy synchronisation hides a memset, a
copy, a launch or a plan upload put on another stream, a fork joined only at misift_ctx_sync, a pinned list read after the
stream has moved on and a stray host wait.  Here every step of used_context.stream_table() runs on a context created on
a stream of the caller's, behind a gate the test put on that stream (stream_util.py says how, and what the premise
asserted on every run shows); every comparison is byte equality with the restatements the calls' own files use.

misift_ctx_set_stream: the context stays one in-order pipeline across a switch.  Before this file it was called by
nothing, and a call on the new stream ran beside (or before) the calls still queued on the old one; docs/LOG.md has what
test_stream_switch_orders_the_new_stream_behind_the_old did on that library."""
import numpy as np
import pytest

import stream_util as SU
import used_context as U
from batch_util import guarded_context

pytestmark = pytest.mark.gpu

MISIFT_EINVAL = -1
# the calls whose kernels read their lists from the pinned ring when they run, not when they are enqueued
READ_WHEN_RUN = ("link_tracks_batch", "link_poses_batch", "triangulate_tracks_batch", "refine_cameras_batch",
                 "resect_cameras_batch")
TRI = dict(min_views=2, num_loops=5)
# two contexts: the gated one's gate has to outlast the other's whole run, its synchronisation and its read-back
TWO_CONTEXT_COPIES = 4 * SU.GATE_COPIES


@pytest.fixture(scope="module")
def gate():
    g = SU.Gate()
    yield g
    g.free()


def _plan(order):
    steps = [(s, "small") for s in U.stream_table()]
    return steps if order == "forward" else steps[::-1]


def test_every_call_behind_a_gate_on_a_caller_stream(gate):
    """The whole table forward on one context; the wait is hipStreamSynchronize of the caller's stream alone, so what
    is compared was complete on that stream."""
    with SU.streams(1) as (S,), guarded_context(1, S) as g:
        run = SU.GatedRun(g, S, _plan("forward"), gate)
        run.warm_up()
        run.gated()
        SU.sync(S)
        run.check("forward")
        # behind the first gate no call waits for a slot of the ring: the host's own enqueue time
        print("host time of the calls behind each gate, ms:", ["%.3f" % (1e3 * t) for t in run.host_s])


def test_every_call_reversed_and_misift_ctx_sync_is_the_wait(gate):
    """The table reversed on a second fresh context and stream; misift_ctx_sync is the wait, and the last gate is over
    when it returns.  Then once more with the per-kernel profile on: LaunchScope records events on the stream."""
    with SU.streams(1) as (S,), guarded_context(1, S) as g:
        run = SU.GatedRun(g, S, _plan("reversed"), gate)
        run.warm_up()
        run.gated()
        g.sync()
        assert SU.ready(run.done[-1])
        run.check("reversed")
        g.profile_enable(True)
        try:
            run.warm_up()                                        # the first profiled pass creates the events it records
            run.gated()
            g.sync()
            assert SU.ready(run.done[-1])
            run.check("reversed, profiled")
        finally:
            g.profile_enable(False)


def test_host_lists_reused_behind_the_gate(gate):
    """More list-carrying calls than twice the ring, the ones that read the pinned copy when they run first; every list
    is overwritten in place with another valid list as soon as its call has returned, while the call is still behind
    the gate.  Every output is the answer to the lists as they were at the call."""
    carriers = [U.step(n) for n in READ_WHEN_RUN]
    carriers += [s for s in U.table() if s.carries_lists and s not in carriers]
    with SU.streams(1) as (S,), guarded_context(1, S) as g:
        count = 2 * g.test_state(SU.RING_SLOTS) + 1
        run = SU.GatedRun(g, S, [(carriers[n % len(carriers)], "small") for n in range(count)], gate)
        assert len(run.bufs) > 2 * run.ring
        run.warm_up()
        run.gated(reuse_lists=True)
        SU.sync(S)
        run.check("reused lists")
        for b in run.bufs:                                       # the lists were rewritten: the premise of the check
            assert any(b.lists[k].tobytes() != b.at_call[k].tobytes() for k in b.lists) or not b.lists


def test_two_contexts_on_two_streams(gate):
    """Context A on S1 behind a gate, context B on S2 ungated, a call on the one between any two of the other.  B is
    synchronised, read back and compared while A's gate is still running: B's work does not sit behind A's stream."""
    steps = [s for s in U.stream_table() if s.takes_slot]        # one gate: as many calls as the ring has slots
    with SU.streams(2) as (S1, S2), guarded_context(1, S1) as a, guarded_context(1, S2) as b:
        ring = a.test_state(SU.RING_SLOTS)
        ra = SU.GatedRun(a, S1, [(s, "small") for s in steps[:ring]], gate)
        rb = SU.GatedRun(b, S2, [(s, "small") for s in steps[::-1][:ring]], gate)
        assert len(ra.bufs) == len(rb.bufs) == ring
        ra.warm_up()
        rb.warm_up()
        done = gate.put(S1, TWO_CONTEXT_COPIES, ra.done[0])
        for x, y in zip(ra.bufs, rb.bufs):
            x.run(S1)
            y.run(S2)
        assert not SU.ready(done), "A's gate was over when the last call returned"
        SU.sync(S2)
        rb.check("context B")
        assert not SU.ready(done), "A's gate was over when B had been synchronised and compared"
        SU.sync(S1)
        ra.check("context A")


# ---- misift_ctx_set_stream

class _Triangulate(U.Triangulate):
    """The triangulation of the scene the refine step's `small` case is made of."""
    sizes = ("small",)

    def build(self, size):
        return dict(U.step("refine_cameras_batch").case("small"), memo={}, **TRI)


class _RefineBehind(U.Refine):
    """misift_refine_cameras_batch on that scene with the points and their status the triangulation's restatement gives:
    what the call finds in the triangulation's own output buffers."""
    sizes = ("small",)

    def __init__(self, tri):
        super().__init__()
        self.tri = tri

    def build(self, size):
        e = self.tri.expected_for("small")
        return dict(U.step("refine_cameras_batch").case("small"), points=e["points"].view(U.f32).reshape(-1, 4),
                    point_status=e["point_status"].view(np.int32))


def _switch_run(gate, first, second, alias, to_second_stream=True):
    """Gate on S1; `first` staged, called and copied out on S1; `second`'s own inputs staged on S1; the switch; `second`
    called through the context and copied out on the stream the context is on now, and the pads behind it.  Only that
    stream is synchronised before `second` is compared."""
    with SU.streams(2) as (S1, S2), guarded_context(1, S1) as g:
        S = S2 if to_second_stream else S1
        try:
            a = SU.GatedBufs(g, first, "small")
            b = SU.GatedBufs(g, second, "small", alias={k: a.dev[k] for k in alias})
            plan = SU.padded([(first, "small"), (second, "small")], g.test_state(SU.RING_SLOTS))
            pads = [SU.GatedBufs(g, s, size) for s, size in plan[2:]]
            done = gate.event()
            for x in [a, b] + pads:                              # the warm-up: the same calls ungated, on one stream
                x.run(S1)
            for x in [a, b] + pads:
                x.reset(S1)
            SU.sync(S1)
            tmp, slots = g.test_state(SU.TEMP_BYTES), g.test_state(SU.SLOTS_HANDED_OUT)
            gate.put(S1, SU.GATE_COPIES, done)
            a.run(S1)
            b.stage(S1)
            g.set_stream(S)
            b.enqueue()
            b.copy_out(S)
            for x in pads:
                x.run(S)
            assert not SU.ready(done), "the gate was over when the last call returned: set_stream or a call waited"
            assert g.test_state(SU.TEMP_BYTES) == tmp and g.test_state(SU.SLOTS_HANDED_OUT) == slots + 2 + len(pads)
            SU.sync(S)
            b.check("behind the switch")
            for x in pads:
                x.check("behind the switch, pad")
            SU.sync(S1)
            a.check("before the switch")
        finally:
            SU.sync(S1)
            SU.sync(S2)


def test_stream_switch_orders_the_new_stream_behind_the_old(gate):
    """triangulate on S1 behind the gate, misift_ctx_set_stream(S2), refine through the context on S2: its points and
    their status are the triangulation's output buffers and its other inputs are staged on S1 behind the gate, so it is
    right only if S2 starts behind everything the context enqueued on S1.  Only S2 is synchronised."""
    tri = _Triangulate()
    _switch_run(gate, tri, _RefineBehind(tri), ("points", "point_status"))


@pytest.mark.parametrize("name", ["link_tracks_batch", "find_fundamental_batch"])
def test_stream_switch_with_the_shared_temp_on_both_sides(gate, name):
    """The same step at `small` twice on different buffers, one before the switch and one behind it: both lay the same
    format over the context's one temp, and both are right."""
    _switch_run(gate, U.step(name), U.step(name), ())


def test_switch_to_the_stream_the_context_is_on(gate):
    """A no-op: nothing is recorded or waited for, and the results are right."""
    tri = _Triangulate()
    _switch_run(gate, tri, _RefineBehind(tri), ("points", "point_status"), to_second_stream=False)


def test_set_stream_arguments_and_back_and_forth():
    """A NULL context is MISIFT_EINVAL.  S1 -> S2 -> S1 -> the NULL stream, a call before every switch, nothing
    synchronised in between; then the table's `small` steps on the NULL stream come out right."""
    from cudasift_amd import capi
    assert capi.lib().misift_ctx_set_stream(None, None) == MISIFT_EINVAL
    with SU.streams(2) as (S1, S2), guarded_context(1, S1) as g:
        assert capi.lib().misift_ctx_set_stream(None, S2) == MISIFT_EINVAL
        hops = [U.Bufs(g, U.step(n), "small") for n in ("link_tracks_batch", "resect_cameras_batch", "link_tracks_batch")]
        after = [U.Bufs(g, s, "small") for s in U.table()]
        for b, s in zip(hops, (S2, S1, None)):
            b.enqueue()
            g.set_stream(s)
        for b in after:
            b.enqueue()
        g.sync()
        SU.sync(S1)
        SU.sync(S2)
        for n, b in enumerate(hops + after):
            b.check("after the switches, call %d" % n)

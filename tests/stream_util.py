"""The batch calls on a caller's own non-blocking stream, behind a gate (test_gpu_caller_stream.py; the premises are
asserted without a GPU in test_stream_cases_cpu.py).  No tests in here, and cudasift_amd.capi is imported inside functions
only.

Every other GPU file creates its contexts on the NULL stream, where legacy synchronisation orders whatever the library
puts on a wrong stream.  Here the context is created on a stream from hipStreamCreateWithFlags(hipStreamNonBlocking), and
the test makes that stream busy with work of its own before it calls the library:

  the gate     GATE_COPIES device-to-device copies between two scratch buffers of GATE_BYTES, enqueued by the test with
               hipMemcpyAsync, and an event recorded behind them.  Finite copy work: it cannot hang, and it is no library
               call, since where the library puts its work is what is under test.
  behind it    per step, all on the caller's stream: every output poisoned again from a device copy of its poisoned
               content (an early memset on a wrong stream is overwritten, a late atomic lands on poison), the staged
               inputs copied over the live ones, the library call, and every buffer the call writes copied to a result
               buffer of its own (so completion is ordered on the stream itself, not only at misift_ctx_sync).
  the premise  right after the last call behind a gate has returned, hipEventQuery of the gate's event is NOT READY: every
               one of those calls was enqueued and returned while its inputs were not there yet, and none of them waited
               for the stream.  It is asserted on every run; a run in which it fails is a failed test.

A live input is what the call is handed.  It holds zeros from upload until the stage copy behind the gate runs: count 0,
offset 0, T = O = 0, no camera, a valid and empty input for every call, so that a kernel that ran early addresses nothing
and merely gives another answer (test_stream_cases_cpu.py: another answer in at least one written buffer).  The poison
word is not used for inputs: as an offset it would be a wild index.

One gate covers at most as many calls as the pinned ring has slots (misift_test_ctx_state(ctx, 1)).  Every batch call
but misift_quantize_batch takes the next slot of the ring and waits on the host for the call that last used it
(mb_ring_slot in misift_host.hip), so the call one ring behind the first call of a gate has to have run before that call
can return, and with it the gate in front of it: a plan that takes more slots than the ring has gets a gate in front of
every `ring` slots' worth of calls, each with its own premise.  The first call behind a later gate blocks until the gate
before it is over; its own gate is enqueued before it and starts after it.

Warm-up.  Growing the temp, a ring slot or the pair plan waits for the stream by design (a slot that grows frees its
pinned memory, which waits for the whole device), so the same plan runs once ungated on the same context first, padded
with `small` steps until it takes a multiple of the ring's slots: every call lands in the same slot in both passes.
Behind the warm-up every live input is zero-filled, every live output poisoned and every result buffer filled with junk
again, and the stream synchronised, before the first gate: a call that ran early must not find the inputs the warm-up
staged, nor its results the warm-up's.  The gated pass asserts that the temp did not change and that the ring counter
advanced by one per call that takes a slot.

Between the first gate and the final synchronisation the test allocates, reads, uploads and synchronises nothing."""
import contextlib
import ctypes as C
import time

import numpy as np

import used_context as U

NOT_READY = 600                                                  # hipErrorNotReady
D2D = 3                                                          # hipMemcpyDeviceToDevice
NON_BLOCKING, DISABLE_TIMING = 1, 2                              # hipStreamNonBlocking, hipEventDisableTiming
TEMP_BYTES, RING_SLOTS, SLOTS_HANDED_OUT = 0, 1, 2               # misift_test_ctx_state
JUNK = 0xEE                                                      # what a result buffer holds until the copy-out has run
GATE_BYTES = 512 << 20
GATE_COPIES = 48                                                 # docs/LOG.md: measured against the host's enqueue time

_hip = None


def hip():
    """The HIP runtime libmisift itself is bound to (capi.hip_runtime).  C.CDLL("libamdhip64.so") is not it in every
    process: once torch has been imported behind libmisift (the whole suite does), that name is torch's bundled runtime,
    a second one, and a stream created by the one aborts inside the other."""
    global _hip
    if _hip is None:
        from cudasift_amd import capi
        h = capi.hip_runtime()
        vp, pvp = C.c_void_p, C.POINTER(C.c_void_p)
        for name, args in dict(hipStreamCreateWithFlags=[pvp, C.c_uint], hipStreamDestroy=[vp], hipStreamSynchronize=[vp],
                               hipMemcpyAsync=[vp, vp, C.c_size_t, C.c_int, vp], hipEventCreateWithFlags=[pvp, C.c_uint],
                               hipEventCreate=[pvp], hipEventRecord=[vp, vp], hipEventQuery=[vp], hipEventSynchronize=[vp],
                               hipEventElapsedTime=[C.POINTER(C.c_float), vp, vp], hipEventDestroy=[vp]).items():
            getattr(h, name).argtypes, getattr(h, name).restype = args, C.c_int
        _hip = h
    return _hip


def ok(rc, what):
    assert rc == 0, "%s failed: hipError %d" % (what, rc)


@contextlib.contextmanager
def streams(n):
    """n non-blocking streams (a blocking one would synchronise with the NULL stream and hide what these tests are for),
    as raw hipStream_t values.  They are drained and destroyed when the body ends: the contexts that use them are opened,
    and so closed, inside it."""
    made = []
    try:
        for _ in range(n):
            s = C.c_void_p()
            ok(hip().hipStreamCreateWithFlags(C.byref(s), NON_BLOCKING), "hipStreamCreateWithFlags")
            made.append(s.value)
        yield made
    finally:
        for s in made:
            hip().hipStreamSynchronize(s)
            hip().hipStreamDestroy(s)


def sync(stream):
    ok(hip().hipStreamSynchronize(stream), "hipStreamSynchronize")


def copy(dst, src, nbytes, stream):
    if nbytes:
        ok(hip().hipMemcpyAsync(dst.ptr, src.ptr, nbytes, D2D, stream), "hipMemcpyAsync")


class Gate:
    """Two scratch buffers and an event.  put(stream) enqueues the copies and records the event behind them; ready() is
    hipEventQuery of that record.  One Gate serves a whole module: its work is ordered by the streams it is put on."""

    def __init__(self, timing=False):
        from cudasift_amd import capi
        self.a, self.b = capi.DevBuf(GATE_BYTES), capi.DevBuf(GATE_BYTES)
        self.events = []
        self.timing = timing

    def event(self):
        e = C.c_void_p()
        if self.timing:
            ok(hip().hipEventCreate(C.byref(e)), "hipEventCreate")
        else:
            ok(hip().hipEventCreateWithFlags(C.byref(e), DISABLE_TIMING), "hipEventCreateWithFlags")
        self.events.append(e.value)
        return e.value

    def put(self, stream, copies=GATE_COPIES, done=None):
        """Returns the event recorded behind the copies (`done`, or a new one: events are created before a gated pass)."""
        for i in range(copies):
            copy(self.b if i % 2 == 0 else self.a, self.a if i % 2 == 0 else self.b, GATE_BYTES, stream)
        done = self.event() if done is None else done
        ok(hip().hipEventRecord(done, stream), "hipEventRecord")
        return done

    def free(self):
        for e in self.events:
            hip().hipEventDestroy(e)
        self.events = []
        self.a.free()
        self.b.free()


def ready(event):
    rc = hip().hipEventQuery(event)
    assert rc in (0, NOT_READY), "hipEventQuery: hipError %d" % rc
    return rc == 0


def _bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class GatedBufs(U.Bufs):
    """One step on a context for a gated pass: the live buffers the call is handed (inputs zero-filled, outputs poisoned),
    a staged device copy of every one of them as U.Bufs would have uploaded it (the inputs' real content, the outputs'
    poisoned content: the calls' outputs are poisoned with two patterns, so each output is poisoned again from its own
    copy), and a poisoned result buffer per buffer the call writes.  `alias` names inputs that are another step's live
    outputs: they are handed over as they are and neither zero-filled nor staged.  Everything is allocated and uploaded
    here, before any gate."""

    def __init__(self, ctx, step, size, alias=None):
        self.ctx, self.step, self.size, self.case = ctx, step, size, step.case(size)
        self.alias = dict(alias or {})
        ups = {k: np.ascontiguousarray(v) for k, v in step.uploads(self.case).items()}
        outs = step.outputs(self.case)
        assert not set(ups) & set(outs) and set(self.alias) <= set(ups)
        self.host = dict(ups, **outs)
        self.inputs, self.outputs = tuple(k for k in ups if k not in self.alias), tuple(outs)
        self.staged = {k: ctx.upload(self.host[k]) for k in self.inputs + self.outputs}
        self.dev = dict(self.alias)
        self.dev.update({k: ctx.upload(np.zeros(max(ups[k].nbytes, 1), np.uint8)) for k in self.inputs})
        self.dev.update({k: ctx.upload(outs[k]) for k in self.outputs})
        self.lists = step.lists(self.case)
        self.at_call = None
        self.written = tuple(step.expected_for(size, self.lists))
        assert set(self.outputs) <= set(self.written) <= set(self.host), (step.name, self.written)
        self.result = {k: ctx.upload(np.full(self.host[k].nbytes, JUNK, np.uint8)) for k in self.written}
        self.zero = ctx.upload(np.zeros(max([ups[k].nbytes for k in self.inputs] + [1]), np.uint8))
        self.junk = ctx.upload(np.full(max([self.host[k].nbytes for k in self.written] + [1]), JUNK, np.uint8))

    def reset(self, stream):
        """Behind a warm-up and in front of a gate (the caller synchronises): the live inputs zero-filled, the live outputs
        poisoned and the result buffers filled with junk again, as they were uploaded.  Without it a call that ran early
        would find the inputs the warm-up staged, and its results would already be there."""
        for k in self.inputs:
            copy(self.dev[k], self.zero, self.host[k].nbytes, stream)
        for k in self.outputs:
            copy(self.dev[k], self.staged[k], self.host[k].nbytes, stream)
        for k in self.written:
            copy(self.result[k], self.junk, self.host[k].nbytes, stream)

    def stage(self, stream):
        """Every output poisoned again, then the staged inputs over the live ones."""
        for k in self.outputs + self.inputs:
            copy(self.dev[k], self.staged[k], self.host[k].nbytes, stream)

    def copy_out(self, stream):
        for k in self.written:
            copy(self.result[k], self.dev[k], self.host[k].nbytes, stream)

    def run(self, stream):
        """stage, the library call, copy-out: library calls and the test's own asynchronous copies only."""
        self.stage(stream)
        self.enqueue()
        self.copy_out(stream)

    def check(self, what):
        """Byte equality of every result buffer with the restatement under the lists as they were at the call, of the live
        buffer it was copied from too, and of every live buffer the call must not write with what was staged."""
        exp = self.step.expected_for(self.size, self.at_call)
        for where, k in [("result", k) for k in self.written] + [("live", k) for k in self.host]:
            up = self.host[k]
            want = _bytes(exp.get(k, up))
            assert want.nbytes == up.nbytes, (self.step.name, k, want.nbytes, up.nbytes)
            if k in self.alias and k not in exp:                 # another step's output: that step's check holds it
                continue
            got = self.ctx.download(self.result[k] if where == "result" else self.dev[k], (want.nbytes,), np.uint8)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, "%s: %s %s, %s (%s): %d bytes differ, first at %s" % (
                what, self.step.name, self.size, k, where, len(bad), bad[:8])


def takers(plan):
    """The calls of a plan that take a slot of the pinned ring: all but misift_quantize_batch, which has no host side
    beyond its launch."""
    return sum(1 for s, _ in plan if s.takes_slot)


def padded(plan, ring):
    """The plan with `small` steps behind it until its calls take a multiple of `ring` slots: the next pass of the same
    plan then finds every call in the slot it had, which holds its lists without growing (growing frees the slot's pinned
    memory, and that waits for the device)."""
    pads = [s for s in U.table() if not s.temp] + [U.step("find_homography_batch")]
    plan = list(plan)
    for n in range(-takers(plan) % ring):
        plan.append((pads[n % len(pads)], "small"))
    assert takers(plan) % ring == 0 and all(s.takes_slot for s in pads)
    return plan


def segments(steps, ring):
    """Ranges [a, b) of a plan such that the calls of one range take at most `ring` slots: what one gate covers."""
    out, a, used = [], 0, 0
    for n, s in enumerate(steps):
        if s.takes_slot and used == ring:
            out.append((a, n))
            a, used = n, 0
        used += int(s.takes_slot)
    return out + [(a, len(steps))] if a < len(steps) else out


class GatedRun:
    """A plan of (step, size) on one context whose stream is `stream`: warm_up() runs it ungated, gated() behind a gate
    in front of every `ring` slots' worth of calls with the premise asserted per gate, check() compares."""

    def __init__(self, ctx, stream, plan, gate):
        self.ctx, self.stream, self.gate = ctx, stream, gate
        self.ring = ctx.test_state(RING_SLOTS)
        assert self.ring >= 1
        plan = padded(plan, self.ring)
        self.bufs = [GatedBufs(ctx, s, size) for s, size in plan]
        self.parts = segments([s for s, _ in plan], self.ring)
        self.slots = takers(plan)
        self.done = [gate.event() for _ in self.parts]
        self.host_s = []                                         # the host time of the calls behind each gate

    def warm_up(self):
        for b in self.bufs:
            b.run(self.stream)
        for b in self.bufs:
            b.reset(self.stream)
        sync(self.stream)

    def gated(self, reuse_lists=False, copies=GATE_COPIES):
        tmp, slots = self.ctx.test_state(TEMP_BYTES), self.ctx.test_state(SLOTS_HANDED_OUT)
        assert slots % self.ring == 0, "the pass does not start at the first slot of the ring"
        for n, (a, b) in enumerate(self.parts):
            self.gate.put(self.stream, copies, self.done[n])
            t0 = time.perf_counter()
            for x in self.bufs[a:b]:
                x.run(self.stream)
                if reuse_lists:
                    x.overwrite_lists()
            self.host_s.append(time.perf_counter() - t0)
            assert not ready(self.done[n]), "the gate in front of calls %d to %d was over when the last of them returned " \
                "(%s, %.3f ms on the host): a call waited for the stream, or the gate is too short" % (
                    a, b - 1, [x.step.name for x in self.bufs[a:b]], 1e3 * self.host_s[-1])
        assert self.ctx.test_state(TEMP_BYTES) == tmp, "the temp grew in the gated pass"
        assert self.ctx.test_state(SLOTS_HANDED_OUT) == slots + self.slots      # one per call that takes one

    def check(self, what):
        for n, b in enumerate(self.bufs):
            b.check("%s, call %d of %d" % (what, n + 1, len(self.bufs)))

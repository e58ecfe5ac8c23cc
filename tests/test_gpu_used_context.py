"""The geometry-chain batch calls on a context other calls have used.

Every other GPU file opens a fresh guarded context per module, so each call meets the context's shared state in its
kindest form: a temp buffer that holds guard poison or what the same call wrote at the same layout, a pinned ring of host
lists nobody else has filled, one context per process.  Here the steps of used_context.table() (one per call, built from
the cases and restatements of the call's own test file) run back to back on one context, at changing sizes, as library
calls only: every buffer is uploaded first, nothing is read and nothing synchronised by the test until all are enqueued.
Every comparison is byte equality with the existing restatements, of every output and of every input a call must not
write.  The premises the sequences rest on are asserted through misift_test_ctx_state as host state: the temp holds
exactly the bytes used_context.tmp_bytes() predicts after every call, so it grows where the sequence means it to and
nowhere else, and every call takes one slot of the ring.  test_used_context_cpu.py asserts, without a GPU,
that the expected answers are well formed, that a reused list gives another answer, and how the temp sizes are ordered."""
import numpy as np
import pytest

import used_context as U
from batch_util import POISON_WORD, guarded_context, num_cus

pytestmark = pytest.mark.gpu

TEMP_BYTES, RING_SLOTS, SLOTS_HANDED_OUT = 0, 1, 2               # misift_test_ctx_state
BUSY_LOOPS = 4000                                                # of the search that keeps the stream busy
HUGE = {"forward": "refine_cameras_batch", "reversed": "link_tracks_batch"}       # the call that makes the temp grow
# the calls whose kernels read their lists from the pinned ring when they run, not when they are enqueued
READ_WHEN_RUN = ("link_tracks_batch", "link_poses_batch", "triangulate_tracks_batch", "refine_cameras_batch",
                 "resect_cameras_batch")


def _ordered(order):
    steps = list(U.table())
    return steps if order == "forward" else steps[::-1]


class _Run:
    """A plan of (step, size) on one context: every buffer uploaded at once, then the calls one by one with the premises
    checked on host state after each, then every buffer compared."""

    def __init__(self, ctx, plan, ncu):
        self.ctx, self.ncu = ctx, ncu
        self.bufs = [U.Bufs(ctx, s, size) for s, size in plan]
        self.tmp, self.slots, self.grew = ctx.test_state(TEMP_BYTES), ctx.test_state(SLOTS_HANDED_OUT), []
        self.at = 0

    def enqueue_next(self, reuse_lists=False):
        b = self.bufs[self.at]
        b.enqueue()
        if reuse_lists:                                          # the library was given these very arrays: pinned without
            b.overwrite_lists()                                  # a GPU in test_used_context_cpu.py, wrapper by wrapper
        now = self.ctx.test_state(TEMP_BYTES)
        assert now == max(self.tmp, b.step.tmp_bytes(b.case, self.ncu)), (b.step.name, b.size, self.tmp, now)
        if now > self.tmp:
            self.grew.append(self.at)
        self.tmp = now
        self.slots += 1                                          # every batch call takes one, with or without a list
        assert self.ctx.test_state(SLOTS_HANDED_OUT) == self.slots, (b.step.name, b.size)
        self.at += 1

    def enqueue_all(self, **kw):
        while self.at < len(self.bufs):
            self.enqueue_next(**kw)

    def check(self, what):
        for n, b in enumerate(self.bufs):
            b.check("%s, call %d of %d" % (what, n + 1, len(self.bufs)))


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_every_call_on_stale_temp(order):
    """Every call at `large`; every call at `small` in the other order; each call at `large` with the same call at
    `small` right behind it (the same format at shifted offsets); one `huge` call of the chain (refine, or link_tracks in
    the reversed order), for which the library has to wait for the stream and replace the temp with work in flight;
    every call at `small` again, on the fresh allocation."""
    steps, ncu = _ordered(order), num_cus()
    plan = [(s, "large") for s in steps] + [(s, "small") for s in steps[::-1]]
    for s in steps:
        plan += [(s, "large"), (s, "small")]
    huge_at = len(plan)
    plan += [(U.step(HUGE[order]), "huge")] + [(s, "small") for s in steps]
    with guarded_context(1) as g:
        run = _Run(g, plan, ncu)
        g.sync()
        assert run.tmp == 0 and run.slots == 0                   # the uploads used neither the temp nor the ring
        run.enqueue_all()
        g.sync()
        run.check(order)
        ring = g.test_state(RING_SLOTS)
        assert run.slots > 2 * ring
        # the temp grew while the first round found its size, then exactly once more: at the huge step
        assert [n for n in run.grew if n >= len(steps)] == [huge_at], (run.grew, huge_at)
        assert run.tmp == plan[huge_at][0].tmp_bytes(run.bufs[huge_at].case, ncu)


def test_every_huge_call_grows_the_temp_with_work_in_flight():
    """Every call that has a `huge` case, in ascending order of the temp it asks for, each with its own `small` case
    right behind it: ten times the library waits for a stream on which another call's work is queued, frees the temp and
    allocates a larger one, and the small call finds its layout in fresh, guard-poisoned memory.  Which calls grew the
    temp is asserted: every huge one and, behind the first, no other."""
    ncu = num_cus()
    steps = sorted((s for s in U.table() if "huge" in s.sizes), key=lambda s: s.tmp_bytes(s.case("huge"), ncu))
    plan = []
    for s in steps:
        plan += [(s, "huge"), (s, "small")]
    with guarded_context(1) as g:
        run = _Run(g, plan, ncu)
        g.sync()
        run.enqueue_all()
        g.sync()
        run.check("huge, ascending")
        assert run.grew == list(range(0, len(plan), 2)) and len(steps) > 2, (run.grew, [s.name for s in steps])


def test_host_lists_may_be_reused_at_once():
    """Behind a search that keeps the stream busy for milliseconds: more list-carrying calls than twice the ring has
    slots, small lists, then large ones (a reused slot has to grow), then small ones again; the caller overwrites every
    list in place, with another valid list, as soon as the call has returned.  Every output is the answer to the lists
    as they were at the call.  The calls whose kernels read the pinned copy when they run come first, directly behind
    the busy search and before the ring wraps round to its slot: they are the ones still queued when their lists and
    their slots' neighbours are rewritten."""
    carriers = [U.step(n) for n in READ_WHEN_RUN]
    carriers += [s for s in U.table() if s.carries_lists and s not in carriers]
    find = U.step("find_fundamental_batch")
    with guarded_context(1) as g:
        ring = g.test_state(RING_SLOTS)
        assert ring >= 1
        count = 3 * ring + 1
        plan = [(carriers[n % len(carriers)], "large" if ring <= n < 2 * ring else "small") for n in range(count)]
        busy = U.Bufs(g, find, "large")
        run = _Run(g, plan, num_cus())
        g.sync()
        find.enqueue(g, busy.case, busy.dev, busy.lists, loops=BUSY_LOOPS)
        run.tmp, run.slots = g.test_state(TEMP_BYTES), g.test_state(SLOTS_HANDED_OUT)
        assert run.slots == 1
        run.enqueue_all(reuse_lists=True)
        assert run.slots == count + 1 > 2 * ring
        g.sync()
        run.check("reused lists")
        assert (g.download(busy.dev["num"], (len(busy.case["sel"]),), np.uint32) != POISON_WORD).all()


def test_two_contexts_interleaved():
    """Two contexts on one thread, the table at `small` and `large` forward on one and reversed on the other, a call
    on the one between any two of the other: temp, ring and plan belong to the context."""
    ncu = num_cus()
    with guarded_context(1) as a, guarded_context(1) as b:
        fwd = [(s, size) for s in _ordered("forward") for size in ("small", "large")]
        rev = [(s, size) for s in _ordered("reversed") for size in ("large", "small")]
        ra, rb = _Run(a, fwd, ncu), _Run(b, rev, ncu)
        a.sync()
        b.sync()
        for _ in fwd:
            ra.enqueue_next()
            rb.enqueue_next()
        a.sync()
        b.sync()
        ra.check("context A")
        rb.check("context B")
        assert ra.tmp == rb.tmp == max(s.tmp_bytes(s.case("large"), ncu) for s in U.table())
        assert ra.slots == rb.slots > 2 * a.test_state(RING_SLOTS)


# ---- the chain

RESECT = dict(num_loops=100, thresh=4.0, min_inliers=12, only_unset=0, install=0)
REFINE = dict(min_obs=6, num_loops=5, max_error=U.INF, orthonormalise=1)
TRI = dict(min_views=2, num_loops=5)


class _Chain:
    """find -> improve -> recover_pose -> link_poses -> link_tracks -> export -> triangulate -> refine -> resect on a
    scene of posegraph_cases.planted_scene, every output poisoned at exactly its stated capacity."""

    def __init__(self, sc):
        import pose_cases as PC
        from cudasift_amd import capi
        self.sc = sc
        pc, S = sc["case"], sc["S"]
        self.n, self.npairs, self.nimg = S["n"], len(sc["pairs"]), pc["nimages"]
        n, npairs, nimg = self.n, self.npairs, self.nimg
        self.total, self.mt, self.mo = nimg * n, nimg * n // 3 + 1, nimg * n
        recs = np.zeros(self.total, capi.POINT_DTYPE)
        for i in range(nimg - 1):
            assert tuple(sc["pairs"][i]) == (i, i + 1)
            recs[i * n:(i + 1) * n] = sc["raw"][i]
        last = sc["raw"][nimg - 2]
        for k, mk in (("xpos", "match_xpos"), ("ypos", "match_ypos")):
            recs[k][(nimg - 1) * n + last["match"]] = last[mk]
        self.recs = recs
        self.K = np.tile(np.array(PC.K_A, U.f32), (nimg, 1))
        self.K8 = np.ascontiguousarray(np.tile(sc["K8"], (npairs, 1)), U.f32)
        self.sel, self.seeds = U.i32(range(npairs)), np.array(sc["seeds"], np.uint32)
        self.hold = U.i32([i for i in pc["pairs"][pc["seed_pair"]] if i != pc["root_image"]])
        self.images, self.res_seeds = U.i32(range(nimg))[::-1].copy(), np.arange(nimg, dtype=np.uint32) + 500
        self.pairs, self.links, self.walk = U.i32(pc["pairs"]), U.i32(pc["links"]), U.i32(pc["walk"])
        self.sizes = dict(F=9 * npairs, num=npairs, fit=npairs, pose=12 * npairs, front=npairs, xyz=4 * n * npairs,
                          link_ratio=len(self.links), link_common=len(self.links), pair_scale=npairs, cam=12 * nimg,
                          cam_pair=nimg, link_summary=8, track=self.total, track_len=self.total, track_frames=self.total,
                          track_summary=8, track_offsets=self.mt + 1, track_root=self.mt, obs=4 * self.mo,
                          export_summary=8, points=4 * self.mt, point_views=self.mt, point_status=self.mt,
                          obs_error=self.mo, tri_summary=8, cam_out=12 * nimg, cam_obs=nimg, cam_rms=2 * nimg,
                          cam_steps=nimg, cam_status=nimg, refine_summary=8, res_cam=12 * nimg, res_cand=nimg,
                          res_inliers=nimg, res_status=nimg, resect_summary=8)

    def upload(self, g):
        sc, n = self.sc, self.n
        self.g = g
        self.d = {k: g.upload(U.poisoned(m)) for k, m in self.sizes.items()}
        self.d.update(rows=g.upload(np.concatenate(sc["raw"])), row_counts=g.upload(np.full(self.npairs, n, np.int32)),
                      recs=g.upload(self.recs), counts=g.upload(np.full(self.nimg, n, np.int32)))
        return self

    def enqueue(self):
        """Library calls only."""
        g, d, pc, S, n = self.g, self.d, self.sc["case"], self.sc["S"], self.n
        npairs, nimg, mt, mo = self.npairs, self.nimg, self.mt, self.mo
        gates = dict(min_score=U.GATES[0], max_ambiguity=U.GATES[1], thresh=S["thresh"])
        edge = dict(min_score=U.GATES[0], max_ambiguity=U.GATES[1], max_error=pc["max_error"])
        g.find_fundamental_batch(self.sel, self.seeds, d["rows"], npairs, d["row_counts"], None, n, max_pts=n,
                                 num_loops=S["find_loops"], fundamental=d["F"], num_inliers=d["num"], **gates)
        g.improve_fundamental_batch(self.sel, d["rows"], npairs, d["row_counts"], d["F"], None, n, num_fit=d["fit"],
                                    num_loops=S["improve_loops"], **gates)
        g.recover_pose_batch(self.sel, self.K8, d["rows"], npairs, d["row_counts"], d["F"], None, n, pose=d["pose"],
                             num_front=d["front"], xyz=d["xyz"], **gates)
        g.link_poses_batch(self.pairs, nimg, d["rows"], d["row_counts"], n, d["pose"], d["front"], d["xyz"], self.links,
                           pc["seed_pair"], pc["root_image"], self.walk, min_common=pc["min_common"],
                           link_ratio=d["link_ratio"], link_common=d["link_common"], pair_scale=d["pair_scale"],
                           cam=d["cam"], cam_pair=d["cam_pair"], summary=d["link_summary"], **edge)
        g.link_tracks_batch(self.pairs, d["rows"], d["row_counts"], n, nimg, d["counts"], None, n, max_records=self.total,
                            track=d["track"], track_len=d["track_len"], track_frames=d["track_frames"],
                            summary=d["track_summary"], **edge)
        g.export_tracks_batch(d["recs"], nimg, d["counts"], None, n, max_records=self.total, track=d["track"],
                              track_len=d["track_len"], track_frames=d["track_frames"], min_len=3, consistent_only=1,
                              max_tracks=mt, max_obs=mo, track_offsets=d["track_offsets"], track_root=d["track_root"],
                              obs=d["obs"], record_obs=None, summary=d["export_summary"])
        g.triangulate_tracks_batch(mt, mo, d["track_offsets"], d["obs"], d["export_summary"], nimg, d["cam"],
                                   d["cam_pair"], self.K, points=d["points"], point_views=d["point_views"],
                                   point_status=d["point_status"], obs_error=d["obs_error"], summary=d["tri_summary"],
                                   **TRI)
        g.refine_cameras_batch(mt, mo, d["track_offsets"], d["obs"], d["export_summary"], d["points"], d["point_status"],
                               nimg, d["cam"], d["cam_pair"], self.K, hold=self.hold, cam_out=d["cam_out"],
                               cam_obs=d["cam_obs"], cam_rms=d["cam_rms"], cam_steps=d["cam_steps"],
                               cam_status=d["cam_status"], summary=d["refine_summary"], **REFINE)
        g.resect_cameras_batch(mt, mo, d["track_offsets"], d["obs"], d["export_summary"], d["points"], d["point_status"],
                               nimg, self.K, self.images, self.res_seeds, n, cam=d["cam_out"], cam_pair=d["cam_pair"],
                               res_cam=d["res_cam"], res_cand=d["res_cand"], res_inliers=d["res_inliers"],
                               res_status=d["res_status"], summary=d["resect_summary"], **RESECT)

    def download(self):
        from cudasift_amd import capi
        got = {k: self.g.download(self.d[k], (max(m, 1),), np.uint32) for k, m in self.sizes.items()}
        got["rows"] = self.g.download(self.d["rows"], (self.npairs * self.n,), capi.POINT_DTYPE)
        got["recs"] = self.g.download(self.d["recs"], (self.total,), capi.POINT_DTYPE)
        return got

    def expected(self):
        """Every stage from its restatement, each fed the restatement of the stage before it."""
        import posegraph_cases as G
        import refine_cases as RC
        import resect_cases as C
        import triangulate_cases as TC
        from test_tracks_cpu import expected_tracks
        from test_tracks_export_cpu import expected_export
        sc, pc, n, nimg = self.sc, self.sc["case"], self.n, self.nimg
        e = dict(F=U.u32(sc["F"]), pose=U.u32(pc["pose"]), front=U.u32(pc["num_front"]), xyz=U.u32(pc["xyz"]),
                 rows=pc["rows"], recs=self.recs)
        with np.errstate(all="ignore"):
            link = G.expected_link_poses(pc)
        for k in ("link_ratio", "link_common", "pair_scale", "cam", "cam_pair"):
            e[k] = U.u32(link[k])
        e["link_summary"] = U.u32(link["summary"])
        edge = (U.GATES[0], U.GATES[1], pc["max_error"])
        counts = [n] * nimg
        lab = expected_tracks([tuple(p) for p in self.pairs.tolist()], pc["rows"], pc["row_counts"], n, counts, None, n,
                              self.total, edge, poison=POISON_WORD)
        for k, v in zip(("track", "track_len", "track_frames", "track_summary"), lab):
            e[k] = U.u32(v)
        ex = expected_export(U.xy_bits(self.recs), counts, None, n, self.total, *lab[:3], 3, 1, self.mt, self.mo,
                             POISON_WORD)
        for k, v in zip(("track_offsets", "track_root", "obs", None, "export_summary"), ex):
            if k:
                e[k] = U.u32(v)
        base = dict(max_tracks=self.mt, max_obs=self.mo, track_offsets=ex[0], obs=ex[2].view(TC.OBS_DTYPE),
                    export_summary=ex[4], nimages=nimg, intrinsics=self.K, cam=link["cam"].reshape(-1, 12),
                    cam_pair=link["cam_pair"])
        with np.errstate(all="ignore"):
            tri = TC.expected_triangulate(dict(base, memo={}, **TRI))
        for k in ("points", "point_views", "point_status", "obs_error"):
            e[k] = tri[k]
        e["tri_summary"] = tri["summary"]
        with_points = dict(base, points=tri["points"].view(U.f32).reshape(-1, 4),
                           point_status=tri["point_status"].view(np.int32))
        with np.errstate(all="ignore"):
            ref = RC.expected_refine(dict(with_points, hold=tuple(self.hold.tolist()), **REFINE))
        for k in ("cam_out", "cam_obs", "cam_rms", "cam_steps", "cam_status"):
            e[k] = ref[k]
        e["refine_summary"] = ref["summary"]
        case = C.resect_case(dict(with_points, cam=ref["cam_out"].view(U.f32).reshape(-1, 12)), self.images,
                             seeds=self.res_seeds, max_cand=n, **RESECT)
        with np.errstate(all="ignore"):
            res = C.expected_resect(case)
        for k in ("res_cam", "res_cand", "res_inliers", "res_status"):
            e[k] = res[k]
        e["resect_summary"] = res["summary"]
        self.facts = dict(T=int(ex[4][2]), refine_status=ref["cam_status"].view(np.int32).tolist(),
                          resect_status=res["res_status"].view(np.int32).tolist())
        return e


def test_the_chain_three_times_at_changing_sizes():
    """The eight-camera chain three times on one context with the same chain on a smaller scene (five cameras of 150
    records) between the runs: five runs enqueued back to back, nothing read or synchronised until the last call is in.
    Every stage of every run is byte-equal to its restatement, so the three runs are byte-equal to one another."""
    import posegraph_cases as G
    import resect_cases as C
    big, little = G.planted_scene(), G.planted_scene(seed=33, ncams=5, n=150)
    with guarded_context(1) as g:
        runs = [_Chain(sc).upload(g) for sc in (big, little, big, little, big)]
        g.sync()
        tmp = []
        for r in runs:
            r.enqueue()
            tmp.append(g.test_state(TEMP_BYTES))
        g.sync()
        assert tmp[0] == tmp[-1] and len(set(tmp)) == 1         # the first run sized the temp for all of them
        want = {id(big): runs[0].expected(), id(little): runs[1].expected()}
        got = [r.download() for r in runs]
        for n, (r, have) in enumerate(zip(runs, got)):
            e = want[id(r.sc)]
            for k, v in e.items():
                a = np.ascontiguousarray(have[k]).reshape(-1).view(np.uint8)
                b = np.ascontiguousarray(v).reshape(-1).view(np.uint8)
                assert a.nbytes == b.nbytes, (n, k, a.nbytes, b.nbytes)
                bad = np.nonzero(a != b)[0]
                assert len(bad) == 0, "run %d, %s: %d bytes differ, first at %s" % (n + 1, k, len(bad), bad[:8])
        for k in ("cam_out", "points", "res_cam", "res_status", "res_inliers"):
            assert got[0][k].tobytes() == got[2][k].tobytes() == got[-1][k].tobytes(), k
            assert got[1][k].tobytes() == got[3][k].tobytes(), k
        f = runs[0].facts
        print("chain: T %d, refine status %s, resect status %s" % (f["T"], f["refine_status"], f["resect_status"]))
        assert f["T"] >= 100 and f["resect_status"].count(C.OK) >= runs[0].nimg - 1

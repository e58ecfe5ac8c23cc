"""misift_recover_pose_batch on the device: the relative pose of every selected frame pair from its F and intrinsics, the
cheirality votes, and the two-view depth of every record.

Every comparison is byte equality with pose_cases.expected_pose (pinned in test_pose_cpu.py to the library's host hooks and
to float64): d_pose, d_num_front, d_votes, d_xyz, and every byte of the records, which the call must not write.  The
outputs have exactly the stated capacity and are poisoned first; all allocations of the module are guarded.  The frame
counts are the ones at which the kernel can go wrong: no records, fewer than a wave, the workgroup's 256 threads and one
more, and a third record per thread.  The kernel stages no records on chip, so there is no staging capacity to exceed."""
import numpy as np
import pytest

import pose_cases as PC
from batch_util import POISON_WORD, guarded_context, layout, span
from test_fundamental_cpu import GATES, f32
from test_pose_cpu import (CHAIN_SCENE_R_BOUND, CHAIN_SCENE_T_BOUND, direction_error, rotation_error)

pytestmark = pytest.mark.gpu

MISIFT_OK, MISIFT_EINVAL = 0, -1


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


def _poisoned(ctx, words):
    return ctx.upload(np.full(max(words, 1), POISON_WORD, np.uint32))


_frame = PC.planted_frame


@pytest.fixture(scope="module")
def batch():
    """frame -> records held, device count, F, K8.  Frame 0 holds 40 records under count -1; the last is in no entry."""
    sizes = [40, 0, 1, 7, 8, 255, 256, 257, 513, 30]
    made = [_frame(n, 300 + f, PC.K_B if f % 2 else PC.K_A) for f, n in enumerate(sizes)]
    frames, Fs, Ks = [m[0] for m in made], [m[1] for m in made], [m[2] for m in made]
    counts = [-1] + sizes[1:]
    sel = [8, 3, 0, 6, 1, 5, 2, 7, 4]                            # not in frame order, without frame 9
    with np.errstate(all="ignore"):
        expected = [PC.expected_pose(frames[f], counts[f], Fs[f], Ks[f], *GATES, PC.THRESH) for f in sel]
    return dict(frames=frames, counts=counts, Fs=Fs, Ks=Ks, sel=sel, expected=expected)


def _recover(ctx, sel, K, recs, counts, offs, stride, F, thresh=PC.THRESH, votes=True, xyz=True):
    """The call on outputs of exactly nsel x 12, nsel, nsel x 4 and 4 x records words, poisoned.  Returns (pose, num_front,
    votes or None, xyz as uint32 or None, the records afterwards)."""
    from cudasift_amd import capi
    ns = len(sel)
    d = ctx.upload(recs)
    dc = ctx.upload(np.asarray(counts, np.int32))
    do = ctx.upload(np.asarray(offs, np.int32)) if offs is not None else None
    dF = ctx.upload(np.ascontiguousarray(F, f32).reshape(ns, 9))
    dpose, dfront = _poisoned(ctx, 12 * ns), _poisoned(ctx, ns)
    dvotes = _poisoned(ctx, 4 * ns) if votes else None
    dxyz = _poisoned(ctx, 4 * len(recs)) if xyz else None
    ctx.recover_pose_batch(sel, np.stack(K), d, len(counts), dc, dF, do, stride, pose=dpose, num_front=dfront,
                           votes=dvotes, xyz=dxyz, min_score=GATES[0], max_ambiguity=GATES[1], thresh=thresh)
    ctx.sync()
    assert ctx.download(dF, (ns, 9), f32).tobytes() == np.ascontiguousarray(F, f32).tobytes()
    return (ctx.download(dpose, (ns, 12), f32), ctx.download(dfront, (ns,), np.int32),
            ctx.download(dvotes, (ns, 4), np.int32) if votes else None,
            ctx.download(dxyz, (len(recs), 4), np.uint32) if xyz else None,
            ctx.download(d, (len(recs),), capi.POINT_DTYPE))


def _compare(got, sel, recs, counts, offs, stride, expected, what):
    pose, front, votes, xyz, after = got
    want = np.full((len(recs), 4), POISON_WORD, np.uint32)       # rows of frames not selected stay poisoned
    for i, (f, e) in enumerate(zip(sel, expected)):
        want[span(offs, stride, f, max(counts[f], 0))] = e["xyz"].view(np.uint32)
        assert pose[i].tobytes() == e["pose"].tobytes() and front[i] == e["num_front"], \
            (what, "entry", i, "frame", f, "count", counts[f], front[i], e["num_front"], pose[i], e["pose"])
        assert votes is None or votes[i].tolist() == e["votes"].tolist(), (what, i, f, votes[i], e["votes"])
    if xyz is not None:
        bad = np.nonzero((xyz != want).any(1))[0]
        assert len(bad) == 0, (what, "%d xyz rows differ, first %s" % (len(bad), bad[:8]),
                               xyz[bad[:2]].view(f32), want[bad[:2]].view(f32))
    assert after.tobytes() == recs.tobytes(), (what, "the records were written")


def _laid_out(batch, padded):
    recs, offs, stride = layout(batch["frames"], batch["counts"], padded, min_stride=0, pad_error=-7.0)
    sel = batch["sel"]
    return recs, offs, stride, np.stack([batch["Fs"][f] for f in sel]), [batch["Ks"][f] for f in sel]


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
def test_every_frame_count(g, batch, padded):
    recs, offs, stride, F, K = _laid_out(batch, padded)
    sel, counts = batch["sel"], batch["counts"]
    got = _recover(g, sel, K, recs, counts, offs, stride, F)
    _compare(got, sel, recs, counts, offs, stride, batch["expected"], "padded" if padded else "packed")
    pose, front, votes = got[:3]
    by_frame = {f: i for i, f in enumerate(sel)}
    for f in (0, 1):                                             # count -1 and no records: hypothesis 0, no vote
        assert front[by_frame[f]] == 0 and not votes[by_frame[f]].any() and pose[by_frame[f]].any()
    for f in range(5, 9):                                        # the larger frames: a clear winner
        v = np.sort(votes[by_frame[f]])[::-1]
        assert v[0] >= 0.6 * counts[f] and v[1] <= 0.1 * counts[f], (f, votes[by_frame[f]])
    ks = np.array(K)
    assert (ks[:, :4] != ks[:, 4:]).any(1).any() and (ks[:, :4] == ks[:, 4:]).all(1).any()     # K1 != K2 and K1 == K2


def test_optional_outputs_and_two_runs(g, batch):
    """d_votes and d_xyz NULL, one at a time and both: the other outputs do not change; two runs are identical."""
    recs, offs, stride, F, K = _laid_out(batch, False)
    sel, counts = batch["sel"], batch["counts"]
    full = _recover(g, sel, K, recs, counts, offs, stride, F)
    again = _recover(g, sel, K, recs, counts, offs, stride, F)
    for a, b in zip(full, again):
        assert a.tobytes() == b.tobytes()
    for votes, xyz in ((False, True), (True, False), (False, False)):
        got = _recover(g, sel, K, recs, counts, offs, stride, F, votes=votes, xyz=xyz)
        _compare(got, sel, recs, counts, offs, stride, batch["expected"], "votes %s xyz %s" % (votes, xyz))


def test_hostile_matrices(g):
    """The CPU file's hostile F, each over the same 70 records: the poses, and a depth or a NaN for every record."""
    cases = PC.hostile_matrices()
    recs1, _, _ = _frame(70, 350, PC.K_B)
    fr = [recs1.copy() for _ in cases]
    counts = [len(p) for p in fr]
    recs, offs, stride = layout(fr, counts, False, min_stride=0, pad_error=0.0)
    sel = list(range(len(cases)))[::-1]
    F, K = np.stack([cases[f][1] for f in sel]), [cases[f][2] for f in sel]
    with np.errstate(all="ignore"):
        exp = [PC.expected_pose(fr[f], counts[f], cases[f][1], cases[f][2], *GATES, PC.THRESH) for f in sel]
    assert [e["valid"] for e in exp] == [cases[f][3] == "valid" for f in sel]
    got = _recover(g, sel, K, recs, counts, offs, stride, F)
    _compare(got, sel, recs, counts, offs, stride, exp, "hostile F")
    for i, e in enumerate(exp):
        if not e["valid"]:                                       # twelve zeros, 0, four zeros, NaN rows
            assert not got[0][i].any() and got[1][i] == 0 and not got[2][i].any()
            assert (got[3][span(offs, stride, sel[i], counts[sel[i]])] == PC.NAN_BITS).all()


def test_hostile_frames(g):
    """The CPU file's hostile record sets, one call per threshold."""
    cases = PC.hostile_frames()
    for thresh in sorted({c[4] for c in cases}):
        mine = [c for c in cases if c[4] == thresh]
        fr = [c[1] for c in mine]
        counts = [len(p) for p in fr]
        recs, offs, stride = layout(fr, counts, True, min_stride=0, pad_error=0.0)
        sel = list(range(len(fr)))[::-1]
        F, K = np.stack([mine[f][2] for f in sel]), [mine[f][3] for f in sel]
        with np.errstate(all="ignore"):
            exp = [PC.expected_pose(fr[f], counts[f], mine[f][2], mine[f][3], *GATES, thresh) for f in sel]
        got = _recover(g, sel, K, recs, counts, offs, stride, F, thresh=thresh)
        _compare(got, sel, recs, counts, offs, stride, exp, "hostile records, thresh %g" % thresh)


def test_find_improve_recover_pose(g):
    """The chain on pose_cases.chain_scene(), nothing read in between: byte-equal to the three restatements, and within
    the CPU file's bounds of the planted pose."""
    from cudasift_amd import capi
    c = PC.expected_chain()
    s, n, C = c["scene"], PC.CHAIN["n"], PC.CHAIN
    d, dc = g.upload(s["recs"]), g.upload(np.array([n], np.int32))
    dfit, dpose, dfront, dvotes, dxyz = (_poisoned(g, k) for k in (1, 12, 1, 4, 4 * n))
    gates = dict(min_score=GATES[0], max_ambiguity=GATES[1], thresh=C["thresh"])
    dF, dfound = g.find_fundamental_batch([0], [C["find_seed"]], d, 1, dc, None, n, max_pts=n, num_loops=C["find_loops"],
                                          **gates)
    g.improve_fundamental_batch([0], d, 1, dc, dF, None, n, num_fit=dfit, num_loops=C["improve_loops"], **gates)
    g.recover_pose_batch([0], s["K8"], d, 1, dc, dF, None, n, pose=dpose, num_front=dfront, votes=dvotes, xyz=dxyz,
                         **gates)
    g.sync()
    e = c["pose"]
    assert g.download(dfound, (1,), np.int32)[0] == c["found"] and g.download(dfit, (1,), np.int32)[0] == c["fit"]
    assert g.download(dF, (9,), f32).tobytes() == c["F"].tobytes()
    pose = g.download(dpose, (12,), f32)
    assert pose.tobytes() == e["pose"].tobytes() and g.download(dfront, (1,), np.int32)[0] == e["num_front"]
    assert g.download(dvotes, (4,), np.int32).tolist() == e["votes"].tolist()
    assert g.download(dxyz, (n, 4), np.uint32).tobytes() == e["xyz"].view(np.uint32).tobytes()
    assert g.download(d, (n,), capi.POINT_DTYPE).tobytes() == c["recs"].tobytes()
    assert rotation_error(pose[:9], s["R"]) <= CHAIN_SCENE_R_BOUND
    assert direction_error(pose[9:], s["t"]) <= CHAIN_SCENE_T_BOUND
    depth = g.download(dxyz, (n, 4), f32)[s["inl"]][:, 2:]        # the planted matches: in front of both cameras
    assert (depth > 0).mean() > 0.95


def test_argument_errors_enqueue_nothing(g, batch):
    from cudasift_amd import capi
    L = capi.lib()
    recs = np.concatenate([batch["frames"][3], batch["frames"][4]])          # two frames of 7 and 8 records
    d, dc = g.upload(recs), g.upload(np.array([7, 8], np.int32))
    do = g.upload(np.array([0, 7, 15], np.int32))
    dF = g.upload(np.stack([batch["Fs"][3], batch["Fs"][4]]))
    dpose, dfront, dvotes, dxyz = _poisoned(g, 24), _poisoned(g, 2), _poisoned(g, 8), _poisoned(g, 60)
    fr = np.array([0, 1], np.int32)
    K = np.stack([batch["Ks"][3], batch["Ks"][4]])
    good = dict(ctx=g.h, nsel=2, frames=fr.ctypes.data, K=K.ctypes.data, recs=d.ptr, nframes=2, counts=dc.ptr,
                offsets=do.ptr, stride=0, min_score=0.85, max_ambiguity=0.95, thresh=PC.THRESH, F=dF.ptr, pose=dpose.ptr,
                front=dfront.ptr, votes=dvotes.ptr, xyz=dxyz.ptr)

    def recover(**kw):
        a = dict(good, **kw)
        return L.misift_recover_pose_batch(*[a[k] for k in good])

    lists = [np.array(v, np.int32) for v in ([0, 2], [-1, 1], [1, 1])]
    bad = [dict(ctx=None), dict(nsel=-1), dict(recs=None), dict(counts=None), dict(F=None), dict(thresh=float("nan")),
           dict(thresh=0.0), dict(thresh=-1.0), dict(offsets=None, stride=-1), dict(frames=None), dict(nframes=0)]
    bad += [dict(frames=v.ctypes.data) for v in lists]
    bad += [dict(K=None), dict(pose=None), dict(front=None)]     # the new cases: NULL intrinsics, d_pose, d_num_front
    broken = []
    for entry in (0, 1):
        for col in range(8):
            for v in ((0.0, -1.0, np.nan, np.inf, -np.inf) if col % 4 < 2 else (np.nan, np.inf, -np.inf)):
                k = K.copy()
                k[entry, col] = v
                broken.append(k)
    bad += [dict(K=k.ctypes.data) for k in broken]
    for kw in bad:
        assert recover(**kw) == MISIFT_EINVAL, kw
    assert recover(nsel=0) == MISIFT_OK                          # nothing happens
    assert recover(nsel=0, K=None, pose=None, front=None) == MISIFT_OK
    g.sync()
    for b, k in ((dpose, 24), (dfront, 2), (dvotes, 8), (dxyz, 60)):
        assert (g.download(b, (k,), np.uint32) == POISON_WORD).all()
    assert g.download(d, (len(recs),), capi.POINT_DTYPE).tobytes() == recs.tobytes()
    ok = K.copy()
    ok[0, 2], ok[1, 7] = -5.0, 0.0                               # a principal point may be anything finite
    assert recover(K=ok.ctypes.data) == MISIFT_OK
    assert recover() == MISIFT_OK                                # the same arguments, unbroken
    g.sync()
    front = g.download(dfront, (2,), np.int32)
    assert (front >= 6).all() and (front <= [7, 8]).all(), front
    assert (g.download(dxyz, (60,), np.uint32) != POISON_WORD).all()


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0

"""misift_improve_fundamental_batch on the device: refits of each frame's fundamental matrix over its inliers, then
match_error under the result.

Every comparison is byte equality with test_fundamental_refine_cpu.expected_improve (pinned there to the library's host
hook and to a float64 refit): F, num_fit, the rounds, every match_error and every other byte of the records.  The outputs
have exactly the stated capacity and are poisoned first; all allocations of the module are guarded.  The frame counts are
the ones at which the kernel can go wrong: the fewer-than-8 exits, the slot boundary 256, a second and a third record per
slot, and one record more than the kernel stages on chip."""
import numpy as np
import pytest

from batch_util import POISON_WORD, guarded_context, layout, span
from fundamental_cases import noisy_records as _records, start_F as _start
from test_fundamental_cpu import GATES, expected_find
from test_fundamental_refine_cpu import LOOPS, NOISE, expected_improve, hostile_cases
from test_gpu_fundamental import _multi_view
from test_tracks_cpu import INF, blank_rows, expected_tracks, plant, set_edge, window_pairs

pytestmark = pytest.mark.gpu

MISIFT_OK, MISIFT_EINVAL = 0, -1


def capacity():
    from cudasift_amd import capi
    return capi.lib().misift_test_fundamental_refine_capacity()


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


@pytest.fixture(scope="module")
def batch():
    """frame -> records held, device count, start F.  Frame 0 holds 40 records under count -1; the last is in no entry."""
    sizes = [40, 0, 7, 8, 9, 255, 256, 257, 511, 512, 513, 1025, capacity() + 1, 30]
    frames = [_records(n, f) for f, n in enumerate(sizes)]
    counts = [-1] + sizes[1:]
    starts = [_start(p, f) for f, p in enumerate(frames)]
    sel = [12, 3, 0, 7, 10, 1, 5, 11, 2, 9, 4, 8, 6]             # not in frame order, without frame 13
    expected = {}                                                # loops -> per entry (records, F, num_fit, rounds)
    for loops in LOOPS:
        expected[loops] = [expected_improve(frames[f][:max(counts[f], 0)], counts[f], starts[f], loops, *GATES, 1.0)
                           for f in sel]
    return dict(frames=frames, counts=counts, starts=starts, sel=sel, expected=expected)


def _poisoned(ctx, words):
    return ctx.upload(np.full(words, POISON_WORD, np.uint32))


def _improve(ctx, sel, recs, counts, offs, stride, F0, loops, thresh=1.0, rounds=True, d_recs=None):
    """improve on a start of exactly nsel x 9 floats and poisoned num_fit / num_rounds of nsel words.  Returns (F, num_fit,
    num_rounds or None, the records, the device buffers)."""
    from cudasift_amd import capi
    d = d_recs if d_recs is not None else ctx.upload(recs)
    dc = ctx.upload(np.asarray(counts, np.int32))
    do = ctx.upload(np.asarray(offs, np.int32)) if offs is not None else None
    dF = ctx.upload(np.ascontiguousarray(F0, np.float32).reshape(len(sel), 9))
    dfit, drounds = _poisoned(ctx, len(sel)), (_poisoned(ctx, len(sel)) if rounds else None)
    ctx.improve_fundamental_batch(sel, d, len(counts), dc, dF, do, stride, num_fit=dfit, num_rounds=drounds,
                                  num_loops=loops, min_score=GATES[0], max_ambiguity=GATES[1], thresh=thresh)
    ctx.sync()
    return (ctx.download(dF, (len(sel), 9), np.float32), ctx.download(dfit, (len(sel),), np.int32),
            ctx.download(drounds, (len(sel),), np.int32) if rounds else None,
            ctx.download(d, (len(recs),), capi.POINT_DTYPE), dict(d=d, dc=dc, do=do, dF=dF, dfit=dfit))


def _compare(got, sel, recs, counts, offs, stride, expected, what):
    """got = _improve's tuple; expected = per entry (records of the frame, F, num_fit, rounds)."""
    F, fit, rounds, after = got[:4]
    want = recs.copy()
    for i, (f, (out, Fe, ce, re)) in enumerate(zip(sel, expected)):
        want[span(offs, stride, f, max(counts[f], 0))] = out
        assert F[i].tobytes() == Fe.tobytes() and fit[i] == ce and (rounds is None or rounds[i] == re), \
            (what, "entry", i, "frame", f, "count", counts[f], fit[i], ce, None if rounds is None else rounds[i], re,
             F[i], Fe)
    if after.tobytes() != want.tobytes():
        a, b = after.view(np.uint8).reshape(len(recs), -1), want.view(np.uint8).reshape(len(recs), -1)
        bad = np.nonzero((a != b).any(1))[0]
        raise AssertionError("%s: %d records differ, first %s" % (what, len(bad), bad[:8]))
    only = [k for k in recs.dtype.names if after[k].tobytes() != recs[k].tobytes()]
    assert only in ([], ["match_error"]), (what, only)


def _laid_out(batch, padded):
    recs, offs, stride = layout(batch["frames"], batch["counts"], padded, min_stride=0, pad_error=-7.0)
    F0 = np.stack([batch["starts"][f] for f in batch["sel"]])
    return recs, offs, stride, F0


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
@pytest.mark.parametrize("loops", LOOPS)
def test_every_frame_count(g, batch, padded, loops):
    recs, offs, stride, F0 = _laid_out(batch, padded)
    sel, counts = batch["sel"], batch["counts"]
    got = _improve(g, sel, recs, counts, offs, stride, F0, loops)
    _compare(got, sel, recs, counts, offs, stride, batch["expected"][loops], "loops %d" % loops)
    F, fit, rounds = got[:3]
    by_frame = {f: i for i, f in enumerate(sel)}
    for f in (0, 1, 2):                                          # count -1, no records, 7 records: F as it was
        assert fit[by_frame[f]] <= 7 and rounds[by_frame[f]] == 0 and F[by_frame[f]].tobytes() == F0[by_frame[f]].tobytes()
    assert (rounds <= loops).all()
    if loops == 5:
        big = by_frame[len(counts) - 2]                          # one record more than is staged on chip
        assert rounds[big] >= 1 and fit[big] > 2000 and counts[sel[big]] == capacity() + 1, (rounds, fit)
        assert (rounds[[by_frame[f] for f in range(5, 12)]] >= 1).all(), rounds


def test_zero_loops_is_score(g, batch):
    """num_loops = 0 against misift_score_fundamental_batch on a second copy of the batch."""
    from cudasift_amd import capi
    recs, offs, stride, F0 = _laid_out(batch, False)
    sel, counts = batch["sel"], batch["counts"]
    F, fit, rounds, after, _ = _improve(g, sel, recs, counts, offs, stride, F0, 0)
    d2, dc, do = g.upload(recs), g.upload(np.asarray(counts, np.int32)), g.upload(offs)
    dF, dfit = g.upload(F0), _poisoned(g, len(sel))
    g.score_fundamental_batch(sel, d2, len(counts), dc, dF, do, stride, num_fit=dfit, min_score=GATES[0],
                              max_ambiguity=GATES[1], thresh=1.0)
    g.sync()
    assert after.tobytes() == g.download(d2, (len(recs),), capi.POINT_DTYPE).tobytes()
    assert fit.tobytes() == g.download(dfit, (len(sel),), np.int32).tobytes()
    assert F.tobytes() == F0.tobytes() and (rounds == 0).all()


def test_score_under_the_result_changes_nothing(g, batch):
    """After five rounds, misift_score_fundamental_batch under the returned F rewrites the same bytes and counts the same
    records."""
    from cudasift_amd import capi
    recs, offs, stride, F0 = _laid_out(batch, True)
    sel, counts = batch["sel"], batch["counts"]
    F, fit, _, after, b = _improve(g, sel, recs, counts, offs, stride, F0, 5)
    dfit = _poisoned(g, len(sel))
    g.score_fundamental_batch(sel, b["d"], len(counts), b["dc"], b["dF"], b["do"], stride, num_fit=dfit,
                              min_score=GATES[0], max_ambiguity=GATES[1], thresh=1.0)
    g.sync()
    assert after.tobytes() == g.download(b["d"], (len(recs),), capi.POINT_DTYPE).tobytes()
    assert fit.tobytes() == g.download(dfit, (len(sel),), np.int32).tobytes()
    assert g.download(b["dF"], F.shape, np.float32).tobytes() == F.tobytes()


def test_two_runs_are_identical_and_rounds_may_be_null(g, batch):
    recs, offs, stride, F0 = _laid_out(batch, False)
    sel, counts = batch["sel"], batch["counts"]
    a = _improve(g, sel, recs, counts, offs, stride, F0, 5)
    b = _improve(g, sel, recs, counts, offs, stride, F0, 5)
    c = _improve(g, sel, recs, counts, offs, stride, F0, 5, rounds=False)    # d_num_rounds = NULL
    for x, y, z in zip(a[:4], b[:4], c[:4]):
        assert x.tobytes() == y.tobytes() and (z is None or x.tobytes() == z.tobytes())
    _compare(c, sel, recs, counts, offs, stride, batch["expected"][5], "no rounds")


@pytest.mark.parametrize("loops", LOOPS)
def test_hostile_cases(g, loops):
    """The CPU file's hostile inputs, one call per threshold."""
    cases = hostile_cases()
    with np.errstate(all="ignore"):
        for thresh in sorted({c[3] for c in cases}):
            mine = [c for c in cases if c[3] == thresh]
            fr = [c[1] for c in mine]
            counts = [len(p) for p in fr]
            recs, offs, stride = layout(fr, counts, False, min_stride=0, pad_error=0.0)
            sel = list(range(len(fr)))[::-1]
            F0 = np.stack([np.ascontiguousarray(mine[f][2], np.float32).reshape(9) for f in sel])
            exp = [expected_improve(fr[f], counts[f], mine[f][2], loops, *GATES, thresh) for f in sel]
            got = _improve(g, sel, recs, counts, offs, stride, F0, loops, thresh=thresh)
            _compare(got, sel, recs, counts, offs, stride, exp, "hostile, thresh %g" % thresh)


def test_find_improve_link(g):
    """Pair rows of a moving camera (4 views, window 3) with 0.5 px noise and planted wrong matches -> find -> improve ->
    link with a finite max_error, nothing read in between: the labels equal expected_tracks on the rows as
    expected_improve leaves them."""
    nf, n, mp = 4, 300, 320
    rng = np.random.default_rng(31)
    perm, pos, line_distance = _multi_view(nf, n, 31)
    pairs = window_pairs(list(range(nf)), 3)
    rows = blank_rows(len(pairs), mp, 32)
    plant(rows, mp, pairs, [{f: int(perm[f][k]) for f in range(nf)} for k in range(n)], 0.1, rng)
    wrong = []
    for i, (f1, f2) in enumerate(pairs):
        o = rows[i * mp:(i + 1) * mp]
        for r in rng.choice(n, 30, replace=False):               # a wrong match, at least 20 px off the epipolar line
            m = next(int(m) for m in rng.permutation(n) if line_distance(f1, f2, r, m) > 20.0)
            set_edge(rows, mp, i, int(r), m)
            wrong.append(i * mp + int(r))
        o["xpos"][:n], o["ypos"][:n] = pos[f1][:, 0], pos[f1][:, 1]
        m = o["match"][:n]
        ok = o["score"][:n] > 0.85                               # the planted rows; the blank ones keep NaN positions
        noise = rng.normal(0, NOISE, (int(ok.sum()), 2))
        o["match_xpos"][:n][ok] = pos[f2][m[ok], 0] + noise[:, 0]
        o["match_ypos"][:n][ok] = pos[f2][m[ok], 1] + noise[:, 1]
    row_counts = [n] * len(pairs)
    sel, seeds = list(range(len(pairs))), [500 + i for i in range(len(pairs))]
    gates = GATES + (1.0,)
    scored, c0, c5 = rows.copy(), [], []
    for i in sel:
        sl = slice(i * mp, i * mp + n)
        F0, c = expected_find(rows[sl], n, seeds[i], 256, *GATES, 1.0, mp)
        scored[sl], _, fit, _ = expected_improve(rows[sl], n, F0, 5, *GATES, 1.0)
        c0.append(c)
        c5.append(fit)
    assert min(c0) > 100 and all(b >= a for a, b in zip(c0, c5)) and sum(c5) > sum(c0), (c0, c5)
    assert (scored["match_error"][wrong] > 1.0).all()
    d_rows = g.upload(rows)
    d_rc, d_cnt = g.upload(np.asarray(row_counts, np.int32)), g.upload(np.full(nf, n, np.int32))
    offs = np.arange(nf + 1, dtype=np.int32) * n
    d_off = g.upload(offs)
    dfit = _poisoned(g, len(pairs))
    dF, _ = g.find_fundamental_batch(sel, seeds, d_rows, len(pairs), d_rc, None, mp, max_pts=mp, num_loops=256,
                                     min_score=gates[0], max_ambiguity=gates[1], thresh=1.0)
    g.improve_fundamental_batch(sel, d_rows, len(pairs), d_rc, dF, None, mp, num_fit=dfit, num_loops=5,
                                min_score=gates[0], max_ambiguity=gates[1], thresh=1.0)
    out = [_poisoned(g, nf * n) for _ in range(3)] + [_poisoned(g, 8)]
    g.link_tracks_batch(pairs, d_rows, d_rc, mp, nf, d_cnt, d_off, 0, max_records=nf * n, min_score=gates[0],
                        max_ambiguity=gates[1], max_error=gates[2], track=out[0], track_len=out[1], track_frames=out[2],
                        summary=out[3])
    g.sync()
    assert g.download(dfit, (len(pairs),), np.int32).tolist() == c5
    got = [g.download(b, (k,), np.int32) for b, k in zip(out, (nf * n,) * 3 + (8,))]
    exp = expected_tracks(pairs, scored, row_counts, mp, [n] * nf, offs, 0, nf * n, gates, poison=POISON_WORD)
    for a, b, name in zip(got, exp, ("track", "track_len", "track_frames", "summary")):
        assert a.tobytes() == b.tobytes(), (name, np.nonzero(a != b)[0][:8])
    loose = expected_tracks(pairs, scored, row_counts, mp, [n] * nf, offs, 0, nf * n, GATES + (INF,))
    assert got[3][1] > 200 and loose[3][3] > got[3][3], (got[3], loose[3])


def test_argument_errors_enqueue_nothing(g, batch):
    from cudasift_amd import capi
    L = capi.lib()
    recs = np.concatenate([batch["frames"][3], batch["frames"][4]])          # two frames of 8 and 9 records
    d, dc = g.upload(recs), g.upload(np.array([8, 9], np.int32))
    do = g.upload(np.array([0, 8, 17], np.int32))
    F0 = np.stack([batch["starts"][3], batch["starts"][4]])
    dF, dn, dr = _poisoned(g, 18), _poisoned(g, 2), _poisoned(g, 2)
    fr = np.array([0, 1], np.int32)
    good = dict(ctx=g.h, nsel=2, frames=fr.ctypes.data, recs=d.ptr, nframes=2, counts=dc.ptr, offsets=do.ptr, stride=0,
                num_loops=5, min_score=0.85, max_ambiguity=0.95, thresh=1.0, F=dF.ptr, num=dn.ptr, rounds=dr.ptr)

    def improve(**kw):
        a = dict(good, **kw)
        return L.misift_improve_fundamental_batch(*[a[k] for k in good])

    lists = [np.array(v, np.int32) for v in ([0, 2], [-1, 1], [1, 1])]
    bad = [dict(ctx=None), dict(nsel=-1), dict(recs=None), dict(counts=None), dict(F=None), dict(num=None),
           dict(num_loops=-1), dict(thresh=float("nan")), dict(thresh=0.0), dict(thresh=-1.0),
           dict(offsets=None, stride=-1), dict(frames=None)]
    bad += [dict(frames=v.ctypes.data) for v in lists]
    for kw in bad:
        assert improve(**kw) == MISIFT_EINVAL, kw
    assert improve(nsel=0) == MISIFT_OK                          # nothing happens
    g.sync()
    for b, k in ((dF, 18), (dn, 2), (dr, 2)):
        assert (g.download(b, (k,), np.uint32) == POISON_WORD).all()
    assert g.download(d, (len(recs),), capi.POINT_DTYPE).tobytes() == recs.tobytes()
    capi.check(L.misift_copy_h2d(g.h, dF.ptr, F0.ctypes.data, F0.nbytes), "misift_copy_h2d")
    assert improve() == MISIFT_OK                                # the same arguments, unbroken
    g.sync()
    assert (g.download(dn, (2,), np.int32) >= 6).all() and (g.download(dr, (2,), np.int32) <= 5).all()


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0

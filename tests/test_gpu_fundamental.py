"""misift_find_fundamental_batch / misift_score_fundamental_batch on the device: a RANSAC fundamental matrix per frame of a
device-resident batch, and the Sampson distance of every record into match_error.

Every comparison is byte equality with test_fundamental_cpu.expected_find / expected_score (pinned there to the library's
host hooks and to float64 geometry): F, the counts, every match_error, and every other byte of the records.  The outputs
have exactly the stated capacity and are poisoned first; all allocations of the module are guarded."""
import numpy as np
import pytest

from batch_util import POISON_WORD, guarded_context, layout, span
from fundamental_cases import (COUNTS, MAX_PTS, SEEDS, SEL, SIZES, batch_records as _records,
                               expected_find_score as _expected, make_batch)
from test_fundamental_cpu import (GATES, SCENE_FIND_SEED, SCENE_LOOPS, SCENE_SEEDS, expected_find, expected_score,
                                  planted_scene)
from test_tracks_cpu import INF, blank_rows, expected_tracks, plant, set_edge, window_pairs

pytestmark = pytest.mark.gpu

MISIFT_OK, MISIFT_EINVAL = 0, -1


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


@pytest.fixture(scope="module")
def batch():
    return make_batch()


def _poisoned(ctx, words):
    return ctx.upload(np.full(words, POISON_WORD, np.uint32))


def _find_score(ctx, sel, seeds, recs, counts, offs, stride, loops, thresh, max_pts, d_recs=None):
    """find then score on poisoned outputs of exactly nsel x 9 and nsel words.  Returns (F, num_inliers, the records after
    find, the records after score, num_fit)."""
    from cudasift_amd import capi
    d = d_recs if d_recs is not None else ctx.upload(recs)
    dc = ctx.upload(np.asarray(counts, np.int32))
    do = ctx.upload(np.asarray(offs, np.int32)) if offs is not None else None
    dF, dn, dfit = _poisoned(ctx, 9 * len(sel)), _poisoned(ctx, len(sel)), _poisoned(ctx, len(sel))
    ctx.find_fundamental_batch(sel, seeds, d, len(counts), dc, do, stride, max_pts=max_pts, num_loops=loops,
                               min_score=GATES[0], max_ambiguity=GATES[1], thresh=thresh, fundamental=dF,
                               num_inliers=dn)
    ctx.sync()
    mid = ctx.download(d, (len(recs),), capi.POINT_DTYPE)
    ctx.score_fundamental_batch(sel, d, len(counts), dc, dF, do, stride, num_fit=dfit, min_score=GATES[0],
                                max_ambiguity=GATES[1], thresh=thresh)
    ctx.sync()
    return (ctx.download(dF, (len(sel), 9), np.float32), ctx.download(dn, (len(sel),), np.int32), mid,
            ctx.download(d, (len(recs),), capi.POINT_DTYPE), ctx.download(dfit, (len(sel),), np.int32))


def _check(ctx, sel, seeds, recs, counts, offs, stride, loops, thresh=1.0, max_pts=MAX_PTS, what=""):
    got = _find_score(ctx, sel, seeds, recs, counts, offs, stride, loops, thresh, max_pts)
    F, num, after, fit = _expected(sel, seeds, recs, counts, offs, stride, loops, thresh, max_pts)
    assert got[2].tobytes() == recs.tobytes(), "%s: find wrote into the records" % what
    for i, f in enumerate(sel):
        assert got[1][i] == num[i] and got[0][i].tobytes() == F[i].tobytes(), \
            (what, "entry", i, "frame", f, "count", counts[f], got[1][i], num[i], got[0][i], F[i])
        assert got[4][i] == fit[i], (what, "num_fit", i, f, got[4][i], fit[i])
    if got[3].tobytes() != after.tobytes():
        a, b = got[3].view(np.uint8).reshape(len(recs), -1), after.view(np.uint8).reshape(len(recs), -1)
        bad = np.nonzero((a != b).any(1))[0]
        raise AssertionError("%s: %d records differ after score, first %s" % (what, len(bad), bad[:8]))
    return got


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
@pytest.mark.parametrize("loops", [1, 16, 17, 64, 65, 200])
def test_every_frame_count(g, batch, padded, loops):
    recs, offs, stride = layout(batch, COUNTS, padded, min_stride=2048, pad_error=-7.0)
    F, num, _, after, fit = _check(g, SEL, SEEDS, recs, COUNTS, offs, stride, loops, what="loops %d" % loops)
    by_frame = {f: i for i, f in enumerate(SEL)}
    for f in (0, 1, 10, 12):                                     # fewer than 8 records or valid records, count -1
        assert num[by_frame[f]] == 0 and (F[by_frame[f]].view(np.uint32) == 0).all(), f
    assert num[by_frame[11]] == -1 and (F[by_frame[11]].view(np.uint32) == 0).all()
    over = after[span(offs, stride, 11, SIZES[11])]
    assert np.isposinf(over["match_error"]).all() and fit[by_frame[11]] == 0
    if loops >= 64:
        assert num[by_frame[9]] > 1000 and num[by_frame[8]] > 250, num


def test_two_runs_are_identical(g, batch):
    recs, offs, stride = layout(batch, COUNTS, False, min_stride=2048, pad_error=-7.0)
    a = _find_score(g, SEL, SEEDS, recs, COUNTS, offs, stride, 200, 1.0, MAX_PTS)
    b = _find_score(g, SEL, SEEDS, recs, COUNTS, offs, stride, 200, 1.0, MAX_PTS)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_planted_scenes(g):
    """The CPU file's scenes through find -> score: equal to the restatement, and on the device's own output every
    planted inlier lies within thresh."""
    scenes = [planted_scene(s) for s in SCENE_SEEDS]
    frames = [s[0] for s in scenes]
    counts = [len(p) for p in frames]
    recs, offs, stride = layout(frames, counts, False, min_stride=0, pad_error=0.0)
    sel = list(range(len(frames)))
    F, num, _, after, fit = _check(g, sel, [SCENE_FIND_SEED] * len(sel), recs, counts, offs, stride, SCENE_LOOPS,
                                   max_pts=2048, what="scenes")
    for f, (_, inl, _) in enumerate(scenes):
        err = after[span(offs, stride, f, counts[f])]["match_error"]
        assert (err[inl] < 1.0).all() and num[f] >= inl.sum() and fit[f] == num[f]


def _multi_view(nf, n, seed):
    """n 3-D points seen in nf pinhole views; record perm[f][k] of frame f is point k.  Returns (perm, pos[f] = (n, 2)
    positions by record, line_distance(f1, f2, r, m): how far record m of f2 lies from the epipolar line of record r of
    f1, in float64 pixels)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform([-4, -3, 6], [4, 3, 14], (n, 3))
    K = np.array([[1400.0, 0, 960], [0, 1400, 540], [0, 0, 1]])
    Ki = np.linalg.inv(K)
    perm = np.stack([rng.permutation(n) for _ in range(nf)])
    Rs, ts, pos = [], [], []
    for f in range(nf):
        a = 0.05 * f
        Rs.append(np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]))
        ts.append(np.array([0.5 * f, 0.05 * f, 0.1 * f]))
        p = (K @ (Rs[f] @ X.T + ts[f][:, None])).T
        by_record = np.zeros((n, 2))
        by_record[perm[f]] = p[:, :2] / p[:, 2:]
        pos.append(by_record)

    def line_distance(f1, f2, r, m):
        R = Rs[f2] @ Rs[f1].T
        t = ts[f2] - R @ ts[f1]
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        line = Ki.T @ tx @ R @ Ki @ np.append(pos[f1][r], 1.0)
        return abs(line @ np.append(pos[f2][m], 1.0)) / np.hypot(line[0], line[1])
    return perm, pos, line_distance


def test_find_score_link(g):
    """Pair rows of a moving camera (4 views, window 3) with planted wrong matches -> find -> score -> link with a finite
    max_error, nothing read in between: the rows equal the restatement's, the wrong matches are no edges, and the
    labels equal expected_tracks on the rows as expected_score leaves them."""
    nf, n, mp = 4, 300, 320
    rng = np.random.default_rng(21)
    perm, pos, line_distance = _multi_view(nf, n, 21)
    pairs = window_pairs(list(range(nf)), 3)
    rows = blank_rows(len(pairs), mp, 22)
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
        o["match_xpos"][:n][ok], o["match_ypos"][:n][ok] = pos[f2][m[ok], 0], pos[f2][m[ok], 1]
    row_counts = [n] * len(pairs)
    sel, seeds = list(range(len(pairs))), [500 + i for i in range(len(pairs))]
    gates = GATES + (1.0,)
    d_rows = g.upload(rows)
    F, num, _, scored, fit = _check(g, sel, seeds, rows, row_counts, None, mp, 256, max_pts=mp, what="rows")
    assert (num > 200).all() and (scored["match_error"][wrong] > 1.0).all()
    # the same on the device with no host read between the three calls
    d_rc, d_cnt = g.upload(np.asarray(row_counts, np.int32)), g.upload(np.full(nf, n, np.int32))
    offs = np.arange(nf + 1, dtype=np.int32) * n
    d_off = g.upload(offs)
    dF, _ = g.find_fundamental_batch(sel, seeds, d_rows, len(pairs), d_rc, None, mp, max_pts=mp, num_loops=256,
                                     min_score=gates[0], max_ambiguity=gates[1], thresh=1.0)
    g.score_fundamental_batch(sel, d_rows, len(pairs), d_rc, dF, None, mp, min_score=gates[0], max_ambiguity=gates[1],
                              thresh=1.0)
    out = [_poisoned(g, nf * n) for _ in range(3)] + [_poisoned(g, 8)]
    g.link_tracks_batch(pairs, d_rows, d_rc, mp, nf, d_cnt, d_off, 0, max_records=nf * n, min_score=gates[0],
                        max_ambiguity=gates[1], max_error=gates[2], track=out[0], track_len=out[1], track_frames=out[2],
                        summary=out[3])
    g.sync()
    got = [g.download(b, (k,), np.int32) for b, k in zip(out, (nf * n,) * 3 + (8,))]
    exp = expected_tracks(pairs, scored, row_counts, mp, [n] * nf, offs, 0, nf * n, gates, poison=POISON_WORD)
    for a, b, name in zip(got, exp, ("track", "track_len", "track_frames", "summary")):
        assert a.tobytes() == b.tobytes(), (name, np.nonzero(a != b)[0][:8])
    loose = expected_tracks(pairs, scored, row_counts, mp, [n] * nf, offs, 0, nf * n, GATES + (INF,))
    assert got[3][3] == 0 and got[3][1] > 250 and loose[3][3] > 0, (got[3], loose[3])


def test_argument_errors_enqueue_nothing(g, batch):
    from cudasift_amd import capi
    L = capi.lib()
    nan = float("nan")
    recs = np.concatenate([batch[5], batch[6]])                  # two frames of 64 and 65 records, stride 64 / packed
    d, dc = g.upload(recs), g.upload(np.array([64, 65], np.int32))
    do = g.upload(np.array([0, 64, 129], np.int32))
    dF, dn = _poisoned(g, 18), _poisoned(g, 2)
    fr, sd = np.array([0, 1], np.int32), np.array([1, 2], np.uint32)
    good = dict(ctx=g.h, nsel=2, frames=fr.ctypes.data, seeds=sd.ctypes.data, recs=d.ptr, nframes=2, counts=dc.ptr,
                offsets=do.ptr, stride=0, max_pts=128, num_loops=16, min_score=0.85, max_ambiguity=0.95, thresh=1.0,
                F=dF.ptr, num=dn.ptr)
    score_keys = [k for k in good if k not in ("seeds", "max_pts", "num_loops")]

    def find(**kw):
        a = dict(good, **kw)
        return L.misift_find_fundamental_batch(*[a[k] for k in good])

    def score(**kw):
        a = dict(good, **kw)
        return L.misift_score_fundamental_batch(*[a[k] for k in score_keys])

    lists = [np.array(v, np.int32) for v in ([0, 2], [-1, 1], [1, 1])]
    common = [dict(ctx=None), dict(nsel=-1), dict(recs=None), dict(counts=None), dict(F=None), dict(num=None),
              dict(thresh=nan), dict(thresh=0.0), dict(thresh=-1.0), dict(offsets=None, stride=-1)]
    common += [dict(frames=v.ctypes.data) for v in lists]
    for kw in common + [dict(max_pts=0), dict(num_loops=0)]:
        assert find(**kw) == MISIFT_EINVAL, kw
    for kw in common:
        assert score(**kw) == MISIFT_EINVAL, kw
    assert find(nsel=0) == MISIFT_OK and score(nsel=0) == MISIFT_OK          # nothing happens
    g.sync()
    assert (g.download(dF, (18,), np.uint32) == POISON_WORD).all() and (g.download(dn, (2,), np.uint32) == POISON_WORD).all()
    assert g.download(d, (len(recs),), capi.POINT_DTYPE).tobytes() == recs.tobytes()
    assert find() == MISIFT_OK and score() == MISIFT_OK          # the same arguments, unbroken
    g.sync()
    num = g.download(dn, (2,), np.int32)
    assert (num >= 8).all(), num


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0

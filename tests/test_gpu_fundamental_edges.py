"""misift_find_fundamental_batch / misift_score_fundamental_batch on the device at the edges of their definition: the
degenerate, non-finite, underflowing and overflowing inputs of fundamental_cases.py (pinned without a GPU in
test_fundamental_edges_cpu.py), and the shapes the kernels treat differently: a last chunk of one valid record and an
exactly full one, max_pts off the multiple of 16 with a frame that fills it, hundreds of entries, and temp memory that
still holds another call's layout while the calls queue up behind one another.

The harness is test_gpu_fundamental's: poisoned outputs of exactly their capacity, a guarded context, and every
comparison byte equality with expected_find / expected_score: F, the counts, num_fit, every match_error and every other
byte of the records."""
import numpy as np
import pytest

import fundamental_cases as FC
from batch_util import POISON_WORD, frames as match_frames, guarded_context, layout, span
from test_fundamental_cpu import GATES, expected_score, gate, hypotheses, solve8
from test_gpu_fundamental import (COUNTS, MAX_PTS, SEEDS, SEL, _check, _expected, _poisoned, _records, make_batch)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


def _guards_ok():
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0


def _zero(F, num, i):
    return num[i] == 0 and (np.ascontiguousarray(F[i]).view(np.uint32) == 0).all()


# ---- forced samples

@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
@pytest.mark.parametrize("loops", [1, 65])
def test_forced_samples(g, loops, padded):
    """Every frame holds exactly 8 valid records, so each hypothesis is a permutation of one sample."""
    named = FC.forced_samples()
    fr = [FC.forced_frame(s, 8 + (7 * i) % 43, 100 + i) for i, (_, s) in enumerate(named)]
    counts = [len(p) for p in fr]
    assert min(counts) == 16 and max(counts) == 58 and all(gate(p, *GATES).sum() == 8 for p in fr)
    recs, offs, stride = layout(fr, counts, padded, min_stride=0, pad_error=-7.0)
    sel = [int(f) for f in np.random.default_rng(1).permutation(len(fr))]
    seeds = [11 + f for f in sel]
    F, num, _, _, fit = _check(g, sel, seeds, recs, counts, offs, stride, loops, max_pts=58, what="forced")
    valid, invalid = 0, []
    for i, f in enumerate(sel):                                  # where the restatement says invalid: nine zeros and 0
        idx, _, _ = hypotheses(fr[f], counts[f], seeds[i], loops, *GATES, 1.0)
        _, ok = solve8(*[fr[f][k][idx] for k in FC.POS])
        if not ok.any():
            assert _zero(F, num, i) and fit[i] == 0, named[f][0]
            invalid.append(named[f][0])
        valid += not _zero(F, num, i)
    assert {"identical", "axis-parallel line", "two points", "scale 1e-22 #0", "scale 1e+25 #47"} <= set(invalid)
    assert sum("column" in n for n in invalid) == 12 and len(invalid) >= 25, invalid
    assert valid >= 40, valid


# ---- gate values

def test_gate_values(g):
    """NaN, +inf, -inf in score and ambiguity, and the floats next to the two gates."""
    made = [FC.gate_frame(s) for s in (1, 2, 3)]
    fr = [m[0] for m in made]
    counts = [len(p) for p in fr]
    recs, offs, stride = layout(fr, counts, False, min_stride=0, pad_error=0.0)
    F, num, _, _, fit = _check(g, [2, 0, 1], [5, 6, 7], recs, counts, offs, stride, 65, max_pts=120, what="gates")
    for i, f in enumerate((2, 0, 1)):
        assert 8 <= num[i] <= made[f][1].sum() and fit[i] == num[i], (f, num[i], fit[i])


# ---- mixed scenes

@pytest.mark.parametrize("loops", FC.MIXED_LOOPS)
def test_mixed_scenes(g, loops):
    """A tenth of the records hostile.  On the device's own output every finite planted inlier lies within thresh, and
    every record with a non-finite position has the restatement's match_error, bit for bit."""
    made = [FC.mixed_scene(s) for s in FC.MIXED_SEEDS]
    fr = [m[0] for m in made]
    counts = [len(p) for p in fr]
    recs, offs, stride = layout(fr, counts, False, min_stride=0, pad_error=0.0)
    sel = list(range(len(fr)))
    F, num, _, after, fit = _check(g, sel, [FC.MIXED_FIND_SEED] * len(sel), recs, counts, offs, stride, loops,
                                   max_pts=600, what="mixed")
    for f, (scene, inl, hostile) in enumerate(made):
        err = after[span(offs, stride, f, counts[f])]["match_error"]
        fin = inl & ~hostile
        assert (err[fin] < 1.0).all() and fin.sum() <= num[f] <= fin.sum() + 3 and fit[f] == num[f]
        bad = ~np.isfinite(np.stack([scene[k] for k in FC.POS])).all(0)
        want, _ = expected_score(scene, counts[f], F[f], *GATES, 1.0)
        assert bad.sum() >= 20 and err[bad].tobytes() == want["match_error"][bad].tobytes()
        assert not (err[bad] < 1.0).any()


# ---- score under a caller's F

SCORE_COUNTS = (0, 1, 255, 256, 257, 1025)                       # around the 256-thread loop of the score kernel


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
def test_score_under_given_F(g, padded):
    """F need not come from find: NaN, +-inf, 1e30 (den overflows), 1e-30 (den underflows), -0, subnormal entries, a
    rank-3 matrix, against positions that are random bit patterns."""
    from cudasift_amd import capi
    mats = FC.score_matrices()
    fr, Fs = [], []
    for m, (_, F) in enumerate(mats):
        for n in SCORE_COUNTS:
            fr.append(FC.score_frame(n, 50 * m + len(fr)))
            Fs.append(F)
    counts = [len(p) for p in fr]
    recs, offs, stride = layout(fr, counts, padded, min_stride=0, pad_error=-7.0)
    sel = [int(f) for f in np.random.default_rng(2).permutation(len(fr))]
    Fsel = np.stack([Fs[f] for f in sel]).astype(np.float32)
    d, dc = g.upload(recs), g.upload(np.asarray(counts, np.int32))
    do = g.upload(offs) if offs is not None else None
    dF, dfit = g.upload(Fsel), _poisoned(g, len(sel))
    g.score_fundamental_batch(sel, d, len(counts), dc, dF, do, stride, num_fit=dfit, min_score=GATES[0],
                              max_ambiguity=GATES[1], thresh=1.0)
    g.sync()
    got, fit = g.download(d, (len(recs),), capi.POINT_DTYPE), g.download(dfit, (len(sel),), np.int32)
    assert g.download(dF, Fsel.shape, np.float32).tobytes() == Fsel.tobytes()
    after = recs.copy()
    nans = 0
    for i, f in enumerate(sel):
        sl = span(offs, stride, f, counts[f])
        after[sl], want = expected_score(recs[sl], counts[f], Fsel[i], *GATES, 1.0)
        assert fit[i] == want, (mats[f // len(SCORE_COUNTS)][0], counts[f], fit[i], want)
        a, b = got[sl]["match_error"], after[sl]["match_error"]
        assert a.tobytes() == b.tobytes(), (mats[f // len(SCORE_COUNTS)][0], counts[f],
                                            np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0][:8])
        nans += int(np.isnan(b).sum())
    assert got.tobytes() == after.tobytes()                      # every other byte, the padding included
    assert nans > 1000                                           # the one NaN of the header is stored, often
    _guards_ok()


# ---- thresholds

def test_extreme_thresholds(g):
    """thresh * thresh is 0, 0, 1e38, +inf and +inf."""
    from test_fundamental_cpu import planted_scene
    c = FC.THRESH_SCENE
    scene, _, _ = planted_scene(c["seed"], n=c["n"])
    with np.errstate(over="ignore"):
        for t, want in zip(FC.THRESHOLDS, (0, 0, c["n"], c["n"], c["n"])):
            F, num, _, _, fit = _check(g, [0], [c["find_seed"]], scene, [c["n"]], None, c["n"], c["loops"], thresh=t,
                                       max_pts=c["n"], what="thresh %g" % t)
            assert num[0] == want and fit[0] == want and np.abs(F[0]).max() > 0, (t, num, fit)


# ---- the count kernel's 512-record chunks

BOUNDARY_KEEP = (511, 512, 513, 1023, 1024, 1025)


@pytest.mark.parametrize("loops", [17, 65])
def test_valid_record_boundaries(g, loops):
    """Frames of about 1300 records with exactly 511 ... 1025 valid ones: a last chunk of one record, a full one."""
    fr = [_records(1290 + 3 * f, 40 + f, keep) for f, keep in enumerate(BOUNDARY_KEEP)]
    for p, keep in zip(fr, BOUNDARY_KEEP):
        assert gate(p, *GATES).sum() == keep
    counts = [len(p) for p in fr]
    recs, offs, stride = layout(fr, counts, False, min_stride=0, pad_error=0.0)
    sel = [3, 0, 5, 2, 4, 1]
    F, num, _, _, fit = _check(g, sel, [60 + f for f in sel], recs, counts, offs, stride, loops, max_pts=1310,
                               what="boundaries")
    if loops == 65:
        for i, f in enumerate(sel):                              # three quarters of the valid records are planted inliers
            assert num[i] > 0.7 * BOUNDARY_KEEP[f] and fit[i] == num[i], (f, num[i])
    _guards_ok()


# ---- max_pts off the multiple of 16

@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
@pytest.mark.parametrize("max_pts", [8, 9, 513, 2001])
def test_max_pts_off_16(g, max_pts, padded):
    """A frame of exactly max_pts records, all valid; one of max_pts + 1 (-1, nothing read); smaller ones in the same
    call.  The temp layout is sized from max_pts rounded up to 16: the guarded temp shows no damage."""
    sizes = [max_pts, max_pts + 1, 0, 7, max_pts // 2, max_pts - 1, max_pts, 8]
    keep = {0: max_pts}
    fr = [_records(n, 70 + f, keep.get(f)) for f, n in enumerate(sizes)]
    recs, offs, stride = layout(fr, sizes, padded, min_stride=0, pad_error=-7.0)
    sel = [6, 1, 0, 7, 3, 5, 2, 4]
    F, num, _, after, fit = _check(g, sel, [80 + f for f in sel], recs, sizes, offs, stride, 33, max_pts=max_pts,
                                   what="max_pts %d" % max_pts)
    by = {f: i for i, f in enumerate(sel)}
    assert num[by[1]] == -1 and (F[by[1]].view(np.uint32) == 0).all() and fit[by[1]] == 0
    assert np.isposinf(after[span(offs, stride, 1, sizes[1])]["match_error"]).all()
    assert num[by[0]] >= 6 and num[by[7]] >= 6 and _zero(F, num, by[2]) and _zero(F, num, by[3])
    _guards_ok()


# ---- many entries

def test_many_entries(g):
    """257 entries over 260 frames of 8 to 40 records, 65 loops: the entry index of every launch is a division."""
    rng = np.random.default_rng(3)
    sizes = [int(n) for n in rng.integers(8, 41, 260)]
    sizes[:4] = [8, 40, 9, 39]
    fr = [_records(n, 200 + f) for f, n in enumerate(sizes)]
    recs, offs, stride = layout(fr, sizes, False, min_stride=0, pad_error=0.0)
    sel = [int(f) for f in rng.permutation(260)[:257]]
    seeds = [int(s) for s in rng.integers(0, 2 ** 32, 257, dtype=np.uint64)]
    seeds[0], seeds[100], seeds[256] = 0, 2 ** 32 - 1, 2 ** 31
    F, num, _, _, fit = _check(g, sel, seeds, recs, sizes, offs, stride, 65, max_pts=40, what="many")
    assert (num >= 6).sum() > 150 and (num == 0).sum() > 5, (num >= 6).sum()       # frames gated below 8 valid records
    _guards_ok()


# ---- stale temp memory

def _buffers(ctx, sel, recs, counts, offs):
    """Everything one find -> score call needs on the device, uploaded (each upload synchronises the stream): the
    records, counts, offsets and the poisoned F, num_inliers and num_fit."""
    do = ctx.upload(np.asarray(offs, np.int32)) if offs is not None else None
    return dict(d=ctx.upload(recs), dc=ctx.upload(np.asarray(counts, np.int32)), do=do, dF=_poisoned(ctx, 9 * len(sel)),
                dn=_poisoned(ctx, len(sel)), dfit=_poisoned(ctx, len(sel)))


def _enqueue(ctx, b, sel, seeds, counts, stride, loops, max_pts):
    """find -> score on uploaded buffers: two library calls, nothing read, no upload, no synchronisation."""
    ctx.find_fundamental_batch(sel, seeds, b["d"], len(counts), b["dc"], b["do"], stride, max_pts=max_pts,
                               num_loops=loops, min_score=GATES[0], max_ambiguity=GATES[1], thresh=1.0,
                               fundamental=b["dF"], num_inliers=b["dn"])
    ctx.score_fundamental_batch(sel, b["d"], len(counts), b["dc"], b["dF"], b["do"], stride, num_fit=b["dfit"],
                                min_score=GATES[0], max_ambiguity=GATES[1], thresh=1.0)


def test_stale_temp():
    """The grow-only temp is shared with the matchers and the homography search.  On a context of its own: the 15-entry
    batch at 200 loops, a 2-entry call (max_pts 9, 1 loop), a homography search and a brute-force match on other
    buffers, the 2-entry call, a call larger than the first (256 loops, max_pts 2048), the 2-entry call.  meta, hcount
    and sample of the small layout lie in bytes the other calls wrote in theirs.  Every buffer of all six steps is
    uploaded first; the steps are then library calls only, with no synchronisation by the test until all are enqueued
    (the library itself waits for the stream where it has to let the temp grow)."""
    from cudasift_amd import capi
    big, offs, stride = layout(make_batch(), COUNTS, False, min_stride=2048, pad_error=-7.0)
    small_fr = [_records(9, 301, 9), _records(8, 302)]
    small, soffs, sstride = layout(small_fr, [9, 8], False, min_stride=0, pad_error=0.0)
    mfr = match_frames([300, 280], 5, True)
    mrecs, moffs, _ = layout(mfr, [300, 280], False, min_stride=0, pad_error=0.0)
    calls = {"big": (SEL, SEEDS, big, COUNTS, offs, stride, 200, MAX_PTS),
             "small": ([1, 0], [7, 2 ** 32 - 1], small, [9, 8], soffs, sstride, 1, 9),
             "bigger": (SEL, SEEDS, big, COUNTS, offs, stride, 256, 2048)}
    steps = ("big", "small", "others", "small", "bigger", "small")
    want = {k: _expected(*v[:7], 1.0, v[7]) for k, v in calls.items()}
    with guarded_context(1) as g:
        bufs = [_buffers(g, calls[s][0], *calls[s][2:5]) if s != "others" else None for s in steps]
        d_h, d_m = g.upload(big), g.upload(mrecs)                # the other APIs' own buffers
        d_hc, d_ho = g.upload(np.asarray(COUNTS, np.int32)), g.upload(offs)
        d_mc, d_mo = g.upload(np.array([300, 280], np.int32)), g.upload(moffs)
        dH, dHn = _poisoned(g, 9 * len(SEL)), _poisoned(g, len(SEL))
        g.sync()
        for s, b in zip(steps, bufs):                            # library calls only from here to the sync
            if s == "others":
                g.find_homography_batch(SEL, SEEDS, d_h, len(COUNTS), d_hc, d_ho, stride, max_pts=MAX_PTS,
                                        num_loops=128, homography=dH, num_matches=dHn)
                g.match_batch([(0, 1)], d_m, 2, d_mc, d_mo, 0)
            else:
                sel, seeds, _, counts, _, st, loops, max_pts = calls[s]
                _enqueue(g, b, sel, seeds, counts, st, loops, max_pts)
        g.sync()
        assert (g.download(dHn, (len(SEL),), np.uint32) != POISON_WORD).all()   # the homography search ran
        assert g.download(d_m, (len(mrecs),), capi.POINT_DTYPE)[:300]["score"].tobytes() != \
            mrecs[:300]["score"].tobytes()                       # and the matcher
        for n, (s, b) in enumerate(zip(steps, bufs)):
            if b is None:
                continue
            sel, recs = calls[s][0], calls[s][2]
            F, num, after, fit = want[s]
            gF, gn = g.download(b["dF"], (len(sel), 9), np.float32), g.download(b["dn"], (len(sel),), np.int32)
            assert gF.tobytes() == F.tobytes() and gn.tobytes() == num.tobytes(), ("step", n + 1, s, gn, num)
            assert g.download(b["dfit"], (len(sel),), np.int32).tobytes() == fit.tobytes(), ("step", n + 1, s)
            assert g.download(b["d"], (len(recs),), capi.POINT_DTYPE).tobytes() == after.tobytes(), ("step", n + 1, s)
        _guards_ok()


def test_guards_intact_at_the_end(g):
    _guards_ok()

"""misift_link_tracks_batch on the device: the accepted matches of a pair-indexed batch joined across pairs into feature
tracks (connected components, labelled by their smallest record index).

Rows are fabricated in numpy from a planted track structure, so no matcher has to run.  The output buffers are poisoned
first and every comparison is byte equality with test_tracks_cpu.expected_tracks (pinned there to a dictionary
union-find): labels are minima and every other output an integer sum, so nothing depends on the dispatch order."""
import numpy as np
import pytest

from batch_util import frames, guarded_context, layout, planted_members as _members, span
from synth import synth_frame
from test_tracks_cpu import (GATES, INF, blank_rows, expected_tracks, gate_rows, plant, set_edge, window_pairs)

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
MISIFT_OK, MISIFT_EINVAL = 0, -1
NAMES = ("track", "track_len", "track_frames", "summary")


def _poisoned(ctx, nints):
    return ctx.upload(np.full(max(nints, 1), POISON, np.uint32))


def _run(ctx, pairs, rows, row_counts, max_pts, counts, offs, stride, max_records, gates=GATES, d_rows=None):
    """One call on poisoned outputs of exactly max_records ints; returns the four arrays as downloaded."""
    d_rows = d_rows if d_rows is not None else ctx.upload(rows if len(rows) else blank_rows(1, 1, 0))
    d_rc = ctx.upload(np.asarray(row_counts if len(row_counts) else [0], np.int32))
    d_cnt = ctx.upload(np.asarray(counts if len(counts) else [0], np.int32))
    d_off = ctx.upload(np.asarray(offs, np.int32)) if offs is not None else None
    out = [_poisoned(ctx, max_records) for _ in range(3)] + [_poisoned(ctx, 8)]
    ctx.link_tracks_batch(pairs, d_rows, d_rc, max_pts, len(counts), d_cnt, d_off, stride, max_records=max_records,
                          min_score=gates[0], max_ambiguity=gates[1], max_error=gates[2], track=out[0],
                          track_len=out[1], track_frames=out[2], summary=out[3])
    ctx.sync()
    return [ctx.download(b, (n,), np.int32) for b, n in zip(out, (max_records,) * 3 + (8,))]


def _check(ctx, pairs, rows, row_counts, max_pts, counts, offs, stride, max_records, gates=GATES, what="", d_rows=None):
    got = _run(ctx, pairs, rows, row_counts, max_pts, counts, offs, stride, max_records, gates, d_rows)
    exp = expected_tracks(pairs, rows, row_counts, max_pts, counts, offs, stride, max_records, gates, poison=POISON)
    for g, e, name in zip(got, exp, NAMES):
        if g.tobytes() != e.tobytes():
            bad = np.nonzero(g != e)[0]
            raise AssertionError("%s %s: %d ints differ, first at %s: got %s, expected %s"
                                 % (what, name, len(bad), bad[:8], g[bad[:8]], e[bad[:8]]))
    return got


SIZES = [300, 64, 2000, 0, 65, 1, 63, 300, 2000, 64, 65, 300]     # frame 7: count -1; frame 11: in no pair
COUNTS = SIZES[:7] + [-1] + SIZES[8:]


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
def test_planted_tracks(ctx, padded):
    """12 frames, window 3, planted tracks of length 1..12 with dropped edges, matches outside the second frame, a pair of
    row count -1; the padding and every int outside the valid records keep the poison."""
    rng = np.random.default_rng(5 + padded)
    mp = 2000
    _, offs, stride = layout(frames(SIZES, 31, True), COUNTS, padded, min_stride=2048, pad_error=0.0)
    pairs = window_pairs(list(range(11)), 3)
    assert not any(11 in p for p in pairs) and len(pairs) == 27
    rows = blank_rows(len(pairs), mp, 17)
    usable = [f for f in range(11) if COUNTS[f] > 0]
    mem = _members(SIZES, usable, [1 + t % 12 for t in range(240)], rng)
    plant(rows, mp, pairs, mem, 0.3, rng)
    row_counts = [max(COUNTS[a], 0) for a, _ in pairs]
    # matches that are no record of the second frame, on rows no track uses; two rows onto one column
    i = pairs.index((2, 4))
    spare = [r for r in range(2000) if not any(t.get(2) == r for t in mem)][:8]
    for r, m in zip(spare, [-1, -7, SIZES[4], SIZES[4] + 5, 3, 3]):
        set_edge(rows, mp, i, r, m)
    # a pair over max_pts as the matcher leaves it: row count -1, rows that would be edges
    j = pairs.index((8, 9))
    row_counts[j] = -1
    # frame 7 (count -1) has no record: rows matching into it, and rows of it, are no edges
    set_edge(rows, mp, pairs.index((6, 7)), 0, 0)
    set_edge(rows, mp, pairs.index((7, 8)), 0, 0)
    max_records = int(offs[-1]) if offs is not None else stride * len(SIZES)
    t, ln, fr, s = _check(ctx, pairs, rows, row_counts, mp, COUNTS, offs, stride, max_records, what="planted")
    assert s[1] > 100 and s[3] >= 1 and 6 <= s[4] <= 16 and s[5] == 0, s
    valid = np.zeros(max_records, bool)
    for f, c in enumerate(COUNTS):
        valid[span(offs, stride, f, max(c, 0))] = True
    for a in (t, ln, fr):
        assert (a[~valid].view(np.uint32) == POISON).all()
    f11 = span(offs, stride, 11, COUNTS[11])
    assert (t[f11] == np.arange(f11.start, f11.stop)).all() and (ln[f11] == 1).all() and (fr[f11] == 1).all()


def test_chain_through_48_frames(ctx):
    """One record per frame, every frame linked to the next: the pointer walks are as deep as the data allows."""
    nf = 48
    pairs = [(f, f + 1) for f in range(nf - 1)]
    rows = blank_rows(nf - 1, 1, 1)
    for i in range(nf - 1):
        set_edge(rows, 1, i, 0, 0)
    t, ln, fr, s = _check(ctx, pairs, rows, [1] * (nf - 1), 1, [1] * nf, np.arange(nf + 1), 0, nf, what="chain")
    assert (t == 0).all() and ln[0] == nf and fr[0] == nf and list(s) == [nf - 1, 1, nf, 0, nf, 0, 0, 0]


def test_one_root_hammered(ctx):
    """4096 rows of one pair all matching column 0: every wavefront links under one root."""
    n = 4096
    rows = blank_rows(1, n, 2)
    for r in range(n):
        set_edge(rows, n, 0, r, 0)
    offs = np.array([0, 3, 3 + n, 3 + n + 5], np.int32)         # frame 1 (the rows) behind frame 0, frame 2 the column
    t, ln, fr, s = _check(ctx, [(1, 2)], rows, [n], n, [3, n, 5], offs, 0, int(offs[-1]), what="hammer")
    assert ln[3] == n + 1 and fr[3] == 2 and (t[3:3 + n + 1] == 3).all()
    assert list(s) == [n, 1, n + 1, 1, n + 1, 0, 0, 0]


def test_components_across_every_xcd_twice(ctx):
    """32 frames x 2048 records, window 3, every planted track through all 32 frames (about 180 k edges): the records of
    one component sit in workgroups all over the chip.  Two runs: byte-identical to each other and to the restatement."""
    nf, n, mp = 32, 2048, 2048
    rng = np.random.default_rng(9)
    pairs = window_pairs(list(range(nf)), 3)
    rows = blank_rows(len(pairs), mp, 3)
    perm = np.stack([rng.permutation(n) for _ in range(nf)])     # track k holds record perm[f][k] of frame f
    for i, (f1, f2) in enumerate(pairs):
        keep = rng.random(n) >= 0.02
        o = rows[i * mp:(i + 1) * mp]
        r = perm[f1][keep]
        o["match"][r] = perm[f2][keep]
        o["score"][r] = np.float32(0.97)
        o["ambiguity"][r] = np.float32(0.3)
    counts, offs = [n] * nf, np.arange(nf + 1) * n
    d_rows = ctx.upload(rows)
    a = _check(ctx, pairs, rows, [n] * len(pairs), mp, counts, offs, 0, nf * n, what="xcd run 1", d_rows=d_rows)
    b = _run(ctx, pairs, rows, [n] * len(pairs), mp, counts, offs, 0, nf * n, d_rows=d_rows)
    for x, y, name in zip(a, b, NAMES):
        assert x.tobytes() == y.tobytes(), name
    s = a[3]
    assert s[0] > 170000 and s[1] == n and s[2] == nf * n and s[3] == 0 and s[4] == nf, s


def test_gates_on_the_device(ctx):
    """The CPU file's boundary rows: score == min_score rejected and the next float accepted, NaN fields, a finite
    max_error against match_error as set, and max_error = inf with match_error left as 0xFF poison."""
    rows, open_, tight = gate_rows()
    args = ([(0, 1)], rows, [16], 16, [16, 16], None, 16, 32)
    for gates, want in ((GATES, open_), ((0.85, 0.95, 2.0), tight)):
        t, ln, fr, s = _check(ctx, *args, gates=gates, what="gates %s" % (gates,))
        assert sorted(np.nonzero(ln[:16] == 2)[0]) == want and s[0] == len(want)
    rows = blank_rows(1, 16, 4)
    set_edge(rows, 16, 0, 5, 9)
    assert np.isnan(rows["match_error"]).all()
    t, ln, fr, s = _check(ctx, [(0, 1)], rows, [16], 16, [16, 16], None, 16, 32, what="inf")
    assert s[0] == 1 and t[16 + 9] == 5
    t, ln, fr, s = _check(ctx, [(0, 1)], rows, [16], 16, [16, 16], None, 16, 32, gates=(0.85, 0.95, 1e30), what="finite")
    assert s[0] == 0


def test_max_records_cuts_off_the_last_frame():
    """max_records one short of the last frame's end: the frame is counted in summary[5], gets no label, its edges are
    dropped, and nothing is written at or beyond max_records (buffers of exactly max_records ints, guarded)."""
    sizes = [70, 130, 64]
    offs = np.array([0, 70, 200, 264], np.int32)
    pairs = [(0, 1), (1, 2), (0, 2)]
    rows = blank_rows(3, 130, 6)
    rng = np.random.default_rng(6)
    plant(rows, 130, pairs, [{0: k, 1: 2 * k, 2: 63 - k} for k in range(60)], 0.1, rng)
    with guarded_context(4) as g:
        t, ln, fr, s = _check(g, pairs, rows, [70, 130, 70], 130, sizes, offs, 0, 263, what="cut")
        assert s[5] == 1 and 40 < s[0] <= 60 and s[4] == 2
        assert (t[200:].view(np.uint32) == POISON).all() and (ln[200:].view(np.uint32) == POISON).all()
        t, ln, fr, s = _check(g, pairs, rows, [70, 130, 70], 130, sizes, offs, 0, 264, what="whole")
        assert s[5] == 0 and s[4] == 3 and s[0] > 120


def test_argument_errors_enqueue_nothing(ctx):
    from cudasift_amd import capi
    L = capi.lib()
    nan = float("nan")
    pairs = np.array([[0, 1]], np.int32)
    rows = blank_rows(1, 8, 7)
    set_edge(rows, 8, 0, 0, 0)
    d_rows, d_rc, d_cnt = ctx.upload(rows), ctx.upload(np.array([8], np.int32)), ctx.upload(np.array([8, 8], np.int32))
    out = [_poisoned(ctx, 16) for _ in range(3)] + [_poisoned(ctx, 8)]
    good = dict(ctx=ctx.h, npairs=1, pairs=pairs.ctypes.data, rows=d_rows.ptr, rc=d_rc.ptr, max_pts=8, nframes=2,
                counts=d_cnt.ptr, offsets=None, stride=8, max_records=16, min_score=0.85, max_ambiguity=0.95,
                max_error=INF, track=out[0].ptr, len=out[1].ptr, frames=out[2].ptr, summary=out[3].ptr)

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_link_tracks_batch(*[a[k] for k in good])

    bad_pairs = [np.array([[0, 2]], np.int32), np.array([[-1, 1]], np.int32), np.array([[2, 0]], np.int32)]
    cases = [dict(ctx=None), dict(npairs=-1), dict(nframes=-1), dict(rows=None), dict(rc=None), dict(counts=None),
             dict(track=None), dict(len=None), dict(frames=None), dict(summary=None), dict(max_pts=0),
             dict(max_records=0), dict(stride=-1), dict(min_score=nan), dict(max_ambiguity=nan), dict(max_error=nan),
             dict(max_error=0.0), dict(max_error=-1.0), dict(nframes=1)]
    cases += [dict(pairs=p.ctypes.data) for p in bad_pairs]
    for kw in cases:
        assert call(**kw) == MISIFT_EINVAL, kw
    ctx.sync()
    for b, n in zip(out, (16, 16, 16, 8)):
        assert (ctx.download(b, (n,), np.uint32) == POISON).all()
    assert call() == MISIFT_OK                                  # the same arguments, unbroken
    ctx.sync()
    assert list(ctx.download(out[3], (8,), np.int32)) == [1, 1, 2, 0, 2, 0, 0, 0]


def test_no_pairs_and_no_frames(ctx):
    """npairs == 0: every valid record a singleton.  nframes == 0: only the summary is written."""
    t, ln, fr, s = _check(ctx, [], blank_rows(0, 4, 0), [], 4, [3, -1, 0, 2], None, 5, 20, what="no pairs")
    assert list(s) == [0, 0, 0, 0, 1, 0, 0, 0] and list(t[:3]) == [0, 1, 2] and list(t[15:17]) == [15, 16]
    t, ln, fr, s = _check(ctx, [], blank_rows(0, 4, 0), [], 4, [], None, 5, 20, what="no frames")
    assert list(s) == [0] * 8 and (t.view(np.uint32) == POISON).all()


def test_chain_with_no_host_read(ctx):
    """extract (packed, async) -> quantize -> mutual int8 pairs (window 3) -> find -> improve on the pair rows -> link
    with a finite max_error, no host read in between; then everything is downloaded and the four outputs must equal the
    restatement on the downloaded rows."""
    from cudasift_amd import capi
    B, h, w, mp = 4, 480, 640, 4096
    base = synth_frame(0, w, h).astype(np.float32)
    imgs = np.stack([np.roll(base, (2 * f, 3 * f), axis=(0, 1)) for f in range(B)]).astype(np.float32)
    d = ctx.upload(imgs)
    sc = capi.DevBuf(4 * capi.scratch_floats(w, h, 5, False) * B)
    cnt = ctx.zeros(4 * (2 * B + 1))
    packed = ctx.zeros(576 * mp * B)
    dq = ctx.zeros(128 * mp * B)
    capi.check(capi.lib().misift_extract_batch_packed_async(ctx.h, d.ptr, B, h * w, w, h, w, 5, 1.0, 3.0, 0.0, sc.ptr,
                                                            None, mp, cnt.ptr, cnt.ptr + 4 * B, packed.ptr),
               "misift_extract_batch_packed_async")
    ctx.quantize_batch(packed, B, cnt.ptr, cnt.ptr + 4 * B, 0, dq)
    pairs = window_pairs(list(range(B)), 3)
    npairs = len(pairs)
    assert npairs == 6
    out, oc, _ = ctx.match_pairs_batch_i8(pairs, packed, dq, B, cnt.ptr, cnt.ptr + 4 * B, 0, max_pts=mp, mutual=True)
    sel = list(range(npairs))
    gates = (0.85, 0.95, 3.0)
    dH, _ = ctx.find_homography_batch(sel, [300 + i for i in sel], out, npairs, oc, None, mp, max_pts=mp,
                                      num_loops=1000, min_score=gates[0], max_ambiguity=gates[1], thresh=5.0)
    ctx.improve_homography_batch(sel, out, npairs, oc, dH, None, mp, num_loops=5, min_score=gates[0],
                                 max_ambiguity=gates[1], thresh=3.0)
    max_records = mp * B
    bufs = [_poisoned(ctx, max_records) for _ in range(3)] + [_poisoned(ctx, 8)]
    ctx.link_tracks_batch(pairs, out, oc, mp, B, cnt.ptr, cnt.ptr + 4 * B, 0, max_records=max_records,
                          min_score=gates[0], max_ambiguity=gates[1], max_error=gates[2], track=bufs[0],
                          track_len=bufs[1], track_frames=bufs[2], summary=bufs[3])
    ctx.sync()
    ci = ctx.download(cnt, (2 * B + 1,), np.int32)
    fc, offs = ci[:B], ci[B:]
    rows = ctx.download(out, (npairs * mp,), capi.POINT_DTYPE)
    counts = ctx.download(oc, (npairs,), np.int32)
    got = [ctx.download(b, (n,), np.int32) for b, n in zip(bufs, (max_records,) * 3 + (8,))]
    assert (fc > 100).all(), fc
    exp = expected_tracks(pairs, rows, counts, mp, fc, offs, 0, max_records, gates, poison=POISON)
    for g, e, name in zip(got, exp, NAMES):
        assert g.tobytes() == e.tobytes(), (name, np.nonzero(g != e)[0][:8])
    tlen = got[1][:int(offs[B])]
    assert int((tlen >= 3).sum()) > 50, int((tlen >= 3).sum())
    assert got[3][3] == exp[3][3] == int(((tlen >= 2) & (tlen != got[2][:int(offs[B])])).sum())


def test_guard_mode():
    """One call with every allocation guarded (the library's temp memory and the outputs): no band damaged."""
    from cudasift_amd import capi
    sizes = [500, 130, 2000, 64]
    pairs = window_pairs([0, 1, 2, 3], 3) + [(2, 2)]
    rng = np.random.default_rng(12)
    rows = blank_rows(len(pairs), 2000, 8)
    plant(rows, 2000, pairs, _members(sizes, [0, 1, 2, 3], [4] * 60 + [2] * 60, rng), 0.2, rng)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    with guarded_context(6) as g:
        _check(g, pairs, rows, [sizes[a] for a, _ in pairs], 2000, sizes, offs, 0, int(offs[-1]), what="guard")
    capi.check_guards()

"""misift_match_pairs_batch_i8: int8 batch matching into pair-indexed output rows, frames repeated freely, with an
optional mutual nearest-neighbour check.

Integer scores are exact and order-free, so every comparison is byte-exact: each output row must carry set-1 record r's
xpos / ypos and the five match fields misift_match_batch_i8 on that pair writes (the numpy restatement
test_match_pairs_i8_cpu.expected_pair_i8, pinned there to brute force and to the oracle's core); with mutual = 1 a row
keeps its match only if misift_match_batch_i8 with the sets swapped names it.  Every other byte of the output, the
records, the q arrays and oversized pairs stay untouched."""
import ctypes as C

import numpy as np
import pytest

from batch_util import (POISON, POISON_WORD, fields_equal, frames, guarded_context, layout, no_match_rows, num_cus, orc,
                        span, untouched)
from synth import descriptors_to_points, synth_descriptors, synth_frame
from test_match_pairs_i8_cpu import expected_pair_i8

pytestmark = pytest.mark.gpu

SIZES1 = [0, 1, 20, 31, 32, 33, 64, 127, 128, 129, 2000, 4100, 50, 77]   # frame 12: count -1; frame 13: in no pair
COUNTS1 = SIZES1[:12] + [-1, 77]
SIZES2 = [4100, 2000, 129, 128, 127, 64, 33, 32, 31, 20, 1, 0, 300]
PAIRS = [(i, (5 * i + 2) % 13) for i in range(13)]
MISIFT_OK, MISIFT_EINVAL = 0, -1


class _Set:
    """One set of records on the device with its 8-bit descriptors (misift_quantize_batch into a patterned buffer, so
    q outside the frames is not zero); q is the host copy of what the device holds."""

    def __init__(self, ctx, recs, counts, offs, stride, seed):
        self.recs, self.counts, self.offs, self.stride = recs, list(counts), offs, stride
        self.d = ctx.upload(recs)
        self.dc = ctx.upload(np.asarray(counts, np.int32))
        self.do = ctx.upload(offs) if offs is not None else None
        pat = np.random.default_rng(seed).integers(-128, 128, (max(len(recs), 1), 128)).astype(np.int8)
        self.dq = ctx.upload(pat)
        ctx.quantize_batch(self.d, len(counts), self.dc, self.do, stride, self.dq)
        ctx.sync()
        self.q = ctx.download(self.dq, pat.shape, np.int8)

    def frame(self, f):
        n = max(int(self.counts[f]), 0)
        sl = span(self.offs, self.stride, f, n)
        return self.recs[sl], self.q[sl]

    def unchanged(self, ctx, what):
        from cudasift_amd import capi
        assert ctx.download(self.d, (len(self.recs),), capi.POINT_DTYPE).tobytes() == self.recs.tobytes(), what + " written"
        assert ctx.download(self.dq, self.q.shape, np.int8).tobytes() == self.q.tobytes(), "q of " + what + " written"


def _run(ctx, pairs, s1, s2, max_pts, mutual):
    """One misift_match_pairs_batch_i8 on poisoned output; returns (out records, counts, num_matched)."""
    from cudasift_amd import capi
    npairs = len(pairs)
    out = ctx.upload(np.full(npairs * max_pts * 576, POISON, np.uint8))
    oc = ctx.upload(np.full(npairs, POISON_WORD, np.int32))
    nm = ctx.upload(np.full(npairs, POISON_WORD, np.int32))
    ctx.match_pairs_batch_i8(pairs, s1.d, s1.dq, len(s1.counts), s1.dc, s1.do, s1.stride, s2.d, s2.dq, len(s2.counts),
                             s2.dc, s2.do, s2.stride, max_pts=max_pts, mutual=mutual, out=out, out_counts=oc,
                             num_matched=nm)
    ctx.sync()
    return (ctx.download(out, (npairs * max_pts,), capi.POINT_DTYPE), ctx.download(oc, (npairs,), np.int32),
            ctx.download(nm, (npairs,), np.int32))


def _check(ctx, pairs, s1, s2, mutual, max_pts=4100, cache=None):
    """Run and compare every pair with the restatement.  cache: expected rows by (f1, f2, mutual), for calls that
    repeat the same frames."""
    got, oc, nm = _run(ctx, pairs, s1, s2, max_pts, mutual)
    s1.unchanged(ctx, "set 1")
    if s2 is not s1:
        s2.unchanged(ctx, "set 2")
    exp_counts = []
    for i, (f1, f2) in enumerate(pairs):
        (p1, q1), (p2, q2) = s1.frame(f1), s2.frame(f2)
        n1, n2 = len(p1), len(p2)
        if n1 > max_pts or n2 > max_pts:
            assert oc[i] == -1 and nm[i] == -1, (i, oc[i], nm[i])
            exp_counts.append(-1)
            continue
        assert oc[i] == n1, (i, oc[i], n1)
        exp_counts.append(n1)
        key = (f1, f2, mutual)
        if cache is None or key not in cache:
            ek = expected_pair_i8(p1, q1, p2, q2, mutual)
            if cache is not None:
                cache[key] = ek
        else:
            ek = cache[key]
        fields_equal(got[i * max_pts:i * max_pts + n1], ek[0], "pair %d (%d x %d)" % (i, n1, n2))
        assert nm[i] == ek[1], (i, nm[i], ek[1])
    untouched(got, exp_counts, max_pts)
    return got, oc, nm


@pytest.mark.parametrize("padded", [False, True])
def test_same_answer_as_match_batch_i8(ctx, padded):
    """Each set-1 frame in one pair: the seven fields equal the restatement and misift_match_batch_i8's set-1 rows byte
    for byte; match_full / match_exact_top2 change nothing."""
    from cudasift_amd import capi
    r1, o1, st1 = layout(frames(SIZES1, 3, True), COUNTS1, padded, min_stride=1, pad_error=0.0)
    r2, o2, st2 = layout(frames(SIZES2, 4, True), SIZES2, padded, min_stride=1, pad_error=0.0)
    s1, s2 = _Set(ctx, r1, COUNTS1, o1, st1, 1), _Set(ctx, r2, SIZES2, o2, st2, 2)
    got, oc, nm = _check(ctx, PAIRS, s1, s2, 0)
    ctx.set_options(match_full=1, match_exact_top2=1)
    try:
        again = _run(ctx, PAIRS, s1, s2, 4100, 0)
    finally:
        ctx.set_options(match_full=0, match_exact_top2=0)
    assert again[0].tobytes() == got.tobytes() and np.array_equal(again[1], oc) and np.array_equal(again[2], nm)
    d1 = ctx.upload(r1)
    ctx.match_batch_i8(PAIRS, d1, s1.dq, len(COUNTS1), s1.dc, s1.do, st1, s2.d, s2.dq, len(SIZES2), s2.dc, s2.do, st2)
    ctx.sync()
    mb = ctx.download(d1, (len(r1),), capi.POINT_DTYPE)
    seen = set()
    for i, (a, b) in enumerate(PAIRS):
        n1, n2 = max(COUNTS1[a], 0), SIZES2[b]
        if n1 == 0:
            assert oc[i] == 0 and nm[i] == 0
            seen.add("n1 == 0")
            continue
        rows = got[i * 4100:i * 4100 + n1]
        if n2 == 0:
            fields_equal(rows, no_match_rows(r1[span(o1, st1, a, n1)]), "empty set 2")
            assert nm[i] == 0
            seen.add("n2 == 0")
            continue
        fields_equal(rows, mb[span(o1, st1, a, n1)], "pair %d against misift_match_batch_i8" % i)
    assert seen == {"n1 == 0", "n2 == 0"}


def _i8_plan(n1, n2):
    """(chunks of the call, plan rows) of misift_match_batch_i8's planner, the one misift_match_pairs_batch_i8 runs."""
    from cudasift_amd import capi
    n1 = np.asarray(n1, np.int32)
    n2 = np.asarray(n2, np.int32)
    plan5 = np.zeros((len(n1), 5), np.int32)
    ni, ch, pb = C.c_int(), C.c_int(), C.c_int()
    capi.check(capi.lib().misift_test_match_i8_plan(num_cus(), len(n1), n1.ctypes.data, n2.ctypes.data,
                                                    plan5.ctypes.data, C.byref(ni), C.byref(ch), C.byref(pb)),
               "misift_test_match_i8_plan")
    return ch.value, plan5


@pytest.mark.parametrize("mutual", [0, 1])
def test_many_to_many(ctx, mutual):
    """Windowed, keyframe (both directions), self pairs, d_recs1 == d_recs2 with d_q1 == d_q2 and separate buffers, in
    an unchunked and a chunked plan.  An unchunked plan needs 16 * num_cus row blocks: every ordered pair of nf frames
    of 16 row blocks each (which holds the windows f, f + 1 .. f + 3, every keyframe in both directions and the self
    pairs), nf * nf >= num_cus."""
    cus = num_cus()
    nf = max(16, int(np.ceil(np.sqrt(cus))))
    sizes = [1930 + 7 * (f % 16) for f in range(nf)]            # 1921 .. 2048 records: 16 row blocks each
    r, o, s = layout(frames(sizes, 7, True), sizes, False, min_stride=1, pad_error=0.0)
    pairs = [(f, g) for f in range(nf) for g in range(nf)]
    for must in [(2, 3), (2, 4), (2, 5), (15, 0), (0, 15), (3, 3)]:
        assert must in pairs
    ch, plan = _i8_plan([sizes[a] for a, _ in pairs], [sizes[b] for _, b in pairs])
    assert ch == 1 and (plan[:, 1] == 16).all() and (plan[:, 3] == 1).all() and plan[:, 1].sum() >= 16 * cus, (ch, plan[:3])
    same = _Set(ctx, r, sizes, o, s, 5)
    cache = {}
    _check(ctx, pairs, same, same, mutual, max_pts=2048, cache=cache)
    other = _Set(ctx, r.copy(), sizes, o, s, 6)
    assert np.array_equal(other.q[:len(r)], same.q[:len(r)])
    _check(ctx, pairs, same, other, mutual, max_pts=2048, cache=cache)
    big = [3000, 2500, 2800]
    r, o, s = layout(frames(big, 8, True), big, True, min_stride=1, pad_error=0.0)
    pairs = [(0, 1), (0, 2), (1, 0), (2, 2)]
    ch, plan = _i8_plan([big[a] for a, _ in pairs], [big[b] for _, b in pairs])
    assert ch > 1 and (plan[:, 3] > 1).all(), (ch, plan)
    same = _Set(ctx, r, big, o, s, 7)
    _check(ctx, pairs, same, same, mutual, max_pts=3000)
    _check(ctx, pairs, same, _Set(ctx, r.copy(), big, o, s, 8), mutual, max_pts=3000)


def _tie_frames():
    """Set 1 with three equal rows, two rows equal to a column, an all-zero row and a row that quantises to zero; set 2
    with duplicate columns.  L2-normalised descriptors: a row's best column is its own copy."""
    from cudasift_amd import capi
    d1 = synth_descriptors(300, 71, True)
    d2 = synth_descriptors(260, 72, True)
    d1[10] = d1[3]
    d1[11] = d1[3]                                   # three equal rows: the smallest (3) must win their column
    d1[200] = d2[40]
    d1[201] = d2[40]                                 # two rows equal to a column
    d1[50] = 0.0                                     # all-zero row: every score 0, never a match
    d1[51] = -d1[52]                                 # quantises to zero
    d2[100] = d2[40]                                 # duplicate columns: the smaller column wins the row
    d2[101] = d1[3]
    d2[102] = d1[3]
    p1 = descriptors_to_points(d1, capi.POINT_DTYPE)
    p2 = descriptors_to_points(d2, capi.POINT_DTYPE)
    p1["xpos"] += 0.25
    p2["ypos"] += 0.5
    return p1, p2


def test_mutual_rule_with_ties(ctx):
    p1, p2 = _tie_frames()
    r1 = np.concatenate([p1, p1])
    r2 = np.concatenate([p2, p2[:130]])
    s1 = _Set(ctx, r1, [300, 300], np.array([0, 300, 600], np.int32), 0, 3)
    s2 = _Set(ctx, r2, [260, 130], np.array([0, 260, 390], np.int32), 0, 4)
    assert (s1.q[51] == 0).all() and (s1.q[50] == 0).all() and s1.q[52].any()
    pairs = [(0, 0), (1, 0), (0, 1), (1, 1)]
    fw = _check(ctx, pairs, s1, s2, 0, max_pts=300)[0][:300]
    assert list(fw["match"][[3, 10, 11]]) == [101, 101, 101] and list(fw["match"][[200, 201]]) == [40, 40]
    assert fw["match"][50] == -1 and fw["match"][51] == -1
    assert fw["ambiguity"][3] == fw["score"][3] / (fw["score"][3] + np.float32(1e-6))      # the duplicate is second
    got, _, nm = _check(ctx, pairs, s1, s2, 1, max_pts=300)
    rows = got[:300]
    assert rows["match"][50] == -1 and rows["match"][51] == -1
    assert rows["match"][3] == 101 and rows["match"][10] == -1 and rows["match"][11] == -1
    assert rows["match"][200] == 40 and rows["match"][201] == -1
    assert rows["score"][201] == 0 and rows["ambiguity"][201] == 0 and rows["match_xpos"][201] == 0
    assert 0 < nm[0] < 300
    # pair 2: set 2 cut to 130 columns, the copies at 40, 100, 101, 102 remain
    assert got[600 + 3]["match"] == 101 and got[600 + 200]["match"] == 40 and got[600 + 201]["match"] == -1


def test_oversized_pairs_and_argument_errors(ctx):
    from cudasift_amd import capi
    sizes = [100, 700, 40]
    r, o, s = layout(frames(sizes, 9, True), sizes, False, min_stride=1, pad_error=0.0)
    st = _Set(ctx, r, sizes, o, s, 9)
    pairs = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]
    got, oc, nm = _check(ctx, pairs, st, st, 1, max_pts=512)
    assert list(oc) == [-1, -1, 100, 40, -1] and nm[0] == -1 and nm[1] == -1 and nm[4] == -1
    L = capi.lib()
    d, dq, dc, do = st.d, st.dq, st.dc, st.do
    out = ctx.upload(np.full(2 * 512 * 576, POISON, np.uint8))
    oc = ctx.upload(np.full(2, 7, np.int32))
    nmb = ctx.upload(np.full(2, 7, np.int32))

    def call(pl, npairs=None, h=ctx.h, recs1=d.ptr, q1=dq.ptr, counts1=dc.ptr, offs1=do.ptr, stride1=0, recs2=d.ptr,
             q2=dq.ptr, counts2=dc.ptr, offs2=do.ptr, stride2=0, max_pts=512, mutual=1, o_=out.ptr, oc_=oc.ptr,
             nm_=nmb.ptr):
        pl = np.ascontiguousarray(pl, np.int32).reshape(-1, 2)
        return L.misift_match_pairs_batch_i8(h, len(pl) if npairs is None else npairs, pl.ctypes.data, recs1, q1, 3,
                                             counts1, offs1, stride1, recs2, q2, 3, counts2, offs2, stride2, max_pts,
                                             mutual, o_, oc_, nm_)
    ok = [(0, 2), (2, 2)]
    bad = [dict(h=None), dict(npairs=-1), dict(pl=[(0, 3), (1, 1)]), dict(pl=[(3, 0), (1, 1)]),
           dict(pl=[(-1, 0), (1, 1)]), dict(pl=[(0, -1), (1, 1)]), dict(recs1=None), dict(recs2=None), dict(q1=None),
           dict(q2=None), dict(counts1=None), dict(counts2=None), dict(o_=None), dict(oc_=None), dict(q1=dq.ptr + 8),
           dict(q2=dq.ptr + 4), dict(max_pts=0), dict(max_pts=-5), dict(mutual=2), dict(mutual=-1), dict(o_=d.ptr),
           dict(offs1=None, stride1=-1), dict(offs2=None, stride2=-1)]
    for kw in bad:
        kw = dict(kw)
        pl = kw.pop("pl", ok)
        assert call(pl, **kw) == MISIFT_EINVAL, kw
    assert call(ok, npairs=0) == MISIFT_OK
    ctx.sync()
    assert (ctx.download(out, (2 * 512 * 576,), np.uint8) == POISON).all(), "an argument error enqueued work"
    assert list(ctx.download(oc, (2,), np.int32)) == [7, 7] and list(ctx.download(nmb, (2,), np.int32)) == [7, 7]
    st.unchanged(ctx, "the set")
    assert call(ok, nm_=None) == MISIFT_OK                  # d_num_matched may be NULL
    ctx.sync()
    assert list(ctx.download(oc, (2,), np.int32)) == [100, 40]
    assert list(ctx.download(nmb, (2,), np.int32)) == [7, 7]
    rows = ctx.download(out, (2 * 512,), capi.POINT_DTYPE)
    for i, (a, b) in enumerate(ok):
        (p1, q1), (p2, q2) = st.frame(a), st.frame(b)
        fields_equal(rows[i * 512:i * 512 + len(p1)], expected_pair_i8(p1, q1, p2, q2, 1)[0], "NULL num_matched")


def test_chain_with_no_host_read(ctx):
    """extract (packed, async) -> quantize -> mutual int8 pairs -> misift_find_homography_batch on the output as it is,
    no host read in between: H and inlier counts equal srand(seed) + misift_find_homography on the downloaded rows."""
    from cudasift_amd import capi
    o = orc()
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
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (3, 0)]
    npairs = len(pairs)
    out, oc, nm = ctx.match_pairs_batch_i8(pairs, packed, dq, B, cnt.ptr, cnt.ptr + 4 * B, 0, max_pts=mp, mutual=True)
    seeds = [200 + i for i in range(npairs)]
    FIND = dict(num_loops=1000, min_score=0.85, max_ambiguity=0.95, thresh=5.0)
    dH, dn = ctx.find_homography_batch(list(range(npairs)), seeds, out, npairs, oc, None, mp, max_pts=mp, **FIND)
    ctx.sync()
    ci = ctx.download(cnt, (2 * B + 1,), np.int32)
    fc, offs = ci[:B], ci[B:]
    counts = ctx.download(oc, (npairs,), np.int32)
    nmatch = ctx.download(nm, (npairs,), np.int32)
    H = ctx.download(dH, (npairs, 3, 3), np.float32)
    num = ctx.download(dn, (npairs,), np.int32)
    rows = ctx.download(out, (npairs * mp,), capi.POINT_DTYPE)
    recs = ctx.download(packed, (int(offs[B]),), capi.POINT_DTYPE)
    q = ctx.download(dq, (int(offs[B]), 128), np.int8)
    assert (fc > 100).all(), fc
    for i, (f1, f2) in enumerate(pairs):
        n = int(counts[i])
        assert n == fc[f1]
        sel = rows[i * mp:i * mp + n].copy()
        a, b = slice(offs[f1], offs[f1] + fc[f1]), slice(offs[f2], offs[f2] + fc[f2])
        e, k = expected_pair_i8(recs[a], q[a], recs[b], q[b], 1)
        fields_equal(sel, e, "chain pair %d" % i)
        assert nmatch[i] == k == int((sel["match"] >= 0).sum()) and 0 < nmatch[i] < n, (i, nmatch[i], n)
        gated = int(((sel["match"] >= 0) & (sel["score"] > FIND["min_score"]) &
                     (sel["ambiguity"] < FIND["max_ambiguity"])).sum())
        assert gated > 50, (i, gated)
        dm = ctx.upload(sel)
        o.srand(seeds[i])
        He, ne = ctx.find_homography(dm.ptr, n, **FIND)
        assert num[i] == ne and np.array_equal(H[i].view(np.uint32), np.asarray(He, np.float32).view(np.uint32)), i
        assert num[i] > 50, num


def test_guard_mode(ctx):
    """One mutual call, chunked, with every allocation guarded: no band damaged."""
    from cudasift_amd import capi
    sizes = [500, 130, 2000]
    pairs = [(0, 1), (1, 2), (2, 0), (2, 2)]
    ch, _ = _i8_plan([sizes[a] for a, _ in pairs], [sizes[b] for _, b in pairs])
    assert ch > 1
    with guarded_context(None) as g:
        r, o, s = layout(frames(sizes, 11, True), sizes, False, min_stride=1, pad_error=0.0)
        st = _Set(g, r, sizes, o, s, 11)
        _check(g, pairs, st, st, 1, max_pts=2000)
    capi.check_guards()

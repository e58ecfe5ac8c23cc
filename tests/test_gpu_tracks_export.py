"""misift_export_tracks_batch on the device: the labels of misift_link_tracks_batch turned into compact observation
lists (selected roots numbered in ascending order, a prefix sum of their lengths, the members of each track in ascending
index order).

Most cases fabricate the label arrays in numpy (test_tracks_cpu.expected_tracks on planted rows, or written out
directly) and upload them, so no matcher and no linker has to run.  Every output buffer has exactly the capacity given
and is poisoned first; every comparison is byte equality with test_tracks_export_cpu.expected_export (pinned there to a
dictionary version): all outputs are integers or copied bit patterns, and none depends on the order of an atomic."""
import functools

import numpy as np
import pytest

from batch_util import fabricated_records, guarded_context, xy_bits
from synth import synth_frame
from test_gpu_tracks import COUNTS, SIZES, _members
from test_tracks_cpu import GATES, blank_rows, expected_tracks, plant, set_edge, window_pairs
from test_tracks_export_cpu import NAMES, expected_export

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
MISIFT_OK, MISIFT_EINVAL = 0, -1
LAUNCHES = 6                                                     # include/misift.h: one memset and six launches


def _poisoned(ctx, nints):
    return ctx.upload(np.full(max(nints, 1), POISON, np.uint32))


class Batch:
    """The device side of one layout and its labels: uploaded once, exported as often as a test likes."""

    def __init__(self, ctx, recs, counts, offs, stride, max_records, labels, d_recs=None):
        self.ctx, self.xy = ctx, xy_bits(recs)
        self.counts, self.offs, self.stride, self.max_records = list(counts), offs, stride, max_records
        self.labels = [np.ascontiguousarray(a[:max_records], np.int32) for a in labels]
        self.d_recs = d_recs if d_recs is not None else ctx.upload(recs)
        self.d_cnt = ctx.upload(np.asarray(self.counts if self.counts else [0], np.int32))
        self.d_off = ctx.upload(np.asarray(offs, np.int32)) if offs is not None else None
        self.d_lab = [ctx.upload(a) for a in self.labels]

    def run(self, min_len, cons, max_tracks, max_obs, record_obs=True):
        """One call on poisoned outputs of exactly the capacities given; the five arrays as downloaded (record_obs None
        when it is left out)."""
        from cudasift_amd import capi
        ctx, n = self.ctx, self.max_records
        out = [_poisoned(ctx, max_tracks + 1), _poisoned(ctx, max_tracks), _poisoned(ctx, 4 * max_obs),
               _poisoned(ctx, n) if record_obs else None, _poisoned(ctx, 8)]
        ctx.export_tracks_batch(self.d_recs, len(self.counts), self.d_cnt, self.d_off, self.stride, max_records=n,
                                track=self.d_lab[0], track_len=self.d_lab[1], track_frames=self.d_lab[2],
                                min_len=min_len, consistent_only=cons, max_tracks=max_tracks, max_obs=max_obs,
                                track_offsets=out[0], track_root=out[1], obs=out[2], record_obs=out[3], summary=out[4])
        ctx.sync()
        shapes = ((max_tracks + 1,), np.int32), ((max_tracks,), np.int32), ((max_obs,), capi.TRACK_OBS_DTYPE), \
            ((n,), np.int32), ((8,), np.int32)
        return [ctx.download(b, *s) if b is not None else None for b, s in zip(out, shapes)]

    def expected(self, min_len, cons, max_tracks, max_obs):
        return expected_export(self.xy, self.counts, self.offs, self.stride, self.max_records, *self.labels, min_len,
                               cons, max_tracks, max_obs, POISON)

    def check(self, min_len, cons, max_tracks=None, max_obs=None, what="", record_obs=True):
        max_tracks = self.max_records if max_tracks is None else max_tracks
        max_obs = self.max_records if max_obs is None else max_obs
        got = self.run(min_len, cons, max_tracks, max_obs, record_obs)
        exp = self.expected(min_len, cons, max_tracks, max_obs)
        for g, e, name in zip(got, exp, NAMES):
            if g is None:
                continue
            if g.tobytes() != e.tobytes():
                a, b = g.view(np.uint32).reshape(len(g), -1), e.view(np.uint32).reshape(len(e), -1)
                bad = np.nonzero((a != b).any(1))[0]
                raise AssertionError("%s %s: %d entries differ, first at %s: got %s, expected %s"
                                     % (what, name, len(bad), bad[:8], a[bad[:4]].tolist(), b[bad[:4]].tolist()))
        return got


# ---- planted tracks

@functools.lru_cache(maxsize=None)
def planted_case(padded):
    """The frames, window and planted tracks of test_gpu_tracks.test_planted_tracks (12 frames of 300, 64, 2000, 0, 65,
    1, 63, 300 with count -1, 2000, 64, 65, 300 records; tracks of length 1..12 with dropped edges; two rows onto one
    column), labelled by expected_tracks.  Computed once per layout and left unchanged."""
    rng = np.random.default_rng(5 + padded)
    mp = 2000
    if padded:
        offs, stride = None, 2048
        max_records = stride * len(SIZES)
    else:
        offs, stride = np.concatenate([[0], np.cumsum(np.maximum(COUNTS, 0))]).astype(np.int32), 0
        max_records = int(offs[-1])
    pairs = window_pairs(list(range(11)), 3)
    rows = blank_rows(len(pairs), mp, 17)
    usable = [f for f in range(11) if COUNTS[f] > 0]
    mem = _members(SIZES, usable, [1 + t % 12 for t in range(240)], rng)
    plant(rows, mp, pairs, mem, 0.3, rng)
    spare = [r for r in range(2000) if not any(t.get(2) == r for t in mem)][:2]
    for r in spare:
        set_edge(rows, mp, pairs.index((2, 4)), r, 3)           # two rows onto one column: an inconsistent track
    row_counts = [max(COUNTS[a], 0) for a, _ in pairs]
    labels = expected_tracks(pairs, rows, row_counts, mp, COUNTS, offs, stride, max_records, GATES, poison=POISON)
    assert labels[3][3] >= 1
    return fabricated_records(max_records, 40 + padded), offs, stride, max_records, labels[:3]


def planted_batch(ctx, padded):
    recs, offs, stride, max_records, labels = planted_case(padded)
    return Batch(ctx, recs, COUNTS, offs, stride, max_records, labels)


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
def test_planted_tracks(ctx, padded):
    """Four (min_len, consistent_only) filters on one uploaded batch; the positions are random bit patterns, NaN
    payloads included, and come back bit for bit.  The filter bites: more than 100 consistent tracks, and strictly more
    observations without the consistency rule."""
    b = planted_batch(ctx, padded)
    assert np.isnan(b.xy.view(np.float32)).any()
    s = {}
    for min_len, cons in ((1, 0), (2, 0), (2, 1), (3, 1)):
        got = b.check(min_len, cons, what="planted %d %d" % (min_len, cons))
        s[min_len, cons] = got[4]
        assert got[4][0] == got[4][2] and got[4][5] == 0
    assert s[2, 1][2] > 100 and s[2, 0][3] > s[2, 1][3] and s[2, 0][2] > s[2, 1][2], s
    assert s[1, 0][3] == sum(max(c, 0) for c in COUNTS) and s[3, 1][2] < s[2, 1][2]


# ---- the scan

def pair_labels(N):
    """Two packed frames of N // 2 and N - N // 2 records; record i is paired with record i + N // 2 for every third i,
    the rest are singletons: the labels misift_link_tracks_batch gives for those edges, written out directly."""
    h = N // 2
    track = np.arange(N, dtype=np.int32)
    tlen = np.ones(N, np.int32)
    i = np.arange(0, h, 3)
    track[i + h] = i
    tlen[i], tlen[i + h] = 2, 0
    return [h, N - h], np.array([0, h, N], np.int32), (track, tlen, tlen.copy())


def scan_sizes():
    sizes = {1, 2, 63, 64, 65, 65536, 131077}
    for n in range(256, 8192 + 1, 256):
        sizes |= {n - 1, n, n + 1}
    return sorted(sizes)


def test_pair_labels_are_the_linkers():
    N = 26
    counts, offs, labels = pair_labels(N)
    rows = blank_rows(1, 13, 1)
    for i in range(0, 13, 3):
        set_edge(rows, 13, 0, i, i)
    exp = expected_tracks([(0, 1)], rows, [13], 13, counts, offs, 0, N, GATES)
    for a, e in zip(labels, exp[:3]):
        assert np.array_equal(a, e)


def test_scan_boundaries(ctx):
    """The device-wide prefix sum at and around every multiple of 256 up to 8192 (the scan tile is 2048 indices, a lane
    owns 8 of them, a workgroup 256 lanes), at 1, 2, 63, 64, 65, and at 65 536 and 131 077 (32 and 65 tiles).  One
    context and one records array serve every size; min_len = 2, so only the pairs are tracks."""
    sizes = scan_sizes()
    recs = fabricated_records(sizes[-1], 3)
    d_recs = ctx.upload(recs)
    for N in sizes:
        counts, offs, labels = pair_labels(N)
        b = Batch(ctx, recs[:N], counts, offs, 0, N, labels, d_recs=d_recs)
        T = (N // 2 + 2) // 3
        got = b.check(2, 1, max_tracks=T + 1, max_obs=2 * T + 1, what="scan N=%d" % N)
        assert list(got[4]) == [T, 2 * T, T, 2 * T, 2 if T else 0, 0, 0, 0], (N, got[4])


# ---- one giant track

def test_one_giant_track(ctx):
    """4096 records of one frame and one of another under one root, small tracks before and behind it.  Without the
    consistency rule it is written, its 4097 observations in ascending index order; with it the track is absent and the
    others keep their numbering."""
    n = 4096
    pairs = [(0, 2), (1, 2), (2, 3)]
    rows = blank_rows(3, n, 2)
    for r in range(3):
        set_edge(rows, n, 0, r, r + 1)                          # frame 0 -> frame 2: three tracks of 2
    for r in range(n):
        set_edge(rows, n, 1, r, 0)                              # frame 1 -> record 0 of frame 2: the giant
    set_edge(rows, n, 2, 4, 0)                                  # frame 2 -> frame 3: a track of 2 behind the giant's root
    counts = [3, n, 5, 4]
    offs = np.array([0, 3, 3 + n, 8 + n, 12 + n], np.int32)
    total = int(offs[-1])
    labels = expected_tracks(pairs, rows, [3, n, 5], n, counts, offs, 0, total, GATES)[:3]
    b = Batch(ctx, fabricated_records(total, 4), counts, offs, 0, total, labels)
    off, root, obs, rob, s = b.check(2, 0, what="giant")
    assert list(root[:5]) == [0, 1, 2, 3, 3 + n + 4] and list(off[:6]) == [0, 2, 4, 6, 6 + n + 1, 8 + n + 1]
    giant = obs[6:6 + n + 1]
    assert list(giant["frame"]) == [1] * n + [2] and list(giant["record"]) == list(range(n)) + [0]
    assert list(s) == [5, n + 9, 5, n + 9, n + 1, 0, 0, 0]
    off, root, obs, rob, s = b.check(2, 1, what="giant left out")
    assert list(root[:4]) == [0, 1, 2, 3 + n + 4] and list(off[:5]) == [0, 2, 4, 6, 8]
    assert list(s) == [4, 8, 4, 8, 2, 0, 0, 0] and (rob[3:3 + n + 1] == -1).all()


def test_chain_through_48_frames(ctx):
    nf = 48
    rows = blank_rows(nf - 1, 1, 1)
    for i in range(nf - 1):
        set_edge(rows, 1, i, 0, 0)
    pairs = [(f, f + 1) for f in range(nf - 1)]
    offs = np.arange(nf + 1, dtype=np.int32)
    labels = expected_tracks(pairs, rows, [1] * (nf - 1), 1, [1] * nf, offs, 0, nf, GATES)[:3]
    b = Batch(ctx, fabricated_records(nf, 5), [1] * nf, offs, 0, nf, labels)
    off, root, obs, rob, s = b.check(2, 1, max_tracks=1, max_obs=nf, what="chain")
    assert list(off) == [0, nf] and list(root) == [0] and list(obs["frame"]) == list(range(nf))
    assert (obs["record"] == 0).all() and list(rob) == list(range(nf)) and list(s) == [1, nf, 1, nf, nf, 0, 0, 0]


def test_components_across_the_chip_twice(ctx):
    """32 frames x 2048 records, every planted track through all 32 frames, labelled by one real
    misift_link_tracks_batch call on fabricated rows (as test_gpu_tracks.test_components_across_every_xcd_twice).  The
    members of one track sit in workgroups all over the chip.  Two exports: byte-identical to each other and to the
    restatement on the downloaded labels."""
    nf, n, mp = 32, 2048, 2048
    rng = np.random.default_rng(9)
    pairs = window_pairs(list(range(nf)), 3)
    rows = blank_rows(len(pairs), mp, 3)
    perm = np.stack([rng.permutation(n) for _ in range(nf)])
    for i, (f1, f2) in enumerate(pairs):
        keep = rng.random(n) >= 0.02
        o = rows[i * mp:(i + 1) * mp]
        r = perm[f1][keep]
        o["match"][r] = perm[f2][keep]
        o["score"][r] = np.float32(0.97)
        o["ambiguity"][r] = np.float32(0.3)
    total = nf * n
    offs = (np.arange(nf + 1) * n).astype(np.int32)
    d_rows, d_rc = ctx.upload(rows), ctx.upload(np.full(len(pairs), n, np.int32))
    d_cnt, d_off = ctx.upload(np.full(nf, n, np.int32)), ctx.upload(offs)
    lab = ctx.link_tracks_batch(pairs, d_rows, d_rc, mp, nf, d_cnt, d_off, 0, max_records=total)
    ctx.sync()
    labels = [ctx.download(a, (total,), np.int32) for a in lab[:3]]
    b = Batch(ctx, fabricated_records(total, 6), [n] * nf, offs, 0, total, labels)
    first = b.check(2, 1, what="chip run 1")
    second = b.run(2, 1, total, total)
    for x, y, name in zip(first, second, NAMES):
        assert x.tobytes() == y.tobytes(), name
    assert list(first[4]) == [n, total, n, total, nf, 0, 0, 0]


# ---- capacity, max_records, record_obs = NULL

GUARD_SIZES = [500, 130, 2000, 64]


@functools.lru_cache(maxsize=None)
def guard_case():
    pairs = window_pairs([0, 1, 2, 3], 3) + [(2, 2)]
    rng = np.random.default_rng(12)
    rows = blank_rows(len(pairs), 2000, 8)
    plant(rows, 2000, pairs, _members(GUARD_SIZES, [0, 1, 2, 3], [4] * 60 + [2] * 60, rng), 0.2, rng)
    offs = np.concatenate([[0], np.cumsum(GUARD_SIZES)]).astype(np.int32)
    total = int(offs[-1])
    labels = expected_tracks(pairs, rows, [GUARD_SIZES[a] for a, _ in pairs], 2000, GUARD_SIZES, offs, 0, total, GATES)
    return fabricated_records(total, 7), offs, total, labels[:3]


def test_capacity():
    """Output buffers of exactly the capacities given, every allocation guarded.  max_tracks = T - 1; max_obs one short
    of the end of the last track; max_obs in the middle of an early track; both generous.  summary[0..3] tells the cases
    apart, everything at and beyond the written prefix keeps the poison and the records of cut tracks get -1 (both by
    the comparison with the restatement, and spelled out here)."""
    recs, offs, total, labels = guard_case()
    with guarded_context(6) as g:
        b = Batch(g, recs, GUARD_SIZES, offs, 0, total, labels)
        whole = b.check(2, 1, max_tracks=total, max_obs=total, what="generous")
        T, O = int(whole[4][2]), int(whole[4][3])
        off = whole[0]
        assert T > 60 and list(whole[4][:4]) == [T, O, T, O]
        early = int(off[3]) + 1
        assert off[3] < early < off[4]
        for max_tracks, max_obs, t, what in ((T - 1, total, T - 1, "max_tracks"), (T + 5, O - 1, T - 1, "last track"),
                                             (T + 5, early, 3, "early track"), (T + 5, O + 7, T, "both generous")):
            o = int(off[t])
            got_off, root, obs, rob, s = b.check(2, 1, max_tracks=max_tracks, max_obs=max_obs, what=what)
            assert list(s[:4]) == [T, O, t, o], (what, s)
            assert (got_off[t + 1:].view(np.uint32) == POISON).all() and (root[t:].view(np.uint32) == POISON).all()
            assert (obs[o:].view(np.uint32) == POISON).all()
            cut = whole[3] >= o                                  # the records of the tracks that are cut now
            assert (rob[cut] == -1).all() and (rob[~cut] == whole[3][~cut]).all()


def test_max_records_cuts_off_the_last_frame():
    """max_records one short of the last frame's end: summary[5] == 1, that frame's records appear in no track and their
    record_obs slots keep the poison."""
    sizes = [70, 130, 64]
    offs = np.array([0, 70, 200, 264], np.int32)
    pairs = [(0, 1), (1, 2), (0, 2)]
    rows = blank_rows(3, 130, 6)
    plant(rows, 130, pairs, [{0: k, 1: 2 * k, 2: 63 - k} for k in range(60)], 0.1, np.random.default_rng(6))
    labels = expected_tracks(pairs, rows, [70, 130, 70], 130, sizes, offs, 0, 263, GATES, poison=POISON)[:3]
    with guarded_context(6) as g:
        b = Batch(g, fabricated_records(264, 8), sizes, offs, 0, 263, labels)
        _, _, obs, rob, s = b.check(2, 1, max_tracks=100, max_obs=263, what="cut")
        assert s[5] == 1 and s[2] > 40 and s[4] == 2
        assert (obs["frame"][:s[3]] < 2).all() and (rob[200:].view(np.uint32) == POISON).all()


def test_record_obs_may_be_null(ctx):
    b = planted_batch(ctx, False)
    with_it = b.check(2, 1, what="with record_obs")
    without = b.check(2, 1, what="without record_obs", record_obs=False)
    assert without[3] is None
    for k in (0, 1, 2, 4):
        assert with_it[k].tobytes() == without[k].tobytes(), NAMES[k]


def test_argument_errors_enqueue_nothing(ctx):
    from cudasift_amd import capi
    L = capi.lib()
    counts, offs, labels = pair_labels(16)
    recs = fabricated_records(16, 9)
    d_recs, d_cnt, d_off = ctx.upload(recs), ctx.upload(np.asarray(counts, np.int32)), ctx.upload(offs)
    d_lab = [ctx.upload(a) for a in labels]
    out = [_poisoned(ctx, 9), _poisoned(ctx, 8), _poisoned(ctx, 4 * 16), _poisoned(ctx, 16), _poisoned(ctx, 8)]
    good = dict(ctx=ctx.h, recs=d_recs.ptr, nframes=2, counts=d_cnt.ptr, offsets=d_off.ptr, stride=0, max_records=16,
                track=d_lab[0].ptr, len=d_lab[1].ptr, frames=d_lab[2].ptr, min_len=2, consistent_only=1, max_tracks=8,
                max_obs=16, track_offsets=out[0].ptr, track_root=out[1].ptr, obs=out[2].ptr, record_obs=out[3].ptr,
                summary=out[4].ptr)

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_export_tracks_batch(*[a[k] for k in good])

    cases = [dict(ctx=None), dict(nframes=-1), dict(recs=None), dict(counts=None), dict(track=None), dict(len=None),
             dict(frames=None), dict(track_offsets=None), dict(track_root=None), dict(obs=None), dict(summary=None),
             dict(obs=out[2].ptr + 4), dict(obs=out[2].ptr + 8), dict(max_records=0), dict(max_records=-3),
             dict(min_len=0), dict(max_tracks=0), dict(max_obs=0), dict(consistent_only=2), dict(consistent_only=-1),
             dict(offsets=None, stride=-1), dict(record_obs=d_lab[0].ptr), dict(record_obs=d_lab[1].ptr),
             dict(record_obs=d_lab[2].ptr)]
    for kw in cases:
        assert call(**kw) == MISIFT_EINVAL, kw
    ctx.sync()
    sizes = (9, 8, 64, 16, 8)
    for buf, n in zip(out, sizes):
        assert (ctx.download(buf, (n,), np.uint32) == POISON).all()
    assert call() == MISIFT_OK                                  # the same arguments, unbroken
    ctx.sync()
    assert list(ctx.download(out[4], (8,), np.int32)) == [3, 6, 3, 6, 2, 0, 0, 0]
    assert list(ctx.download(out[0], (9,), np.uint32)) == [0, 2, 4, 6] + [POISON] * 5


def test_no_frames(ctx):
    """nframes == 0 is no error: only the summary and track_offsets[0] are written."""
    z = np.zeros(4, np.int32)
    b = Batch(ctx, fabricated_records(4, 10), [], None, 5, 4, (z, z, z))
    off, root, obs, rob, s = b.check(2, 1, max_tracks=3, max_obs=5, what="no frames")
    assert list(off.view(np.uint32)) == [0, POISON, POISON, POISON] and list(s) == [0] * 8


# ---- launches

def test_fixed_launch_count(ctx):
    """The number of tracks_export_* launches is the one include/misift.h states, whatever the data: an empty batch of
    frames with count 0, the planted case, the giant-track case."""
    z = np.zeros(8, np.int32)
    empty = Batch(ctx, fabricated_records(8, 11), [0, 0, 0], None, 2, 8, (z, z, z))
    n = 4096
    track = np.zeros(n + 1, np.int32)
    tlen = np.zeros(n + 1, np.int32)
    tlen[0] = n + 1
    tfr = np.zeros(n + 1, np.int32)
    tfr[0] = 2
    giant = Batch(ctx, fabricated_records(n + 1, 12), [n, 1], np.array([0, n, n + 1], np.int32), 0, n + 1,
                  (track, tlen, tfr))
    for b, cons, written in ((empty, 1, 0), (planted_batch(ctx, False), 1, None), (giant, 0, 1)):
        ctx.sync()
        ctx.profile_reset()
        ctx.profile_enable(True)
        try:
            got = b.check(2, cons, what="launch count")
            prof = ctx.profile_read()
        finally:
            ctx.profile_enable(False)
        ours = {k: v["calls"] for k, v in prof.items() if k.startswith("tracks_export_")}
        assert len(ours) == LAUNCHES and all(c == 1 for c in ours.values()), ours
        assert written is None or got[4][2] == written


# ---- the whole chain

def test_chain_with_no_host_read(ctx):
    """extract (packed, async) -> quantize -> mutual int8 pairs (window 3) -> find -> improve -> link -> export
    (min_len 3, consistent only), no host read in between (test_gpu_tracks.test_chain_with_no_host_read with the export
    appended).  After one sync everything is downloaded: the export equals the restatement on the downloaded labels and
    records, and every observation carries the position bits of the packed record it names."""
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
    out, oc, _ = ctx.match_pairs_batch_i8(pairs, packed, dq, B, cnt.ptr, cnt.ptr + 4 * B, 0, max_pts=mp, mutual=True)
    sel = list(range(npairs))
    gates = (0.85, 0.95, 3.0)
    dH, _ = ctx.find_homography_batch(sel, [300 + i for i in sel], out, npairs, oc, None, mp, max_pts=mp,
                                      num_loops=1000, min_score=gates[0], max_ambiguity=gates[1], thresh=5.0)
    ctx.improve_homography_batch(sel, out, npairs, oc, dH, None, mp, num_loops=5, min_score=gates[0],
                                 max_ambiguity=gates[1], thresh=3.0)
    max_records = mp * B
    lab = [_poisoned(ctx, max_records) for _ in range(3)] + [_poisoned(ctx, 8)]
    ctx.link_tracks_batch(pairs, out, oc, mp, B, cnt.ptr, cnt.ptr + 4 * B, 0, max_records=max_records,
                          min_score=gates[0], max_ambiguity=gates[1], max_error=gates[2], track=lab[0],
                          track_len=lab[1], track_frames=lab[2], summary=lab[3])
    max_tracks, max_obs = max_records // 3 + 1, max_records
    exp_out = [_poisoned(ctx, max_tracks + 1), _poisoned(ctx, max_tracks), _poisoned(ctx, 4 * max_obs),
               _poisoned(ctx, max_records), _poisoned(ctx, 8)]
    ctx.export_tracks_batch(packed, B, cnt.ptr, cnt.ptr + 4 * B, 0, max_records=max_records, track=lab[0],
                            track_len=lab[1], track_frames=lab[2], min_len=3, consistent_only=1, max_tracks=max_tracks,
                            max_obs=max_obs, track_offsets=exp_out[0], track_root=exp_out[1], obs=exp_out[2],
                            record_obs=exp_out[3], summary=exp_out[4])
    ctx.sync()
    ci = ctx.download(cnt, (2 * B + 1,), np.int32)
    fc, offs = ci[:B], ci[B:]
    recs = ctx.download(packed, (max_records,), capi.POINT_DTYPE)
    labels = [ctx.download(a, (max_records,), np.int32) for a in lab[:3]]
    shapes = ((max_tracks + 1,), np.int32), ((max_tracks,), np.int32), ((max_obs,), capi.TRACK_OBS_DTYPE), \
        ((max_records,), np.int32), ((8,), np.int32)
    got = [ctx.download(a, *s) for a, s in zip(exp_out, shapes)]
    assert (fc > 100).all(), fc
    exp = expected_export(xy_bits(recs), fc, offs, 0, max_records, *labels, 3, 1, max_tracks, max_obs, POISON)
    for g, e, name in zip(got, exp, NAMES):
        assert g.tobytes() == e.tobytes(), name
    T, O = int(got[4][2]), int(got[4][3])
    assert T > 50 and got[4][0] == T and O >= 3 * T, got[4]
    obs = got[2][:O]
    named = recs[offs[obs["frame"]] + obs["record"]]
    for k in ("xpos", "ypos"):
        assert np.array_equal(np.ascontiguousarray(obs[k]).view(np.uint32), np.ascontiguousarray(named[k]).view(np.uint32))


# ---- guard mode, robustness

def test_guard_mode():
    """One planted call with every allocation guarded (the library's temp memory and the outputs): no band damaged."""
    from cudasift_amd import capi
    recs, offs, total, labels = guard_case()
    with guarded_context(6) as g:
        Batch(g, recs, GUARD_SIZES, offs, 0, total, labels).check(2, 0, what="guard")
    capi.check_guards()


def test_labels_of_random_ints_stay_inside_the_capacities():
    """Label arrays no linker wrote: any int32 in every slot, a third of the records claiming to be roots with lengths
    anywhere up to max_records (so the sums wrap), labels that point at roots, at non-roots and outside the index
    space.  The contents are unspecified; the call returns MISIFT_OK, the sync succeeds and no guard band of the outputs
    (exactly the capacities given) or of the library's temp memory is damaged: the range checks hold."""
    sizes = [700, 0, 2500, 900]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    total = int(offs[-1])
    rng = np.random.default_rng(13)
    any32 = lambda: rng.integers(-2 ** 31, 2 ** 31, total).astype(np.int32)       # noqa: E731
    g_idx = np.arange(total, dtype=np.int32)
    kind = rng.integers(0, 3, total)
    track = np.where(kind == 0, g_idx, np.where(kind == 1, rng.integers(0, total, total).astype(np.int32), any32()))
    kind = rng.integers(0, 3, total)
    tlen = np.where(kind == 0, rng.integers(1, 50, total), np.where(kind == 1, rng.integers(1, total + 1, total), any32()))
    with guarded_context(6) as g:
        b = Batch(g, fabricated_records(total, 14), sizes, offs, 0, total, (track, tlen.astype(np.int32), any32()))
        for max_tracks, max_obs in ((total, total), (40, 300)):
            b.run(1, 0, max_tracks, max_obs)                     # run() checks the return code and syncs

"""misift_export_tracks_batch without a GPU: the numpy restatement expected_export (what tests/test_gpu_tracks_export.py
holds the device to, byte for byte) pinned to a plain Python dictionary version on random and hand-built label arrays,
and the library's symbol, binding and NULL-context check.  The label arrays come from test_tracks_cpu.expected_tracks,
the restatement of the call that writes them on the device."""
import numpy as np
import pytest

from test_tracks_cpu import _case, blank_rows, expected_tracks, frame_spans, set_edge

POISON = 0x5A5A5A5A
NAMES = ("track_offsets", "track_root", "obs", "record_obs", "summary")


# ---- the expected answer, restated in numpy

def expected_export(recs_xy, counts, offsets, stride, max_records, track, tlen, tframes, min_len, consistent_only,
                    max_tracks, max_obs, poison):
    """(track_offsets, track_root, obs, record_obs, summary) as misift_export_tracks_batch defines them; the slots the
    call never writes hold `poison`.  recs_xy[g] = the (xpos, ypos) bit patterns of the record with global index g, as
    uint32.  obs is a capi.TRACK_OBS_DTYPE array built from 32-bit words, so NaN payloads survive."""
    from cudasift_amd import capi
    spans = frame_spans(counts, offsets, stride, max_records)
    valid = np.zeros(max_records, bool)
    frame_of = np.zeros(max_records, np.int64)
    local_of = np.zeros(max_records, np.int64)
    for f, (b, n, ok) in enumerate(spans):
        if ok and n:
            valid[b:b + n] = True
            frame_of[b:b + n] = f
            local_of[b:b + n] = np.arange(n)
    track = np.asarray(track[:max_records]).astype(np.int64)
    tlen = np.asarray(tlen[:max_records]).astype(np.int64)
    tframes = np.asarray(tframes[:max_records]).astype(np.int64)
    sel = valid & (track == np.arange(max_records)) & (tlen >= min_len)
    if consistent_only:
        sel &= tlen == tframes
    roots = np.nonzero(sel)[0]                                   # ascending: the numbering
    lens = tlen[roots]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    written = (np.arange(len(roots)) < max_tracks) & (off[1:] <= max_obs)
    T = int(written.sum())
    assert written[:T].all()                                     # off is increasing: a prefix
    O = int(off[T])
    number = np.full(max_records, -1, np.int64)
    number[roots[:T]] = np.arange(T)
    g = np.nonzero(valid)[0]
    m = g[number[track[g]] >= 0]
    m = m[np.argsort(track[m], kind="stable")]                   # by root, then by global index
    assert len(m) == O
    p32 = np.uint32(poison)
    track_offsets = np.full(max_tracks + 1, p32, np.uint32)
    track_root = np.full(max_tracks, p32, np.uint32)
    words = np.full((max_obs, 4), p32, np.uint32)
    record_obs = np.full(max_records, p32, np.uint32)
    track_offsets[:T + 1] = off[:T + 1]
    track_root[:T] = roots[:T]
    words[:O, 0] = frame_of[m]
    words[:O, 1] = local_of[m]
    words[:O, 2:] = np.asarray(recs_xy, np.uint32)[m]
    record_obs[g] = np.uint32(0xFFFFFFFF)                        # -1
    record_obs[m] = np.arange(O)
    summary = np.array([len(roots), lens.sum(), T, O, lens[:T].max() if T else 0,
                        sum(1 for _, _, ok in spans if not ok), 0, 0], np.int32)
    return (track_offsets.view(np.int32), track_root.view(np.int32), words.view(capi.TRACK_OBS_DTYPE).reshape(max_obs),
            record_obs.view(np.int32), summary)


# ---- the reference the restatement is pinned to: the same definition, one record at a time

def export_by_dict(recs_xy, counts, offsets, stride, max_records, track, tlen, tframes, min_len, consistent_only,
                   max_tracks, max_obs, poison):
    from cudasift_amd import capi
    where = {}                                                   # g -> (frame, record)
    dropped = 0
    for f, c in enumerate(counts):
        n = max(int(c), 0)
        b = int(offsets[f]) if offsets is not None else f * int(stride)
        if n and not (b >= 0 and b + n <= max_records):
            dropped += 1
            continue
        for r in range(n):
            where[b + r] = (f, r)
    members = {}
    for g in sorted(where):
        members.setdefault(int(track[g]), []).append(g)
    selected = []
    for g in sorted(where):
        if int(track[g]) != g or int(tlen[g]) < min_len:
            continue
        if consistent_only and int(tlen[g]) != int(tframes[g]):
            continue
        selected.append(g)
    p32 = np.uint32(poison)
    track_offsets = np.full(max_tracks + 1, p32, np.uint32)
    track_root = np.full(max_tracks, p32, np.uint32)
    words = np.full((max_obs, 4), p32, np.uint32)
    record_obs = np.full(max_records, p32, np.uint32)
    for g in where:
        record_obs[g] = 0xFFFFFFFF
    track_offsets[0] = 0
    off, T, longest, cut = 0, 0, 0, False
    for t, root in enumerate(selected):
        n = int(tlen[root])
        assert n == len(members[root])
        if not cut and t < max_tracks and off + n <= max_obs:
            track_root[t] = root
            track_offsets[t + 1] = off + n
            for k, g in enumerate(sorted(members[root])):
                words[off + k] = (where[g][0], where[g][1], recs_xy[g][0], recs_xy[g][1])
                record_obs[g] = off + k
            T, longest = t + 1, max(longest, n)
            off += n
        else:
            cut = True                                           # off only grows: nothing behind a cut track fits
    summary = np.array([len(selected), sum(int(tlen[g]) for g in selected), T, off, longest, dropped, 0, 0], np.int32)
    return (track_offsets.view(np.int32), track_root.view(np.int32), words.view(capi.TRACK_OBS_DTYPE).reshape(max_obs),
            record_obs.view(np.int32), summary)


def _same(args):
    a, b = expected_export(*args, POISON), export_by_dict(*args, POISON)
    for x, y, what in zip(a, b, NAMES):
        assert x.tobytes() == y.tobytes(), (what, x[:16], y[:16])
    return a


def random_xy(n, seed):
    """(n, 2) random bit patterns, NaN payloads and infinities among them."""
    return np.random.default_rng(seed).integers(0, 2 ** 32, (max(n, 1), 2), dtype=np.uint64).astype(np.uint32)


def _labels(case):
    """The layout arguments and the three label arrays of a test_tracks_cpu case, as expected_export takes them."""
    counts, offs, stride, max_records = case[4:8]
    track, tlen, tframes, _ = expected_tracks(*case, (0.85, 0.95, float("inf")), poison=POISON)
    return (random_xy(max_records, max_records), counts, offs, stride, max_records, track, tlen, tframes)


# ---- tests

def test_library_exports_the_call():
    """Fails without the feature: the symbol, its row in capi.SIGNATURES, the binding, the observation's dtype and the
    NULL-context check."""
    from cudasift_amd import capi
    assert "misift_export_tracks_batch" in capi.SIGNATURES
    assert hasattr(capi.Context, "export_tracks_batch")
    assert capi.TRACK_OBS_DTYPE.itemsize == 16
    assert capi.TRACK_OBS_DTYPE.names == ("frame", "record", "xpos", "ypos")
    L = capi.lib()
    assert hasattr(L, "misift_export_tracks_batch")
    rc = L.misift_export_tracks_batch(None, None, 2, None, None, 16, 32, None, None, None, 2, 1, 8, 32, None, None, None,
                                      None, None)
    assert rc == -1                                             # MISIFT_EINVAL


def _random_case(seed):
    """A test_tracks_cpu case of random rows over 3..7 frames of -1..8 records, packed or padded by the seed's parity."""
    rng = np.random.default_rng(100 + seed)
    nf = int(rng.integers(3, 8))
    counts = [int(c) for c in rng.integers(-1, 9, nf)]
    counts[-1] = max(counts[-1], 2)                              # the last frame holds records (it may be dropped)
    npairs = int(rng.integers(4, 16))
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, nf, (npairs, 2))]
    max_pts = 8
    n = npairs * max_pts
    rows = blank_rows(npairs, max_pts, seed)
    rows["score"] = rng.random(n, dtype=np.float32) * np.float32(1.5)
    rows["ambiguity"] = rng.random(n, dtype=np.float32) * np.float32(0.9)
    rows["match"] = rng.integers(-1, 9, n)
    return _case(pairs, rows, max_pts, counts, padded=bool(seed & 1))


FILTERS = [(m, c) for m in (1, 2, 3) for c in (0, 1)]


@pytest.mark.parametrize("seed", range(12))
def test_random_labels(seed):
    """Labels from expected_tracks on random rows (as test_tracks_cpu.test_random_graphs builds them): both layouts,
    frames of count 0 and -1, every (min_len, consistent_only), capacities that cut at a track boundary, inside a track
    (it is dropped whole) and not at all, by max_obs and by max_tracks; every fourth seed a max_records that drops the
    last frame."""
    case = _random_case(seed)
    counts = case[4]
    if seed % 4 == 3:
        b, n_last, _ = frame_spans(counts, case[5], case[6], case[7])[-1]
        case = case[:7] + (b + n_last - 1,)                      # one short of the last frame's end
    lab = _labels(case)
    for min_len, cons in FILTERS:
        whole = _same(lab + (min_len, cons, lab[4] + 2, lab[4] + 3))
        s = whole[4]
        assert s[0] == s[2] and s[1] == s[3] and s[5] == (seed % 4 == 3)
        off, T = whole[0], int(s[2])
        if T == 0:
            continue
        j = T // 2
        end_j = int(off[j + 1])
        cuts = [(T + 2, end_j, j + 1),                           # at a track boundary
                (max(j, 1), lab[4], max(j, 1)),                  # by max_tracks
                (T, int(off[T]), T)]                             # exactly enough
        if end_j > 1:
            cuts.append((T + 2, end_j - 1, j))                   # inside track j (its last slot missing): dropped whole
        for max_tracks, max_obs, want in cuts:
            got = _same(lab + (min_len, cons, max_tracks, max_obs))
            assert got[4][2] == want, (min_len, cons, max_tracks, max_obs, got[4])
            assert got[4][0] == s[0] and got[4][1] == s[1]


def test_random_labels_cover_the_filters():
    """The random cases are worth their name: over the twelve seeds there are selected tracks at every filter, and
    consistent_only drops some."""
    seen = {f: 0 for f in FILTERS}
    for seed in range(12):
        lab = _labels(_random_case(seed))
        for f in FILTERS:
            seen[f] += int(expected_export(*lab, f[0], f[1], lab[4], lab[4], POISON)[4][0])
    assert all(v > 0 for v in seen.values()), seen
    assert seen[(2, 1)] < seen[(2, 0)] and seen[(3, 1)] < seen[(3, 0)], seen


def test_chain_through_eight_frames():
    pairs = [(f, f + 1) for f in range(7)]
    rows = blank_rows(7, 4, 1)
    for i in range(7):
        set_edge(rows, 4, i, 2, 2)
    lab = _labels(_case(pairs, rows, 4, [4] * 8))
    xy = lab[0]
    off, root, obs, rob, s = _same(lab + (2, 1, 4, 40))
    assert list(off.view(np.uint32)) == [0, 8, POISON, POISON, POISON]
    assert list(root.view(np.uint32)) == [2, POISON, POISON, POISON]
    assert list(obs["frame"][:8]) == list(range(8)) and list(obs["record"][:8]) == [2] * 8
    w = obs.view(np.uint32).reshape(40, 4)
    assert (w[:8, 2:] == xy[2:32:4]).all() and (w[8:] == POISON).all()
    assert list(rob) == [k // 4 if k % 4 == 2 else -1 for k in range(32)]
    assert list(s) == [1, 8, 1, 8, 8, 0, 0, 0]


def test_two_rows_one_column():
    """Exported with consistent_only = 0 in index order, absent with 1."""
    rows = blank_rows(1, 4, 3)
    set_edge(rows, 4, 0, 0, 1)
    set_edge(rows, 4, 0, 3, 1)
    lab = _labels(_case([(0, 1)], rows, 4, [4, 2]))
    off, root, obs, rob, s = _same(lab + (2, 0, 3, 6))
    assert list(off.view(np.uint32)) == [0, 3, POISON, POISON] and root[0] == 0
    assert [(int(o["frame"]), int(o["record"])) for o in obs[:3]] == [(0, 0), (0, 3), (1, 1)]
    assert list(rob) == [0, -1, -1, 1, -1, 2] and list(s) == [1, 3, 1, 3, 3, 0, 0, 0]
    off, root, obs, rob, s = _same(lab + (2, 1, 3, 6))
    assert list(off.view(np.uint32)) == [0, POISON, POISON, POISON] and (root.view(np.uint32) == POISON).all()
    assert (obs.view(np.uint32) == POISON).all() and list(rob) == [-1] * 6 and list(s) == [0] * 8


def test_singletons_at_min_len_one():
    rows = blank_rows(0, 4, 12)
    lab = _labels(_case([], rows, 4, [2, 0, -1, 3], padded=True))         # stride 6
    off, root, obs, rob, s = _same(lab + (1, 1, 8, 8))
    assert list(off.view(np.uint32)) == [0, 1, 2, 3, 4, 5, POISON, POISON, POISON]
    assert list(root.view(np.uint32)) == [0, 1, 18, 19, 20, POISON, POISON, POISON]
    assert [(int(o["frame"]), int(o["record"])) for o in obs[:5]] == [(0, 0), (0, 1), (3, 0), (3, 1), (3, 2)]
    exp = np.full(24, POISON, np.uint32)
    exp[[0, 1, 18, 19, 20]] = np.arange(5)
    assert list(rob.view(np.uint32)) == list(exp) and list(s) == [5, 5, 5, 5, 1, 0, 0, 0]
    _, _, _, rob, s = _same(lab + (2, 0, 8, 8))
    assert list(s) == [0] * 8 and list(rob[[0, 1, 18, 19, 20]]) == [-1] * 5


def test_capacity_drops_a_track_whole():
    """Three tracks of 2: max_obs 5 writes two of them and not half of the third; max_tracks 1 writes one."""
    rows = blank_rows(1, 4, 5)
    for r in range(3):
        set_edge(rows, 4, 0, r, r)
    lab = _labels(_case([(0, 1)], rows, 4, [4, 4]))
    off, root, obs, rob, s = _same(lab + (2, 1, 4, 5))
    assert list(off.view(np.uint32)) == [0, 2, 4, POISON, POISON] and list(root[:2]) == [0, 1]
    assert list(s) == [3, 6, 2, 4, 2, 0, 0, 0] and list(rob) == [0, 2, -1, -1, 1, 3, -1, -1]
    assert (obs.view(np.uint32).reshape(5, 4)[4] == POISON).all()
    _, _, _, rob, s = _same(lab + (2, 1, 1, 5))
    assert list(s) == [3, 6, 1, 2, 2, 0, 0, 0] and list(rob) == [0, -1, -1, -1, 1, -1, -1, -1]


def test_no_frames():
    """nframes == 0: only the summary and track_offsets[0] are written."""
    z = np.zeros(4, np.int32)
    off, root, obs, rob, s = _same((random_xy(4, 0), [], None, 5, 4, z, z, z, 2, 1, 3, 5))
    assert list(off.view(np.uint32)) == [0, POISON, POISON, POISON] and list(s) == [0] * 8
    for a in (root, obs, rob):
        assert (a.view(np.uint32) == POISON).all()

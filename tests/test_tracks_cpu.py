"""misift_link_tracks_batch without a GPU: the numpy restatement expected_tracks (what tests/test_gpu_tracks.py holds the
device to, byte for byte) pinned to a plain Python dictionary union-find on random and hand-built graphs, the gate rule
at and around equality, match values outside the second frame, and the library's symbol and NULL-context check."""
import numpy as np
import pytest

INF = float("inf")
GATES = (0.85, 0.95, INF)                                        # min_score, max_ambiguity, max_error


# ---- the expected answer, restated in numpy

def frame_spans(counts, offsets, stride, max_records):
    """Per frame (base, n, takes part): n = max(count, 0); a frame holding records that do not all lie in
    [0, max_records) takes no part.  An empty frame always does (it has nothing to place)."""
    out = []
    for f, c in enumerate(counts):
        n = max(int(c), 0)
        b = int(offsets[f]) if offsets is not None else f * int(stride)
        out.append((b, n, n == 0 or (b >= 0 and b + n <= max_records)))
    return out


def accepted_edges(pairs, rows, row_counts, max_pts, spans, gates):
    """(u, v): the global indices of every accepted row, in row order."""
    min_score, max_amb, max_err = (np.float32(g) for g in gates)
    us, vs = [], []
    for i, (f1, f2) in enumerate(pairs):
        (b1, n1, ok1), (b2, n2, ok2) = spans[f1], spans[f2]
        k = min(int(row_counts[i]), n1, max_pts)
        if k <= 0 or not (ok1 and ok2):
            continue
        sel = rows[i * max_pts:i * max_pts + k]
        m = sel["match"]
        with np.errstate(invalid="ignore"):
            ok = (m >= 0) & (m < n2) & (sel["score"] > min_score) & (sel["ambiguity"] < max_amb)
            if np.isfinite(max_err):
                ok &= sel["match_error"] < max_err
        r = np.nonzero(ok)[0]
        us.append(b1 + r)
        vs.append(b2 + m[r].astype(np.int64))
    if not us:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(us).astype(np.int64), np.concatenate(vs).astype(np.int64)


def expected_tracks(pairs, rows, row_counts, max_pts, counts, offsets, stride, max_records, gates, poison=0):
    """(track, track_len, track_frames, summary) as misift_link_tracks_batch defines them; the slots the call never
    writes hold `poison`.  Components by minimum-label propagation with pointer jumping."""
    spans = frame_spans(counts, offsets, stride, max_records)
    u, v = accepted_edges(pairs, rows, row_counts, max_pts, spans, gates)
    valid = np.zeros(max_records, bool)
    frame_of = np.zeros(max_records, np.int64)
    for f, (b, n, ok) in enumerate(spans):
        if ok and n:
            valid[b:b + n] = True
            frame_of[b:b + n] = f
    lab = np.arange(max_records, dtype=np.int64)
    while len(u):
        m = np.minimum(lab[u], lab[v])
        new = lab.copy()
        for idx in (u, v, lab[u], lab[v]):
            np.minimum.at(new, idx, m)
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, lab):
            break
        lab = new
    g = np.nonzero(valid)[0]
    track = np.full(max_records, poison, np.int64)
    tlen = np.full(max_records, poison, np.int64)
    tframes = np.full(max_records, poison, np.int64)
    track[g] = lab[g]
    tlen[g] = 0
    tframes[g] = 0
    roots, n_rec = np.unique(lab[g], return_counts=True)
    tlen[roots] = n_rec
    nframes = max(len(counts), 1)
    keys = np.unique(lab[g] * nframes + frame_of[g])
    r2, n_fr = np.unique(keys // nframes, return_counts=True)
    tframes[r2] = n_fr
    long_ = n_rec >= 2
    summary = np.zeros(8, np.int64)
    summary[0] = len(u)
    summary[1] = int(long_.sum())
    summary[2] = int(n_rec[long_].sum())
    summary[3] = int((tlen[roots[long_]] != tframes[roots[long_]]).sum())
    summary[4] = int(n_rec.max()) if len(n_rec) else 0
    summary[5] = sum(1 for _, _, ok in spans if not ok)
    to32 = lambda a: (a & 0xFFFFFFFF).astype(np.uint32).view(np.int32)       # noqa: E731  (poison may be a bit pattern)
    return to32(track), to32(tlen), to32(tframes), summary.astype(np.int32)


# ---- fabricated rows

def window_pairs(frames, window):
    """(f, f + 1) ... (f, f + window) over the listed frames, in list order."""
    return [(frames[a], frames[b]) for a in range(len(frames)) for b in range(a + 1, min(a + window, len(frames) - 1) + 1)]


def blank_rows(npairs, max_pts, seed):
    """npairs * max_pts rows no gate accepts: random scores below any threshold used here, random in-range-looking
    matches, and match_error (like every byte the matchers never write) 0xFF poison."""
    from cudasift_amd import capi
    rows = np.frombuffer(b"\xff" * (576 * npairs * max_pts), capi.POINT_DTYPE).copy()
    rng = np.random.default_rng(seed)
    n = npairs * max_pts
    rows["score"] = rng.random(n, dtype=np.float32) * np.float32(0.5)
    rows["ambiguity"] = rng.random(n, dtype=np.float32)
    rows["match"] = rng.integers(-1, 50, n)
    return rows


def set_edge(rows, max_pts, i, r, m, score=0.97, ambiguity=0.3):
    o = rows[i * max_pts + r:i * max_pts + r + 1]
    o["score"], o["ambiguity"], o["match"] = score, ambiguity, m


def plant(rows, max_pts, pairs, members, drop, rng):
    """members: per track {frame: record}.  Every pair (f1, f2) both of whose frames a track visits gets the row
    members[f1] -> members[f2], unless dropped with probability `drop`."""
    for i, (f1, f2) in enumerate(pairs):
        for t in members:
            if f1 in t and f2 in t and f1 != f2 and rng.random() >= drop:
                set_edge(rows, max_pts, i, t[f1], t[f2])


# ---- the reference the restatement is pinned to: a dictionary union-find over the same definition, one row at a time

def tracks_by_dict(pairs, rows, row_counts, max_pts, counts, offsets, stride, max_records, gates, poison=0):
    min_score, max_amb, max_err = (np.float32(g) for g in gates)
    base, cnt, ok = {}, {}, {}
    for f, c in enumerate(counts):
        cnt[f] = max(int(c), 0)
        base[f] = int(offsets[f]) if offsets is not None else f * int(stride)
        ok[f] = cnt[f] == 0 or (base[f] >= 0 and base[f] + cnt[f] <= max_records)
    parent, frame = {}, {}
    for f in cnt:
        if ok[f]:
            for r in range(cnt[f]):
                parent[base[f] + r] = base[f] + r
                frame[base[f] + r] = f

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    edges = 0
    for i, (f1, f2) in enumerate(pairs):
        if not (ok[f1] and ok[f2]):
            continue
        for r in range(max(min(int(row_counts[i]), cnt[f1], max_pts), 0)):
            o = rows[i * max_pts + r]
            m = int(o["match"])
            if not (0 <= m < cnt[f2]):
                continue
            if not (o["score"] > min_score and o["ambiguity"] < max_amb):
                continue
            if np.isfinite(max_err) and not o["match_error"] < max_err:
                continue
            edges += 1
            a, b = find(base[f1] + r), find(base[f2] + m)
            if a != b:
                parent[max(a, b)] = min(a, b)
    track = np.full(max_records, poison, np.int64)
    tlen, tframes = track.copy(), track.copy()
    comp = {}
    for g in parent:
        comp.setdefault(find(g), []).append(g)
        track[g], tlen[g], tframes[g] = find(g), 0, 0
    summary = np.zeros(8, np.int64)
    summary[0] = edges
    for root, mem in comp.items():
        assert root == min(mem)
        tlen[root] = len(mem)
        tframes[root] = len({frame[g] for g in mem})
        summary[4] = max(summary[4], len(mem))
        if len(mem) >= 2:
            summary[1] += 1
            summary[2] += len(mem)
            summary[3] += tlen[root] != tframes[root]
    summary[5] = sum(1 for f in ok if not ok[f])
    to32 = lambda a: (a & 0xFFFFFFFF).astype(np.uint32).view(np.int32)       # noqa: E731
    return to32(track), to32(tlen), to32(tframes), summary.astype(np.int32)


def _same(case, gates=GATES, poison=0x5A5A5A5A):
    a = expected_tracks(*case, gates, poison=poison)
    b = tracks_by_dict(*case, gates, poison=poison)
    for x, y, what in zip(a, b, ("track", "len", "frames", "summary")):
        assert np.array_equal(x, y), (what, np.nonzero(x != y)[0][:8], x[:16], y[:16])
    return a


def _packed(sizes):
    return np.concatenate([[0], np.cumsum(np.maximum(sizes, 0))]).astype(np.int32)


def _case(pairs, rows, max_pts, counts, *, padded=False, row_counts=None, max_records=None):
    """The argument tuple of expected_tracks up to the gates, packed or padded to stride max(counts) + 3."""
    counts = list(counts)
    if row_counts is None:
        row_counts = [min(max(counts[f1], 0), max_pts) for f1, _ in pairs]
    if padded:
        stride = max(max(counts), 0) + 3
        offs, total = None, stride * len(counts)
    else:
        offs, stride = _packed(counts), 0
        total = int(offs[-1])
    return (pairs, rows, np.asarray(row_counts, np.int32), max_pts, counts, offs, stride,
            max_records if max_records is not None else max(total, 1))


# ---- tests

def test_library_exports_the_call():
    """Fails without the feature: the symbol, its row in capi.SIGNATURES, the binding, and the NULL-context check."""
    from cudasift_amd import capi
    assert "misift_link_tracks_batch" in capi.SIGNATURES
    assert hasattr(capi.Context, "link_tracks_batch")
    L = capi.lib()
    assert hasattr(L, "misift_link_tracks_batch")
    pairs = np.zeros(2, np.int32)
    rc = L.misift_link_tracks_batch(None, 1, pairs.ctypes.data, None, None, 16, 2, None, None, 16, 32, 0.85, 0.95, INF,
                                    None, None, None, None)
    assert rc == -1                                             # MISIFT_EINVAL


@pytest.mark.parametrize("seed", range(12))
def test_random_graphs(seed):
    """Rows random in every field: random edges, some gated away, matches out of range, frames of count 0 and -1, self
    pairs, repeated pairs; both layouts."""
    rng = np.random.default_rng(seed)
    nf = int(rng.integers(2, 7))
    counts = [int(c) for c in rng.integers(-1, 9, nf)]
    npairs = int(rng.integers(0, 10))
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, nf, (npairs, 2))]
    max_pts = 6
    n = npairs * max_pts
    rows = blank_rows(npairs, max_pts, seed)
    rows["score"] = rng.random(n, dtype=np.float32) * np.float32(1.5)
    rows["match"] = rng.integers(-2, 10, n)
    rc = [int(rng.choice([-1, min(max(counts[a], 0), max_pts), max_pts + 2])) for a, _ in pairs]
    case = _case(pairs, rows, max_pts, counts, padded=bool(seed & 1), row_counts=rc)
    _same(case)
    rows["match_error"] = rng.random(n, dtype=np.float32) * np.float32(4)
    _same(case, gates=(0.85, 0.95, 2.0))


def test_chain_through_eight_frames():
    pairs = [(f, f + 1) for f in range(7)]
    rows = blank_rows(7, 4, 1)
    for i in range(7):
        set_edge(rows, 4, i, 2, 2)
    track, tlen, tfr, s = _same(_case(pairs, rows, 4, [4] * 8))
    assert list(track[2::4]) == [2] * 8 and tlen[2] == 8 and tfr[2] == 8
    assert list(s) == [7, 1, 8, 0, 8, 0, 0, 0]


def test_cycle():
    pairs = [(0, 1), (1, 2), (2, 0)]
    rows = blank_rows(3, 3, 2)
    set_edge(rows, 3, 0, 1, 0)
    set_edge(rows, 3, 1, 0, 2)
    set_edge(rows, 3, 2, 2, 1)
    track, tlen, tfr, s = _same(_case(pairs, rows, 3, [3, 3, 3]))
    assert track[1] == track[3] == track[8] == 1 and tlen[1] == 3 and tfr[1] == 3
    assert list(s) == [3, 1, 3, 0, 3, 0, 0, 0]


def test_two_rows_one_column_is_inconsistent():
    rows = blank_rows(1, 4, 3)
    set_edge(rows, 4, 0, 0, 1)
    set_edge(rows, 4, 0, 3, 1)
    track, tlen, tfr, s = _same(_case([(0, 1)], rows, 4, [4, 2]))
    assert tlen[0] == 3 and tfr[0] == 2 and track[3] == 0 and track[5] == 0
    assert list(s) == [2, 1, 3, 1, 3, 0, 0, 0]


def test_late_edge_merges_two_long_tracks():
    pairs = [(f, f + 1) for f in range(9)] + [(2, 7)]
    rows = blank_rows(len(pairs), 2, 4)
    for i in range(9):
        if i != 4:                                              # 0..4 and 5..9 stay apart ...
            set_edge(rows, 2, i, 1, 1)
    _, tlen, _, s = _same(_case(pairs, rows, 2, [2] * 10))
    assert s[1] == 2 and tlen[1] == 5 and tlen[11] == 5
    set_edge(rows, 2, 9, 1, 1)                                  # ... until the last pair's row joins them
    track, tlen, tfr, s = _same(_case(pairs, rows, 2, [2] * 10))
    assert (track[1::2] == 1).all() and tlen[1] == 10 and tfr[1] == 10 and tlen[11] == 0
    assert list(s) == [9, 1, 10, 0, 10, 0, 0, 0]


def test_duplicate_edges_count_twice():
    pairs = [(0, 1), (0, 1), (1, 0)]
    rows = blank_rows(3, 2, 5)
    set_edge(rows, 2, 0, 0, 1)
    set_edge(rows, 2, 1, 0, 1)
    set_edge(rows, 2, 2, 1, 0)                                  # the same edge seen from the other side
    _, tlen, tfr, s = _same(_case(pairs, rows, 2, [2, 2]))
    assert tlen[0] == 2 and tfr[0] == 2
    assert list(s) == [3, 1, 2, 0, 2, 0, 0, 0]


def test_self_pairs():
    rows = blank_rows(1, 3, 6)
    set_edge(rows, 3, 0, 0, 0)                                  # a self edge: counted, a no-op
    set_edge(rows, 3, 0, 1, 2)                                  # two records of one frame: inconsistent
    track, tlen, tfr, s = _same(_case([(0, 0)], rows, 3, [3]))
    assert list(track) == [0, 1, 1] and list(tlen) == [1, 2, 0] and list(tfr) == [1, 1, 0]
    assert list(s) == [2, 1, 2, 1, 2, 0, 0, 0]


def gate_rows():
    """One pair of 16 x 16, rows 0..12 each its own boundary case against GATES / max_error 2; returns (rows, the rows
    that are edges with max_error = inf, the rows that are edges with max_error = 2)."""
    f32, nan = np.float32, np.float32("nan")
    up, dn = (lambda x: np.nextafter(f32(x), f32(9))), (lambda x: np.nextafter(f32(x), f32(-9)))
    rows = blank_rows(1, 16, 7)
    spec = [  # score, ambiguity, match_error
        (f32(0.85), 0.3, 1.0), (up(0.85), 0.3, 1.0), (dn(0.85), 0.3, 1.0),
        (0.97, f32(0.95), 1.0), (0.97, dn(0.95), 1.0), (0.97, up(0.95), 1.0),
        (nan, 0.3, 1.0), (0.97, nan, 1.0), (0.97, 0.3, nan),
        (0.97, 0.3, f32(2.0)), (0.97, 0.3, dn(2.0)), (0.97, 0.3, up(2.0)), (f32(INF), -f32(INF), 0.0),
    ]
    for r, (sc, am, er) in enumerate(spec):
        set_edge(rows, 16, 0, r, r, sc, am)
        rows["match_error"][r] = er
    return rows, [1, 4, 8, 9, 10, 11, 12], [1, 4, 10, 12]


def test_gates_at_and_around_equality():
    rows, open_, tight = gate_rows()
    for gates, want in ((GATES, open_), ((0.85, 0.95, 2.0), tight)):
        track, tlen, _, s = _same(_case([(0, 1)], rows, 16, [16, 16]), gates=gates)
        assert sorted(np.nonzero(tlen[:16] == 2)[0]) == want, (gates, np.nonzero(tlen[:16] == 2)[0])
        assert s[0] == len(want) and all(track[16 + r] == r for r in want)


def test_infinite_max_error_never_reads_match_error():
    rows = blank_rows(1, 4, 8)
    set_edge(rows, 4, 0, 1, 3)
    assert np.isnan(rows["match_error"]).all()                   # 0xFF poison
    _, tlen, _, s = _same(_case([(0, 1)], rows, 4, [4, 4]))
    assert tlen[1] == 2 and s[0] == 1
    _, tlen, _, s = _same(_case([(0, 1)], rows, 4, [4, 4]), gates=(0.85, 0.95, 1e30))
    assert tlen[1] == 1 and s[0] == 0                           # finite: NaN < x is false


def test_match_outside_the_second_frame():
    rows = blank_rows(2, 8, 9)
    for r, m in enumerate([-1, -7, 5, 6, 4, 2 ** 31 - 1, -2 ** 31]):     # n2 = 5: only m = 4 is an edge
        set_edge(rows, 8, 0, r, m)
    set_edge(rows, 8, 1, 0, 0)                                  # frame 2 has count -1: no record 0
    track, tlen, _, s = _same(_case([(0, 1), (0, 2)], rows, 8, [8, 5, -1]))
    assert s[0] == 1 and tlen[4] == 2 and track[8 + 4] == 4


def test_rows_beyond_the_counts_are_ignored():
    rows = blank_rows(3, 4, 10)
    for i in range(3):
        for r in range(4):
            set_edge(rows, 4, i, r, 0)
    # pair 0: 2 rows by the row count; pair 1: frame 1 has 3 records; pair 2: row count -1
    case = _case([(0, 1), (1, 0), (0, 1)], rows, 4, [4, 3], row_counts=[2, 4, -1])
    _, tlen, _, s = _same(case)
    assert s[0] == 5 and tlen[0] == 5


def test_frames_outside_max_records_take_no_part():
    rows = blank_rows(2, 3, 11)
    set_edge(rows, 3, 0, 0, 0)
    set_edge(rows, 3, 1, 1, 2)                                  # touches frame 2, which is cut off
    poison = 0x5A5A5A5A
    track, tlen, _, s = _same(_case([(0, 1), (1, 2)], rows, 3, [3, 3, 3], max_records=8), poison=poison)
    assert list(s) == [1, 1, 2, 0, 2, 1, 0, 0]
    assert (track[6:].view(np.uint32) == poison).all() and track[3] == 0 and tlen[4] == 1


def test_no_pairs_gives_singletons():
    rows = blank_rows(0, 4, 12)
    track, tlen, tfr, s = _same(_case([], rows, 4, [2, 0, 3], padded=True))
    stride = 6
    for f, n in enumerate([2, 0, 3]):
        for r in range(stride):
            g = f * stride + r
            assert (track[g], tlen[g], tfr[g]) == ((g, 1, 1) if r < n else (0x5A5A5A5A,) * 3)
    assert list(s) == [0, 0, 0, 0, 1, 0, 0, 0]

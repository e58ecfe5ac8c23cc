"""The premises of detect_cases.py, proved on the oracle and on the candidate model (no GPU): every case reaches the path
it names, with the counts stated, and the model's candidate set contains everything the oracle detects — the scan's in-row
test really is a necessary condition."""
import numpy as np
import pytest

import detect_cases as dc

F = np.float32
RUNS = dict(dc.all_runs())
WITH_DETECTIONS = [n for n, c in RUNS.items() if c["detections"]]


def levels_of(name):
    c = RUNS[name]
    w, h, noct = c["geom"]
    for f, frame in enumerate(c["frames"]):
        for k, level in enumerate(frame):
            yield c, f, k, level, dc.planes_of(level, noct, k + 1)


def test_geometry_of_the_cases():
    assert dc.GEOM_R[0] % 4 != 0 and dc.GEOM_Q[0] % 4 == 0
    for g in (dc.GEOM_R, dc.GEOM_Q):
        assert (g[0] + dc.STRIP - 1) // dc.STRIP == 3                              # three strips on the finest level
        assert all((w + dc.STRIP - 1) // dc.STRIP <= 2 for w, _ in dc.level_sizes(*g)[:-1])
    # the four-octave case: coarsest level 8 x 8, one pixel less in either direction is a tiny call (misift_tiny_call)
    w, h, noct = dc.GEOM_T
    tiny = lambda w, h: w < 16 or h < 16 or (w >> (noct - 1)) < 8 or (h >> (noct - 1)) < 8
    assert dc.level_sizes(w, h, noct)[0] == (8, 8) and not tiny(w, h) and tiny(63, h) and tiny(w, 63)
    for name, c in RUNS.items():
        sizes = dc.level_sizes(*c["geom"])
        assert len(c["frames"]) in (1, 2, dc.SMALL_FRAMES + 1), name
        for frame in c["frames"]:
            assert [a.shape for a in frame] == [(h, w) for w, h in sizes] and all(a.dtype == F for a in frame), name
    for name in ("lattice_r5", "lattice_q5", "subpixel"):
        fr = RUNS[name]["frames"]
        assert len(fr) == dc.SMALL_FRAMES + 1
        assert all((a == a[0, 0]).all() for a in fr[1])                            # a flat frame between two busy ones
        busy = [f for i, f in enumerate(fr) if i != 1]
        assert all(not np.array_equal(a[-1], b[-1]) for i, a in enumerate(busy) for b in busy[i + 1:])   # different content per frame


@pytest.mark.parametrize("name", WITH_DETECTIONS)
def test_restated_refinement_counts_what_the_oracle_detects(name):
    """refine_np is only used to count paths; it earns that by finding the oracle's detections, one for one."""
    for (c, f, k, level, planes), e in zip(levels_of(name), [e for row in dc.expected(name) for e in row]):
        sub = F(2 ** (c["geom"][2] - k - 1))
        r = dc.refine_np(planes, c["thresh"], F(c["lowest_scale"]) / sub)
        kept = r["kept"]
        assert int(kept.sum()) == e["n"], (name, f, k)
        a = np.sort(np.stack([r["xpos"][kept], r["ypos"][kept]], 1).astype(np.float64), axis=0)
        b = np.sort(np.stack([e["pts"]["xpos"], e["pts"]["ypos"]], 1).astype(np.float64), axis=0)
        assert np.allclose(a, b, rtol=0, atol=1e-3), (name, f, k)


@pytest.mark.parametrize("name", list(RUNS))
def test_model_contains_every_extremum_of_the_oracle(name):
    """Necessity of the in-row test: every 26-neighbour extremum of planes 1..5 — hence every position and scale index the
    oracle detects at — is among the model's candidates; and the model never names a border pixel."""
    c = RUNS[name]
    for (c, f, k, level, planes), e in zip(levels_of(name), [e for row in dc.expected(name) for e in row]):
        r = dc.refine_np(planes, c["thresh"], 0.0)
        ext = r["x"].astype(np.uint32) | (r["y"].astype(np.uint32) << 14) | (r["s"].astype(np.uint32) << 28)
        assert np.isin(ext, e["codes"]).all(), (name, f, k)
        assert len(ext) >= e["n"]
        if c["detections"] and e["n"]:                     # the oracle's own records: each sits on a modelled candidate
            xy = set(zip(*dc.decode(e["codes"])[:2]))
            kept = np.flatnonzero(r["kept"])
            for p in e["pts"]:
                j = kept[np.argmin(np.abs(r["xpos"][kept] - p["xpos"]) + np.abs(r["ypos"][kept] - p["ypos"]))]
                assert abs(r["xpos"][j] - p["xpos"]) < 1e-3 and abs(r["ypos"][j] - p["ypos"]) < 1e-3
                assert (int(r["x"][j]), int(r["y"][j])) in xy
        x, y, s = dc.decode(e["codes"])
        h, w = level.shape
        assert ((x >= 1) & (x <= w - 2) & (y >= 1) & (y <= h - 2) & (s <= 4)).all()
        assert len(e["codes"]) < dc.cand_cap(w, h) or name == "overflow"


@pytest.mark.parametrize("name", ["lattice_r1", "lattice_r5", "lattice_q1", "lattice_q5"])
def test_lattice_covers_every_row_and_column_of_the_finest_level(name):
    c = RUNS[name]
    w, h, noct = c["geom"]
    for f, row in enumerate(dc.expected(name)):
        e = row[-1]
        if len(c["frames"]) > 1 and f == 1:
            assert all(r["n"] == 0 and len(r["codes"]) == 0 for r in row)          # the flat frame: nothing at all
            continue
        xs, ys = np.rint(e["pts"]["xpos"]).astype(int), np.rint(e["pts"]["ypos"]).astype(int)
        assert set(range(2, w - 2)) <= set(xs), (name, f, sorted(set(range(2, w - 2)) - set(xs)))
        assert set(range(2, h - 2)) <= set(ys), (name, f, sorted(set(range(2, h - 2)) - set(ys)))
        # hence: both columns at the strip seams, all four positions of a quad, both rows at any segment seam
        for seam in (dc.STRIP, 2 * dc.STRIP):
            assert {seam - 1, seam} <= set(xs)
        assert {0, 1, 2, 3} <= set(xs % 4)
        # blobs were planted on rows 1 and h-2 and columns 1 and w-2; the expectation there is the oracle's, which never
        # reports row or column 0 or the last one
        x, y, _ = dc.decode(e["codes"])
        assert x.min() >= 1 and y.min() >= 1 and x.max() <= w - 2 and y.max() <= h - 2
        assert (np.floor(e["pts"]["xpos"] + 0.5) >= 1).all()
        assert {1, h - 2} <= set(y) and {1, w - 2} <= set(x)                       # the model does see candidates there
        # ... and blobs centred ON the outermost rows and columns, whose DoG peaks where nothing may be reported
        P = np.abs(dc.planes_of(c["frames"][f][-1], noct, noct)[1:6])
        for edge in (P[:, 0, 8:w - 8], P[:, h - 1, 8:w - 8], P[:, 8:h - 8, 0], P[:, 8:h - 8, w - 1]):
            assert edge.max() > c["thresh"]
    # the coarser levels (one or two strips) have a detection on every row too: both sides of any segment seam
    for f, row in enumerate(dc.expected(name)):
        for k, (lw, lh) in enumerate(dc.level_sizes(w, h, noct)[:-1]):
            if not (len(c["frames"]) > 1 and f == 1):
                assert set(range(2, lh - 2)) <= set(np.rint(row[k]["pts"]["ypos"]).astype(int)), (name, f, k)


def test_ties_are_exact_in_every_plane_and_yield_no_keypoint():
    c = RUNS["ties"]
    seen = 0
    for (c, f, k, level, planes), e in zip(levels_of("ties"), dc.expected("ties")[0]):
        h, w = level.shape
        assert e["n"] == 0, k                                                      # no keypoint anywhere on a tie level
        for cx, cy in dc.tie_spots(w, h):
            px = dc.tie_pixels(cx, cy)
            assert len(px) in (2, 4)
            for s in range(7):
                v = [planes[s, y, x] for x, y in px]
                assert all(a.tobytes() == v[0].tobytes() for a in v), (k, cx, cy, s)
            assert max(abs(planes[s, px[0][1], px[0][0]]) for s in range(1, 6)) > c["thresh"]   # and they would be extrema
            got = set(zip(*dc.decode(e["codes"])[:2]))
            if cx != int(cx):
                assert not got & set(px)                       # a tie within the row: not strictly above, the scan drops it
            else:
                assert set(px) <= got                          # a tie between rows passes the in-row test: refine must drop it
            seen += len(px)
    kinds = {len(dc.tie_pixels(cx, cy)) for cx, cy in dc.tie_spots(*dc.GEOM_Q[:2])}
    assert kinds == {2, 4} and seen >= 30
    assert any(int(cx) % dc.STRIP == dc.STRIP - 1 for cx, _ in dc.tie_spots(*dc.GEOM_Q[:2]))      # one astride a strip seam


def test_broken_ties_yield_exactly_one_keypoint_each():
    c = RUNS["ties_ulp"]
    total = 0
    for (c, f, k, level, planes), e in zip(levels_of("ties_ulp"), dc.expected("ties_ulp")[0]):
        h, w = level.shape
        spots = dc.tie_spots(w, h)
        assert len(c["ulps"][k]) == len(spots)
        for (cx, cy), u in zip(spots, c["ulps"][k]):
            assert 1 <= u <= 256
            assert dc.spot_detections(e["pts"], cx, cy) == 1, (k, cx, cy)
        assert e["n"] == len(spots)
        total += len(spots)
        # half the raise is not enough (the raise is the smallest power of two that shows in the planes)
        if spots:
            half = dc.tie_level(w, h, [u // 2 for u in c["ulps"][k]], dc.TIE_SIGMA[k])
            pts, n = dc.oracle_detections(half, c["geom"][2], k + 1, c["thresh"], 0.0)
            for (cx, cy), u in zip(spots, c["ulps"][k]):
                assert dc.spot_detections(pts[:n], cx, cy) != 1 or u == 1
    assert total >= 10 and min(min(u) for u in c["ulps"] if u) == 1


def test_threshold_and_scale_floor_at_the_ulp():
    runs = {n: (c, at, present) for n, c, at, present in dc.ulp_cases()}
    base = RUNS["lattice_r1"]
    w, h, noct = base["geom"]
    planes = dc.planes_of(base["frames"][0][-1], noct, noct)
    for name, (c, (x, y, s), present) in runs.items():
        r = dc.refine_np(planes, c["thresh"], c["lowest_scale"])
        j = np.flatnonzero((r["x"] == x) & (r["y"] == y) & (r["s"] == s))
        e = dc.expected(name)[0][-1]
        if present:
            assert len(j) == 1 and r["kept"][j[0]], name
            assert (np.abs(e["pts"]["xpos"] - r["xpos"][j[0]]) + np.abs(e["pts"]["ypos"] - r["ypos"][j[0]])).min() < 1e-3
        else:
            assert len(j) == 0 or not r["kept"][j[0]], name
            assert ((np.abs(e["pts"]["xpos"] - x) > 0.75) | (np.abs(e["pts"]["ypos"] - y) > 0.75)).all(), name
    teq, tb = runs["thresh_eq"][0]["thresh"], runs["thresh_below"][0]["thresh"]
    x, y, s = runs["thresh_eq"][1]
    assert F(teq) == abs(planes[s + 1, y, x]) and F(tb) == np.nextafter(F(teq), F(0))
    assert dc.expected("thresh_below")[0][-1]["n"] > dc.expected("thresh_eq")[0][-1]["n"]
    feq, fa = runs["floor_eq"][0]["lowest_scale"], runs["floor_above"][0]["lowest_scale"]
    assert F(fa) == np.nextafter(F(feq), F(np.inf))
    assert (dc.expected("floor_eq")[0][-1]["pts"]["scale"] == F(feq)).any()
    assert dc.expected("floor_eq")[0][-1]["n"] > dc.expected("floor_above")[0][-1]["n"] > 0


def test_edge_sweep_lands_on_both_sides_of_the_limit():
    passed = failed = 0
    for c, f, k, level, planes in levels_of("edge"):
        r = dc.refine_np(planes, c["thresh"], 0.0)
        passed += int(r["edge_ok"].sum())
        failed += int((~r["edge_ok"]).sum())
    assert passed >= 10 and failed >= 10, (passed, failed)


def test_subpixel_case_takes_the_fallback_and_the_solve():
    fb = direct = 0
    for c, f, k, level, planes in levels_of("subpixel"):
        r = dc.refine_np(planes, c["thresh"], 0.0)
        fb += int((r["kept"] & r["fallback"]).sum())
        direct += int((r["kept"] & ~r["fallback"]).sum())
    assert fb >= 5 and direct >= 20, (fb, direct)


def test_queue_case_reaches_direct_append_and_flush_below_capacity():
    c = RUNS["queue"]
    w, h, noct = c["geom"]
    level = c["frames"][0][-1]
    sr = dc.strip_row_counts(dc.model_mask(dc.planes_of(level, noct, noct), c["thresh"]))
    assert (sr > dc.CQ_CAP).sum() >= 10                                            # direct append: one row of a strip over 64
    small = (sr > 0) & (sr <= dc.CQ_CAP)
    pair = small[:, :-1] & small[:, 1:] & (sr[:, :-1] + sr[:, 1:] < dc.CQ_CAP)
    run = np.zeros_like(sr)
    for y in range(1, sr.shape[1]):                                                # rows that each fit and together do not
        run[:, y] = np.where(small[:, y], run[:, y - 1] + sr[:, y], 0)
    assert pair.any() and (run > dc.CQ_CAP).any()
    for k, (lw, lh) in enumerate(dc.level_sizes(w, h, noct)):
        assert len(dc.expected("queue")[0][k]["codes"]) < dc.cand_cap(lw, lh)
    assert dc.expected("queue")[0][-1]["n"] < c["max_pts"]
    # ... and the overflow case exceeds the finest octave's list, and only that one
    e = dc.expected("overflow")[0]
    sizes = dc.level_sizes(*RUNS["overflow"]["geom"])
    assert len(e[-1]["codes"]) > dc.cand_cap(*sizes[-1])
    assert all(len(e[k]["codes"]) < dc.cand_cap(*sizes[k]) for k in range(len(sizes) - 1))


def test_nonfinite_pixels_leave_every_blob_its_keypoint():
    c = RUNS["nonfinite"]
    w, h, noct = c["geom"]
    level, blobs = dc.nonfinite_level(w, h)
    assert np.array_equal(level, c["frames"][0][-1], equal_nan=True)
    assert int(np.isnan(level).sum()) == 9 and int(np.isinf(level).sum()) == 1
    planes = dc.planes_of(c["frames"][0][-1], noct, noct)
    assert np.isnan(planes).any()
    e = dc.expected("nonfinite")[0][-1]
    for cx, cy, _, _, _ in blobs:
        assert all(max(abs(cx - px), abs(cy - py)) >= 20 for px, py in dc.NONFINITE_AT.values())
        assert dc.spot_detections(e["pts"], cx, cy) >= 1, (cx, cy)
    assert np.isfinite(np.stack([e["pts"][f] for f in ("xpos", "ypos", "scale", "sharpness", "edgeness")])).all()
    # the oracle's minima and maxima skip NaN neighbours (fminf / fmaxf), and so does the model: candidates next to the hole
    x, y, _ = dc.decode(e["codes"])
    assert len(x) >= e["n"]

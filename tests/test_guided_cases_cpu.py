"""The hostile scenes of guided_cases.py without a GPU.

- The disc walk of misift_match_guided_batch through the host-only hook misift_test_guided_gather, which is compiled
  from the function the kernel calls: its gate equals the numpy float32 restatement byte for byte on every scene, and
  every record that passes lies in a cell the row walks.  The epipolar hooks get the same check on the same scenes.
- The disc walk is selective: cells are at least r' wide, so [p - r', p + r'] meets at most 3 of them per axis and a row
  walks at most 9 cells, on a saturated 64 x 64 grid and on a grid whose cells are exactly r' wide.
- The premises of the scenes, on the restatement (what test_gpu_guided_hostile.py compares the device with), so that
  the GPU tests cannot pass vacuously.  They are conditions, not measurements: a scene that misses one is changed."""
import numpy as np
import pytest

import guided_cases as gc
from epipolar_util import f32

SCENES = [(k, n) for k in gc.KINDS for n in gc.NAMES]


def _guided_hook(H, xy1, xy2, radius):
    """(pass, visited, (gx, gy)) from misift_test_guided_gather."""
    from cudasift_amd import capi
    H = np.ascontiguousarray(H, f32).reshape(9)
    xy1 = np.ascontiguousarray(xy1, f32).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, f32).reshape(-1, 2)
    n1, n2 = len(xy1), len(xy2)
    ps = np.full((n1, n2), 7, np.uint8)
    vis = np.full((n1, n2), 7, np.uint8)
    g = np.zeros(2, np.int32)
    assert capi.lib().misift_test_guided_gather(H.ctypes.data, xy1.ctypes.data, n1, xy2.ctypes.data, n2, radius,
                                                ps.ctypes.data, vis.ctypes.data, g.ctypes.data) == 0
    assert ((ps | vis) <= 1).all()
    return ps.astype(bool), vis.astype(bool), (int(g[0]), int(g[1]))


def _frames_of(s, i):
    f1, f2 = s.pairs[i]
    return s.fr1[f1], s.fr2[f2]


# ---- the gather

@pytest.mark.parametrize("kind,name", SCENES)
def test_gather_on_every_scene(kind, name):
    """The hook's gate is the restatement's, and no candidate lies outside the cells its row walks."""
    s = gc.scene(kind, name)
    passed = 0
    for i in range(len(s.pairs)):
        a, b = _frames_of(s, i)
        xy1, xy2 = gc.xy(a), gc.xy(b)
        exp = gc.gate(kind, s.mats[i], xy1, xy2, s.radius)
        if kind == "guided":
            ps, vis, g = _guided_hook(s.mats[i], xy1, xy2, s.radius)
        else:
            from test_epipolar_cpu import _hooks
            ps, vis, g = _hooks(s.mats[i], xy1, xy2, s.radius)
        assert np.array_equal(ps, exp), (name, i, "gate differs from numpy in", int((ps != exp).sum()))
        missed = ps & ~vis
        assert not missed.any(), (name, i, "candidates in unvisited cells", np.argwhere(missed)[:4].tolist(), g)
        assert not vis[:, ~np.isfinite(xy2).all(1)].any(), (name, i, "a non-finite record in a cell")
        assert 1 <= g[0] <= 64 and 1 <= g[1] <= 64
        passed += int(ps.sum())
    assert passed > 0, name


def _cell_centres(w, h, gx, gy):
    """One record at the centre of every cell of a gx x gy grid over [0, w] x [0, h], then the box's corners."""
    cx, cy = (np.arange(gx) + 0.5) * (w / gx), (np.arange(gy) + 0.5) * (h / gy)
    p = np.stack(np.meshgrid(cx, cy), 2).reshape(-1, 2)
    return np.concatenate([p, [[0, 0], [w, 0], [0, h], [w, h]]]).astype(f32)


@pytest.mark.parametrize("what", ["saturated", "exact"])
def test_disc_walk_is_selective(what):
    r = 2.0
    rp = r * (1.0 + 1.0 / 1024) + 1e-20
    if what == "saturated":                                        # 1920 x 1080: cells 30 x 16.9, far wider than r'
        w, h, gx, gy = 1920.0, 1080.0, 64, 64
    else:                                                          # cells exactly r' wide: 40 r' is exact in float32
        w, h, gx, gy = 40 * rp, 24 * rp, 40, 24
        assert float(f32(w)) == w and float(f32(h)) == h
    xy2 = _cell_centres(w, h, gx, gy)
    rng = np.random.default_rng(5)
    xy1 = np.stack([rng.uniform(-0.1 * w, 1.1 * w, 600), rng.uniform(-0.1 * h, 1.1 * h, 600)], 1).astype(f32)
    on_edges = np.stack([np.arange(40) * (w / gx), np.arange(40) % gy * (h / gy)], 1).astype(f32)    # on cell borders
    xy1 = np.concatenate([xy1, on_edges])
    ps, vis, g = _guided_hook(np.eye(3, dtype=f32), xy1, xy2, r)
    if what == "saturated":
        assert g == (gx, gy), g
    else:                                                          # fl(40 r' / r') + 1, whichever way the quotient rounds
        assert g[0] in (gx, gx + 1) and g[1] in (gy, gy + 1), g
    assert not (ps & ~vis).any()
    cells = vis[:, :gx * gy].sum(1)                                # one record per cell: the cells a row walks
    assert cells.max() <= 9, cells.max()
    inside = (xy1[:, 0] >= 0) & (xy1[:, 0] <= w) & (xy1[:, 1] >= 0) & (xy1[:, 1] <= h)
    assert (cells[inside] >= 1).all()
    assert inside.sum() > 300
    if what == "exact":                                            # 2 r' across cells r' wide: three per axis is usual
        assert (cells == 9).any()


# ---- the premises

@pytest.mark.parametrize("kind,name", SCENES)
def test_scene_shapes(kind, name):
    s = gc.scene(kind, name)
    if name not in gc.WITNESS and name != "greedy":
        assert tuple(s.counts1) == gc.ROWS, s.counts1
    if name not in gc.WITNESS:
        assert max(s.counts2) == 2100 and sorted(s.counts2)[-2] <= 300, s.counts2
    assert len({f1 for f1, _ in s.pairs}) == len(s.pairs)


@pytest.mark.parametrize("kind,name", SCENES)
def test_every_scene_matches_some_rows_and_not_others(kind, name):
    s, r1, o1, r2, o2, ef, enf = gc.expected(kind, name)
    rows = np.concatenate([ef[f1]["match"] for f1, _ in s.pairs])
    assert (rows >= 0).sum() >= 20 and (rows < 0).sum() >= 20, (name, int((rows >= 0).sum()), int((rows < 0).sum()))
    assert np.array_equal(enf, [(ef[f1]["match"] >= 0).sum() for f1, _ in s.pairs])
    print(kind, name, "matched", int((rows >= 0).sum()), "unmatched", int((rows < 0).sum()), "num_found", enf.tolist())


@pytest.mark.parametrize("kind", gc.KINDS)
def test_ties_occur(kind):
    """Every tenth planted partner has a copy: rows whose runner-up is the best score itself."""
    for name in ("offset", "degenerate", "leaving"):
        s, _, _, _, _, ef, _ = gc.expected(kind, name)
        e = np.concatenate(ef)
        tie = (e["match"] >= 0) & (e["ambiguity"] == e["score"] / (e["score"] + f32(1e-6)))
        assert tie.sum() >= 3, (name, int(tie.sum()))


@pytest.mark.parametrize("kind", gc.KINDS)
def test_greedy_row(kind):
    s = gc.scene(kind, "greedy")
    a, b = _frames_of(s, 0)
    g = gc.gate(kind, s.mats[0], gc.xy(a), gc.xy(b), s.radius)
    n = g.sum(1)
    assert n[gc.GREEDY_ROW] >= gc.GREEDY_N, n[gc.GREEDY_ROW]
    others = np.delete(n, gc.GREEDY_ROW)
    assert others.max() <= 3 and set(others.tolist()) == {0, 1, 2, 3}, np.bincount(others)
    # GREEDY_BEST of the row's candidates share its best score: the smallest index wins a 200-way tie
    _, _, _, _, _, ef, _ = gc.expected(kind, "greedy")
    row = ef[s.pairs[0][0]][gc.GREEDY_ROW]
    same = np.nonzero((b["data"] == a["data"][gc.GREEDY_ROW]).all(1) & g[gc.GREEDY_ROW])[0]
    assert len(same) == gc.GREEDY_BEST and row["match"] == same.min()
    assert row["ambiguity"] == row["score"] / (row["score"] + f32(1e-6))
    print(kind, "greedy row", int(n[gc.GREEDY_ROW]), "others", np.bincount(others).tolist())


@pytest.mark.parametrize("family,pair", [("gate", 0), ("matrix", 2)])
@pytest.mark.parametrize("kind", gc.KINDS)
@pytest.mark.parametrize("name", sorted(gc.WITNESS))
def test_contraction_witnesses(kind, name, family, pair):
    """At least 64 witnesses per fused form, and on every one the fused gate changes `match`: the witness record is the
    strict best of its row over the whole frame, and the two gates disagree on it."""
    from batch_util import orc
    ext, radius = gc.WITNESS[name]
    M, p1, p2, form, found = gc.witnesses(kind, ext, radius, family)
    if family == "gate":
        assert form.count("x") >= 64 and form.count("y") >= 64, found
    else:
        assert form.count("xy") >= 128, found
    s, _, _, _, _, ef, _ = gc.expected(kind, name)
    a, b = _frames_of(s, pair)
    assert np.array_equal(gc.xy(a), p1) and np.array_equal(gc.xy(b), p2) and np.array_equal(s.mats[pair], M)
    full = a.copy()
    orc().match(full, len(a), b.copy(), len(b), full=True, exact=True)
    assert np.array_equal(full["match"], np.arange(len(a)))        # record i is row i's best of all
    assert (full["ambiguity"] < 1).all()                           # and strictly so
    d = gc.gate(kind, M, p1, p2, radius).diagonal()
    assert np.array_equal(d, gc.gate_diag(kind, M, p1, p2, radius))
    for fused in ("x", "y"):
        kw = {"fused": fused} if family == "gate" else {"fused_m": fused}
        rows = np.nonzero([fused in f for f in form])[0]
        other = gc.gate_diag(kind, M, p1, p2, radius, **kw)
        assert (d[rows] != other[rows]).all(), fused
    assert all(f in ("x", "y", "xy") for f in form)
    got = ef[s.pairs[pair][0]]["match"]
    assert np.array_equal(got == np.arange(len(a)), d)             # the restatement's match is the witness iff it passes
    assert 10 <= d.sum() <= len(a) - 10                            # flips both ways
    print(kind, name, family, "found", found, "used", len(form), "pass the contract's gate", int(d.sum()))


@pytest.mark.parametrize("kind", gc.KINDS)
def test_nonfinite_scene(kind):
    s = gc.scene(kind, "nonfinite")
    fin2 = [np.isfinite(gc.xy(p)).all(1) for p in s.fr2]
    assert sorted(int(f.sum()) for f in fin2)[:2] == [0, 1]
    straddled = 0
    for i in range(len(s.pairs)):
        a, b = _frames_of(s, i)
        fin = np.isfinite(gc.xy(b)).all(1)
        if len(b) > 1:
            assert not fin[0] and not fin[-1]
        g = gc.gate(kind, s.mats[i], gc.xy(a), gc.xy(b), s.radius)
        assert not g[:, ~fin].any() and not g[~np.isfinite(gc.xy(a)).all(1)].any()
        for row in g:                                              # candidates before and after a non-finite record
            c = np.nonzero(row)[0]
            if len(c) >= 2 and (~fin[c[0]:c[-1]]).any():
                straddled += 1
    assert straddled >= 20, straddled
    assert sum(int((~np.isfinite(gc.xy(p)).all(1)).sum()) for p in s.fr1) >= 20
    print(kind, "rows whose candidates straddle a non-finite record", straddled)


@pytest.mark.parametrize("kind", gc.KINDS)
def test_degenerate_scene(kind):
    """All records at one point form one cell: every record is a candidate of a row within reach, none of one outside."""
    s = gc.scene(kind, "degenerate")
    seen = 0
    for i in range(len(s.pairs)):
        a, b = _frames_of(s, i)
        p = gc.xy(b)
        if (p == p[0]).all():
            n = gc.gate(kind, s.mats[i], gc.xy(a), p, s.radius).sum(1)
            assert set(n.tolist()) == {0, len(b)}, np.bincount(n)
            seen += 1
        else:
            assert (p[:, 0] == p[0, 0]).all() or (p[:, 1] == p[0, 1]).all()
    assert seen == 2


@pytest.mark.parametrize("kind", gc.KINDS)
def test_outlier_scene(kind):
    """radius = +inf: every finite row has the same candidates, and the record at 3e38 is not among a guided row's."""
    s = gc.scene(kind, "outlier_inf")
    for i in range(len(s.pairs)):
        a, b = _frames_of(s, i)
        g = gc.gate(kind, s.mats[i], gc.xy(a), gc.xy(b), s.radius)
        live = g.any(1)
        assert (g[live] == g[live][0]).all() and g[live][0].sum() >= len(b) - 2
        assert np.array_equal(live, np.isfinite(gc.xy(a)).all(1))
        if kind == "guided":
            assert not g[:, 17].any() and b["xpos"][17] == f32(3e38)


@pytest.mark.parametrize("kind", gc.KINDS)
def test_radius_scenes(kind):
    s = gc.scene(kind, "radius_small")
    a, b = _frames_of(s, 0)
    assert f32(s.radius) * f32(s.radius) > 0 and np.abs(gc.xy(b)).min() >= 1e5
    s = gc.scene(kind, "radius_huge")
    r2 = f32(s.radius) * f32(s.radius)
    assert np.isfinite(r2)
    if kind == "epipolar":                                         # both factors finite, the product +inf
        from epipolar_util import lines_np
        a, _ = _frames_of(s, 0)
        n2 = lines_np(s.mats[0], a["xpos"], a["ypos"])[3]
        with np.errstate(over="ignore"):
            assert (np.isfinite(n2) & np.isinf(r2 * n2)).sum() >= 64


@pytest.mark.parametrize("kind", gc.KINDS)
def test_leaving_scene(kind):
    s = gc.scene(kind, "leaving")
    _, _, _, _, _, ef, enf = gc.expected(kind, "leaving")
    if kind == "epipolar":
        assert (enf[:3] == np.array(s.counts1[:3])).all() and (enf[3:] == 0).all(), enf
        return
    assert enf[0] >= 60 and enf[1] == 0 and enf[2] == 0 and enf[3] >= 8 and enf[4] == 0, enf
    a, b = _frames_of(s, 0)
    H = s.mats[0].astype(np.float64)
    q = H @ np.stack([a["xpos"], a["ypos"], np.ones(len(a))]).astype(np.float64)
    px, py = q[0] / q[2], q[1] / q[2]
    outside = (px < 0) | (px > 500) | (py < 0) | (py > 500)
    assert (outside & (ef[0]["match"] >= 0)).sum() >= 60           # matched although the projection is off the box
    a, _ = _frames_of(s, 3)
    den = s.mats[3][2, 0] * a["xpos"] + s.mats[3][2, 1] * a["ypos"] + s.mats[3][2, 2]
    assert (den == 0).sum() >= 10 and (den < 0).sum() >= 20 and (den > 0).sum() >= 10
    assert ((den < 0) & (ef[3]["match"] >= 0)).sum() >= 4 and (ef[3]["match"][den == 0] == -1).all()


# ---- the hook's arguments

def test_guided_hook_rejects_bad_arguments():
    from cudasift_amd import capi
    L = capi.lib()
    H = np.eye(3, dtype=f32).reshape(9)
    p = np.zeros(2, f32)
    out = np.zeros(1, np.uint8)
    g = np.zeros(2, np.int32)

    def call(h=H.ctypes.data, a=p.ctypes.data, n1=1, b=p.ctypes.data, n2=1, r=1.0, ps=out.ctypes.data,
             vis=out.ctypes.data, grid=g.ctypes.data):
        return L.misift_test_guided_gather(h, a, n1, b, n2, r, ps, vis, grid)
    assert call() == 0
    assert call(h=None) == -1
    assert call(n1=-1) == -1 and call(n2=-1) == -1
    assert call(a=None) == -1 and call(b=None) == -1
    assert call(ps=None) == -1 and call(vis=None) == -1
    assert call(grid=None) == -1
    assert call(r=0.0) == -1 and call(r=-1.0) == -1 and call(r=float("nan")) == -1
    assert call(a=None, n1=0, ps=None, vis=None) == 0              # nothing to write
    assert call(r=float("inf")) == 0 and tuple(g) == (1, 1)

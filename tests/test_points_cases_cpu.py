"""The planted-detection cases (points_cases.py) reach what they claim — conditions on the generator, checked without a GPU:
every class is populated, the kernels' path predicates (restated in numpy float32) have members on both sides, the oracle
meets its own special cases on them, and the hand-written expectation is the oracle's ExtractSift."""
import numpy as np
import pytest

import points_cases as pc
from points_cases import F

M = 4096


def labelled(c, label, k=None):
    """(level index, w, h, records) of the case's records with that label."""
    out = []
    for i, ((w, h), d, l) in enumerate(zip(pc.level_sizes(*c["geom"]), c["dets"], c["labels"])):
        if k is None or k == i:
            sel = d[l == label]
            if len(sel):
                out.append((i, w, h, sel))
    return out


def test_levels_have_the_library_s_sizes_and_every_content_kind_is_used():
    from cudasift_amd import capi
    for geom in (pc.GEOM_A, pc.GEOM_B):
        lay = capi.pyramid_layout(*geom)                       # finest first
        assert [(w, h) for _, w, h, _ in lay][::-1] == pc.level_sizes(*geom)
    sizes = pc.level_sizes(*pc.GEOM_B)
    assert sizes[0] == (12, 7) and sizes[1] == (24, 15) and sizes[2] == (48, 30)       # under 13 / under 40 in one or both axes
    assert all(s % 2 == 1 for s in pc.GEOM_A[:2])
    used = set()
    for n in pc.CASE_NAMES:
        c = pc.case(n)
        used |= set(c["kinds"])
        for lv, (w, h) in zip(c["levels"], pc.level_sizes(*c["geom"])):
            assert lv.shape == (h, w) and lv.dtype == np.float32 and lv.min() >= 0.0 and lv.max() <= 255.0
    assert set(pc.CONTENT_KINDS) <= used, set(pc.CONTENT_KINDS) - used
    assert np.ptp(pc.content("flat", 20, 10)) == 0.0
    imp = pc.content("impulse", 21, 11)
    assert (imp != imp[0, 0]).sum() == 1


def test_every_class_is_populated_and_sizes_stay_small():
    seen = {}
    for n in pc.CASE_NAMES:
        c = pc.case(n)
        assert c["geom"][0] <= 200 and c["geom"][1] <= 150 and pc.total(c) <= 2000
        for d, l in zip(c["dets"], c["labels"]):
            assert d.shape == (len(l), 5) and d.dtype == np.float32 and np.isfinite(d).all() and (d[:, 2] > 0).all()
            for lab in l:
                seen[lab] = seen.get(lab, 0) + 1
    for lab in ("interior", "border", "inside", "window", "cinterior", "binade_x", "binade_y", "binade_xy", "reach_edge",
                "reach_over", "reach_big", "reach_tiny", "flat", "impulse_near", "dups", "small"):
        assert seen.get(lab, 0) >= 6, (lab, seen)
    # nothing further out than the guard's far side
    for n in pc.CASE_NAMES:
        c = pc.case(n)
        for (w, h), d in zip(pc.level_sizes(*c["geom"]), c["dets"]):
            assert (d[:, 0] >= -64.5).all() and (d[:, 0] <= w + 64.5).all()
            assert (d[:, 1] >= -64.5).all() and (d[:, 1] <= h + 64.5).all()


def test_octave_counts_cover_the_launch_edges():
    counts = {n: [len(d) for d in pc.case(n)["dets"]] for n in pc.CASE_NAMES}
    flat = [v for c in counts.values() for v in c]
    for want in (1, 63, 64, 65, 257):
        assert want in flat, (want, counts)
    assert counts["counts"][1] == 0 and counts["counts"][0] > 0 and counts["counts"][2] > 0     # an empty octave between two others
    assert None in pc.MULTI and len(pc.MULTI) == 5
    assert pc.total(pc.empty_case()) == 0
    assert len({tuple(c["geom"]) for c in pc.multi_frames()}) == 1
    assert sum(pc.total(c) for c in pc.multi_frames()) > 500


def test_identity_keys_are_unique():
    from util import point_keys
    for n in pc.CASE_NAMES:
        c = pc.case(n)
        sharp = np.concatenate([d[:, 3] for d in c["dets"]])
        assert len(np.unique(sharp.view(np.uint32))) == len(sharp), n
        pts, num, cnt, _ = pc.expected(c, M)
        firsts = np.concatenate([np.arange(int(cnt[2 * o - 1]), int(cnt[2 * o])) for o in range(1, c["geom"][2] + 1)])
        keys = point_keys(pts[firsts])
        assert len(set(keys)) == len(keys) == pc.total(c), n


def test_border_class_sits_on_every_edge_corner_and_side_of_the_guard():
    c = pc.case("border")
    for k, w, h, d in labelled(c, "border"):
        if k == 0:
            continue
        x, y = d[:, 0], d[:, 1]
        for vx in pc.border_coords(w):
            for vy in pc.border_coords(h):
                assert ((x == F(vx)) & (y == F(vy))).any(), (k, vx, vy)
        s = pc.sane(x, y, w, h)
        assert s.sum() >= 50 and (~s).sum() >= 50
        for v in (-63.5, w + 63.5):
            assert pc.sane(F(v), F(5.0), w, h)
        for v in (-64.0, -64.5, w + 64.0, w + 64.5):
            assert not pc.sane(F(v), F(5.0), w, h)
        # mid-edge members: one coordinate on the border, the other well inside
        assert ((x > 20) & (x < w - 20) & ((y <= 0.5) | (y >= h - 1))).any()
        assert ((y > 20) & (y < h - 20) & ((x <= 0.5) | (x >= w - 1))).any()


def test_position_thresholds_have_members_on_both_sides():
    c = pc.case("thresholds")
    (k, w, h, ins), = labelled(c, "inside")
    (_, _, _, win), = labelled(c, "window")
    (_, _, _, cin), = labelled(c, "cinterior")
    for axis, n in ((0, w), (1, h)):
        p = ins[:, axis]
        # xpos - 7 >= 1: 8 and its upper neighbour pass, its lower neighbour fails; xpos + 8 <= n - 2 likewise around n - 10
        # (the members reach three ulps to either side: the sum xpos + 8 is rounded before it is compared)
        for v, upper in ((8.0, False), (n - 10.0, True)):
            vals = pc.around_wide(v)
            res = [bool(pc.orient_inside_1d(t, n)) for t in vals]
            assert res[3] and True in res and False in res, (axis, v, res)           # the threshold itself passes; both sides
            assert res == sorted(res, reverse=upper), (axis, v, res)                 # one flip, between two neighbours
            for t in vals:
                assert (p == t).sum() >= 3, (axis, t)
        q = win[:, axis]
        lo, mid, hi = pc.around(19.0)
        assert pc.window_interior_1d(mid, n) and pc.window_interior_1d(hi, n) and not pc.window_interior_1d(lo, n)
        lo2, mid2, hi2 = pc.around(n - 20.0)
        assert pc.window_interior_1d(lo2, n) and not pc.window_interior_1d(mid2, n) and not pc.window_interior_1d(hi2, n)
        assert all(pc.window_interior_1d(v, n) for v in pc.around(n - 21.0))
        for v in (lo, mid, hi, lo2, mid2, hi2) + tuple(pc.around(n - 21.0)):
            assert (q == v).sum() >= 3, (axis, v)
        r = cin[:, axis]
        ok = pc.descr_interior_1d(r, cin[:, 2], n)
        other_ok = pc.descr_interior_1d(cin[:, 1 - axis], cin[:, 2], (h if axis == 0 else w))
        assert (ok & other_ok).sum() >= 6 and (~ok & other_ok).sum() >= 6       # this axis alone decides, either way
    # both axes on their threshold at once, all nine combinations of the sides
    for vx, vy in ((8.0, 8.0), (w - 10.0, h - 10.0)):
        for tx in pc.around(vx):
            for ty in pc.around(vy):
                assert ((ins[:, 0] == tx) & (ins[:, 1] == ty)).any()
    for vx, vy in ((19.0, 19.0), (w - 20.0, h - 20.0), (19.0, h - 20.0)):
        for tx in pc.around(vx):
            for ty in pc.around(vy):
                assert ((win[:, 0] == tx) & (win[:, 1] == ty)).any()


def test_binade_class_fails_the_shared_grid_test():
    c = pc.case("binade")
    (k, w, h, bx), = labelled(c, "binade_x")
    (_, _, _, by), = labelled(c, "binade_y")
    (_, _, _, bxy), = labelled(c, "binade_xy")
    ux, uy = ~pc.binade_safe_1d(bx[:, 0]), ~pc.binade_safe_1d(by[:, 1])
    assert ux.sum() >= 10 and uy.sum() >= 10, (ux.sum(), uy.sum())
    assert (~ux).sum() >= 10 and (~uy).sum() >= 10                      # "exactly at the power of two": mostly safe
    assert pc.binade_safe_1d(bx[:, 1]).all() and pc.binade_safe_1d(by[:, 0]).all()      # only x resp. only y can be unsafe
    assert (~pc.binade_safe_1d(bxy[:, 0]) & ~pc.binade_safe_1d(bxy[:, 1])).sum() >= 10
    total_unsafe = 0
    for d in c["dets"]:
        total_unsafe += int((~pc.binade_safe_1d(d[:, 0]) | ~pc.binade_safe_1d(d[:, 1])).sum())
    assert total_unsafe >= 10
    # the construction: (xpos - 4.5) + j is the power of two, or the float just below it (as close as xpos, which lies in a
    # higher binade for small j, can put it: within 32 ulps of the power), for every j = 0 ... 10 and power 4 ... 128
    xp = (bx[:, 0] - F(4.5)).astype(F)
    for p2 in (4, 8, 16, 32, 64, 128):
        for j in range(11):
            s = (xp + F(j)).astype(F)
            assert (s == F(p2)).any(), (p2, j)
            assert ((s < F(p2)) & (s >= F(p2) * F(1.0 - 2.0 ** -19))).any(), (p2, j)


def test_reach_class_straddles_the_window_limit():
    lo, mid, hi = pc.around(pc.REACH_LIMIT)
    rs = pc.reach_scales()
    assert {r for _, r in rs} == {lo, mid, hi}
    c = pc.case("reach")
    edge = np.concatenate([d for _, _, _, d in labelled(c, "reach_edge")])
    r = pc.reach_of(edge[:, 2])
    assert np.isin(r, [lo, mid, hi]).all() and len(r) >= 6
    assert (r == lo).sum() >= 2 and (r == mid).sum() >= 2 and (r == hi).sum() >= 2
    allr = np.concatenate([pc.reach_of(d[:, 2]) for d in c["dets"]])
    assert (allr > pc.REACH_LIMIT).sum() >= 30
    big = np.concatenate([d for _, _, _, d in labelled(c, "reach_big")])
    assert {3.0, 8.0, 40.0} <= set(big[:, 2].tolist())
    tiny = np.concatenate([d for _, _, _, d in labelled(c, "reach_tiny")])
    assert tiny[:, 2].max() <= 0.05
    # within 20 px of every border of the finest level, and in the interior
    (k, w, h, e2), = labelled(c, "reach_edge", 2)
    x, y = e2[:, 0], e2[:, 1]
    for cond in (x < 20, x > w - 20, y < 20, y > h - 20, (x > 40) & (x < w - 40) & (y > 40) & (y < h - 40)):
        for v in (lo, mid, hi):
            assert (cond & (pc.reach_of(e2[:, 2]) == v)).any()
    # 45-degree content: the oracle's orientation of the interior members lies on the diagonal (45 or 225 degrees)
    pts, num, cnt, _ = pc.expected(c, M)
    fin = pts[int(cnt[5]):int(cnt[6])]
    sel = fin[(fin["xpos"] > 40) & (fin["xpos"] < w - 40) & (fin["ypos"] > 40) & (fin["ypos"] < h - 40) & (fin["scale"] > 2.0) &
              (fin["scale"] < 2.2)]
    assert len(sel) >= 3
    assert (np.abs((sel["orientation"] % 180.0) - 45.0) < 12.0).all(), sel["orientation"]
    assert pc.count_big(c, M) >= 30


def test_oracle_meets_its_special_cases_on_the_cases_built_for_them():
    pts, num, cnt, st = pc.expected(pc.case("flat"), M)
    assert st["empty_hists"] > 0 and st["nan_guards"] > 0, st
    c = pc.case("flat")
    # flat patch: orientation 0, and the all-zero descriptor comes out as 1/sqrt(128) in every element (fminf(NaN, 0.2) = 0.2)
    lvl = slice(int(cnt[3]), int(cnt[4]))
    assert (pts["orientation"][lvl] == 0.0).all()
    assert np.allclose(pts["data"][lvl], 1.0 / np.sqrt(128.0), rtol=1e-6, atol=0.0)
    far = np.concatenate([pts[int(cnt[2 * o - 1]):int(cnt[2 * o])][c["labels"][o - 1] == "flat"] for o in (1, 3)])
    assert len(far) >= 40 and (far["orientation"] == 0.0).all() and np.allclose(far["data"], 1.0 / np.sqrt(128.0), rtol=1e-6)
    pts, num, cnt, st = pc.expected(pc.case("dups"), M)
    dups = sum(int(cnt[2 * o + 1]) - int(cnt[2 * o]) for o in (1, 2, 3))
    assert dups >= 20, cnt
    # opposite peaks on the grating: the two orientations of a keypoint differ by about 180 degrees
    seg = pts[int(cnt[3]):int(cnt[5])]
    from util import associate, circ_diff_deg
    first, second = seg[:int(cnt[4]) - int(cnt[3])], seg[int(cnt[4]) - int(cnt[3]):]
    assert len(second) >= 5
    for q in second:
        p = first[first["sharpness"] == q["sharpness"]]
        assert len(p) == 1 and circ_diff_deg(p["orientation"][0], q["orientation"]) > 150.0
    for n in pc.CASE_NAMES:
        p, num, cnt, _ = pc.expected(pc.case(n), M)
        noct = pc.case(n)["geom"][2]
        tot = int(cnt[2 * noct + 1])
        assert tot <= M and not np.isnan(p["data"][:tot]).any(), n
        assert np.isfinite(p["orientation"][:tot]).all() and np.array_equal(cnt[1:2 * noct + 2], np.sort(cnt[1:2 * noct + 2]))
        assert num == int(cnt[2 * noct])


def test_tile_order_is_a_permutation_in_the_device_s_order():
    c = pc.case("interior")
    t = pc.tile_order(c)
    for (w, h), a, b in zip(pc.level_sizes(*c["geom"]), c["dets"], t["dets"]):
        assert sorted(map(tuple, a.tolist())) == sorted(map(tuple, b.tolist()))
        tx = (w >> 5) + 1
        key = np.clip(b[:, 1].astype(np.int32) >> 5, 0, (h >> 5)) * tx + np.clip(b[:, 0].astype(np.int32) >> 5, 0, tx - 1)
        assert (np.diff(key) >= 0).all()
        same = np.diff(key) == 0
        assert (np.diff(b[:, 1])[same] >= 0).all()
    # at a capacity inside octave 2 the oracle keeps a prefix of each octave, and drops are counted
    M2 = 200
    p, num, cnt, st = pc.expected(t, M2)
    assert int(cnt[3]) < M2 < int(cnt[4]) and num == M2 and st["capacity_drops"] >= 0
    full, _, cfull, _ = pc.expected(t, M)
    below = cnt < M2
    assert np.array_equal(cnt[below], cfull[below])
    n1 = int(cnt[3])
    assert np.array_equal(p[:n1].tobytes(), full[:n1].tobytes())
    assert np.array_equal(p[n1:M2].tobytes(), full[int(cfull[3]):int(cfull[3]) + M2 - n1].tobytes())


@pytest.mark.parametrize("scale_up,fix", [(False, False), (True, False), (True, True)])
def test_expected_is_the_oracle_s_extract_on_a_natural_image(stereo, scale_up, fix):
    """points_cases.expected() restates extract_octave and RescalePositions by hand; fed with the levels and the
    detections of the oracle's own pipeline on a photograph it must give orc.extract's records, counters and numPts byte
    for byte — with scale_up (only the first numPts records are halved) and with fix_numpts."""
    from oracle import pyoracle as orc
    img = stereo[0][200:340, 300:480]
    noct, thresh = 3, 2.0
    ref, nref, cref = orc.extract(img, num_octaves=noct, thresh=thresh, scale_up=scale_up, max_pts=M, fix_numpts=fix)
    base = orc.lowpass(orc.scaleup(img) if scale_up else img, 1.0)
    levels = [base]
    for _ in range(noct - 1):
        levels.append(orc.scaledown(levels[-1]))
    levels = levels[::-1]                                          # coarsest first
    dets = []
    for o in range(1, noct + 1):
        sub = float(2 ** (noct - o))
        p, n = orc.findpoints(orc.laplace(levels[o - 1], noct, o), thresh, subsampling=sub, lowest_scale=0.0, max_pts=M)
        dets.append(np.stack([p[f][:n] for f in ("xpos", "ypos", "scale", "sharpness", "edgeness")], axis=1).astype(np.float32))
    h, w = levels[-1].shape
    c = {"name": "natural_%d_%d" % (scale_up, fix), "geom": (w, h, noct), "levels": levels, "dets": dets}
    got, ngot, cgot, _ = pc.expected(c, M, scale_up=scale_up, fix_numpts=fix)
    assert nref == ngot and np.array_equal(cref, cgot), (cref, cgot)
    tot = int(cref[2 * noct + 1])
    assert tot > 60 and int(cref[2 * noct + 1]) > int(cref[2 * noct])           # the finest octave has second orientations
    for f in ("xpos", "ypos", "scale", "sharpness", "edgeness", "orientation", "subsampling", "data"):
        assert np.array_equal(ref[f][:tot], got[f][:tot]), f

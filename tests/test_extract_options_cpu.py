"""The premises of the extraction-option tests (extract_cases.py), each a condition on the ORACLE's output: a GPU test of
test_gpu_extract_options.py must not pass for lack of content.  If one of these fails, the input changes, not the bound."""
import numpy as np
import pytest

import extract_cases as xc
from extract_cases import expected, frames6, small6
from util import associate


def _valid(pts, n, cnt, f, noct):
    """Every record of frame f the per-keypoint kernels wrote (the finest octave's second orientations lie past numPts)."""
    return pts[f, :int(cnt[f][2 * noct + 1])]


def _finest(cnt, noct=4):
    return np.array([xc.octave_counts(c, noct)[0][-1] for c in cnt])


def test_frames6_is_what_the_case_table_was_measured_on():
    pts, n, cnt = expected(frames6())
    assert n.tolist() == [448, 904, 719, 648, 567, 486]
    assert _finest(cnt).tolist() == [174, 450, 317, 269, 240, 173]
    assert n.max() + 1 < xc.ARGS["max_pts"] // 2          # capacity is out of scope: nothing comes near max_pts


def test_weight_modes_differ_on_nearly_every_record():
    """fracbits 8 vs 23: a kernel that took the wrong weight mode anywhere fails on essentially every record."""
    p8, n8, _ = expected(frames6())
    p23, n23, _ = expected(frames6(), fracbits=23)
    assert (n8 != n23).any()                               # even numPts moves (crop 4: 567 -> 565)
    for f in range(6):
        a, b = p8[f, :n8[f]], p23[f, :n23[f]]
        ia, ib, _, _ = associate(a, b)
        assert len(ia) >= 0.95 * min(len(a), len(b)), f
        A, B = a[ia], b[ib]
        orient = (A["orientation"].view(np.uint32) != B["orientation"].view(np.uint32)).sum()
        descr = (np.abs(A["data"].astype(np.float64) - B["data"]).max(axis=1) > 1e-6).sum()
        assert orient >= 0.9 * len(ia) and descr >= 0.9 * len(ia), (f, orient, descr, len(ia))


def test_zero_fraction_bits_mean_exact_weights():
    a, b = expected(frames6(), fracbits=0), expected(frames6(), fracbits=23)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    a, b = expected(frames6()[xc.SINGLE], fracbits=0), expected(frames6()[xc.SINGLE], fracbits=23)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("blur", xc.BLURS)
def test_every_blur_moves_every_frame(blur):
    _, n1, c1 = expected(frames6())
    _, n, c = expected(frames6(), init_blur=blur)
    assert (n != n1).all(), (n, n1)
    assert (n >= 50).all(), n
    fine1, fine = _finest(c1), _finest(c)
    assert (fine > fine1).all() if blur < 1.0 else (fine < fine1).all(), (fine, fine1)


def test_measured_counts_per_blur():
    want = {0.0: [698, 1229, 1147, 966, 832, 828], 0.5: [645, 1203, 1057, 919, 785, 735], 2.0: [185, 347, 323, 275, 250, 189]}
    for blur, n in want.items():
        assert expected(frames6(), init_blur=blur)[1].tolist() == n, blur


def test_partial_floor_cuts_into_the_finest_octave_on_every_frame():
    _, _, c0 = expected(frames6())
    for bits in (8, 23):
        _, _, c = expected(frames6(), lowest_scale=xc.FLOOR_PARTIAL, fracbits=bits)
        for f in range(6):
            d0, d = xc.octave_counts(c0[f], 4)[0], xc.octave_counts(c[f], 4)[0]
            assert d[:3] == d0[:3], f                                    # the coarser octaves are untouched
            assert 0.1 * d0[3] <= d[3] <= 0.9 * d0[3], (f, d[3], d0[3])
    assert _finest(expected(frames6(), lowest_scale=xc.FLOOR_PARTIAL)[2]).tolist() == [69, 149, 141, 107, 84, 89]


def test_high_floor_empties_whole_octaves():
    _, n, c = expected(frames6(), lowest_scale=xc.FLOOR_OCTAVES)
    _, _, c0 = expected(frames6())
    assert n.tolist() == [153, 234, 197, 174, 159, 140]
    for f in range(6):
        d0, d = xc.octave_counts(c0[f], 4)[0], xc.octave_counts(c[f], 4)[0]
        assert d[3] == 0 and 0 < d[2] < d0[2] and d[:2] == d0[:2], (f, d, d0)


@pytest.mark.parametrize("bits", [8, 23])
def test_scale_up_with_the_partial_floor_keeps_records_on_every_frame(bits):
    """scale_up doubles the floor: the up-sampled pyramid's finest octave goes, the next is cut into."""
    _, n, c = expected(small6(), lowest_scale=xc.FLOOR_PARTIAL, scale_up=True, fracbits=bits)
    _, n0, c0 = expected(small6(), scale_up=True, fracbits=bits)
    assert (n >= 10).all(), n
    assert bits != 8 or n.tolist() == [27, 229, 175, 61, 130, 196]
    for f in range(6):
        d0, d = xc.octave_counts(c0[f], 4)[0], xc.octave_counts(c[f], 4)[0]
        assert d[3] == 0 and 0 < d[2] < d0[2] and d[:2] == d0[:2], (f, d, d0)


@pytest.mark.parametrize("case", sorted(xc.CASES))
def test_every_case_has_duplicates_border_and_interior_keypoints(case):
    kw = xc.CASES[case]
    noct = kw.get("num_octaves", xc.ARGS["num_octaves"])
    pts, n, cnt = expected(frames6(), **kw)
    det = np.array([xc.octave_counts(c, noct)[0] for c in cnt])
    dup = np.array([xc.octave_counts(c, noct)[1] for c in cnt])
    # every octave of the batch has second orientations — except the octaves FLOOR_OCTAVES empties on purpose
    live = det.sum(axis=0) > 0
    assert live.all() or kw.get("lowest_scale") == xc.FLOOR_OCTAVES, det
    assert live.sum() >= 3 and (dup.sum(axis=0)[live] >= 1).all(), (det, dup)
    for f in range(6):
        recs = _valid(pts, n, cnt, f, noct)
        d = xc.border_distance(recs)
        assert (d < xc.NEAR).sum() >= xc.NEAR_MIN and (d >= xc.DEEP).sum() >= xc.DEEP_MIN, \
            (case, f, int((d < xc.NEAR).sum()), int((d >= xc.DEEP).sum()))
    assert int(cnt[:, 2 * noct + 1].max()) <= 1441          # capacity overflow is out of scope: max_pts is 4096


def test_the_single_call_frame_has_content_in_every_case():
    for case, kw in xc.CASES.items():
        noct = kw.get("num_octaves", xc.ARGS["num_octaves"])
        pts, n, cnt = expected(frames6()[xc.SINGLE], **kw)
        b, _, cb = expected(frames6(), **kw)
        assert np.array_equal(cnt, cb[xc.SINGLE]), case             # batch and single entry of the oracle agree
        assert n >= 200, (case, n)
    # one octave only (the plain LowPass, no ScaleDown): the finest octave's keypoints at every blur
    for blur in xc.BLURS:
        assert expected(frames6()[xc.SINGLE], init_blur=blur, num_octaves=1)[1] >= 20, blur

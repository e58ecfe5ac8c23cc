"""The premises of the drop-in API scenarios (dropin_cases.py) on the oracle, and its helpers on doctored data.  No GPU:
tools/dropin_check.cpp --list / --poison touch none, and everything else here is the oracle and NumPy."""
import os
import subprocess

import numpy as np
import pytest

import dropin_cases as dc
import extract_capacity_cases as cc
from cudasift_amd.capi import POINT_DTYPE


@pytest.mark.parametrize("flavour", ["default", "managed"])
def test_table_names_are_the_drivers(flavour):
    exe = dc.BINARIES[flavour]
    assert os.path.exists(exe), "%s is not built (make all)" % exe
    r = subprocess.run([exe, "--list"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == dc.scenario_names(flavour)
    r = subprocess.run([exe, "--poison"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and int(r.stdout) == cc.POISON_BYTE


def test_every_scenario_builds_its_inputs(tmp_path):
    """Every input stays within 256 x 192 pixels and 4096 records, and survives the dump."""
    for name, s in dc.SCENARIOS.items():
        for v in s["variants"]:
            e = s["inputs"](v)
            path = tmp_path / ("%s_%s.dump" % (name, v))
            dc.write_dump(path, e)
            back = dc.read_dump(path)
            assert list(back) == list(e), name
            if "w" in e:
                assert e["w"] <= 256 and e["h"] <= 192 and back["img1"].size == e["w"] * e["h"]
                assert back["img1"].dtype == np.float32 and np.array_equal(back["img1"], e["img1"].ravel())
            for k, a in back.items():
                if k.startswith("set"):
                    assert a.dtype == np.uint8 and a.size % 576 == 0 and a.size // 576 <= 4096, (name, k)


def test_extraction_premises():
    """The oracle, under the shim's default cap, gives every image more than 64 keypoints and every second image at least
    32 (below that MatchSiftData compares nothing), and no call overflows the driver's arrays."""
    seen = set()
    for name, s in dc.SCENARIOS.items():
        for size, view in s["extracts"]:
            seen.add((size, view))
            pts, n, cnt = dc.oracle_extract(size, view)
            noct = dc.CALLS[size]["noct"]
            assert n > 64 and (view == 1 or n >= 32), (name, size, view, n)
            assert int(cnt[2 * noct + 1]) <= dc.ALLOC, (name, size, view, cnt)
            cc.key_index(pts[:int(cnt[2 * noct + 1])])          # check_frame's five-field key is unique
    assert seen == {("big", 1), ("big", 2), ("small", 1), ("small", 2)}
    assert dc.oracle_extract("small", 1)[1] == 119 and dc.oracle_extract("small", 2)[1] == 107      # test_gpu_dropin.py's patch
    for size, view in seen:
        assert int(dc.oracle_extract(size, view)[2][2 * dc.CALLS[size]["noct"] + 1]) <= dc.DEMO_MAX
    assert dc.oracle_extract("big", 1)[1] <= dc.DEVICE_ONLY_MAX


def test_the_cap_never_bites_on_these_images():
    """The reference's 32-extrema cap changes no record of any image used here: what the shim's default is held to is the
    oracle WITH the cap, which on these inputs is also the oracle without it (docs/LOG.md says what that leaves open)."""
    from oracle import pyoracle as orc
    for size in dc.CALLS:
        for view in (1, 2):
            c = dc.CALLS[size]
            pts, n, cnt = orc.extract(dc.image(size, view), c["noct"], c["blur"], c["thresh"], max_pts=dc.ALLOC)
            ref, nref, rcnt = dc.oracle_extract(size, view)
            assert n == nref and np.array_equal(cnt, rcnt) and pts[:n].tobytes() == ref[:n].tobytes()


def test_extract_options_premises():
    ref, n, cnt = dc.oracle_extract("big", 1)
    noct = dc.CALLS["big"]["noct"]
    # maxPts below the count: the cap really cuts, and inside a segment
    assert 1 < dc.CAP < n
    cls, seg = cc.classify(cnt, dc.CAP, noct)
    assert cls == "inside a duplicate segment" and seg == ("dup", 3), (cls, seg, cnt)
    assert cc.classify(cnt, 1, noct)[0] == "M = 1"
    # lowestScale: above the smallest scale present, removes some records and keeps some
    low, nlow, _ = dc.oracle_extract("big", 1, lowest_scale=dc.LOWEST_SCALE)
    assert ref["scale"][:n].min() < dc.LOWEST_SCALE < ref["scale"][:n].max()
    assert 0 < nlow < n and low["scale"][:nlow].min() >= dc.LOWEST_SCALE
    # scaleUp: another record set altogether
    up, nup, ucnt = dc.oracle_extract("big", 1, scale_up=True)
    assert nup > n and int(ucnt[2 * noct + 1]) <= dc.ALLOC
    # big_keypoint: whether a keypoint is deferred to descr_big is the kernel's decision (its patch reach against a test
    # knob) and shows only in a device counter: nothing to check without a GPU.  What can be said here is that the frame
    # holds keypoints of scale > 1 at their level, the ones the knob is meant to send there.
    assert ((ref["scale"][:n] / ref["subsampling"][:n]) > 1.0).sum() > 32
    assert dc.BORROWED_PITCH >= dc.CALLS["big"]["w"] and dc.BORROWED_PITCH % 128 and dc.BORROWED_PITCH % 4 and dc.BORROWED_OFFSET % 4


def test_match_premises():
    a, b = dc.match_sets()
    assert len(a) <= dc.MATCH_ALLOC[0] and len(b) <= dc.MATCH_ALLOC[1] and len(b) % 32
    full, n31 = dc.oracle_match(200, 167), dc.oracle_match(200, 31)
    assert (full["match"] >= 0).all() and full["match"].max() < 160          # 32 * (167 // 32) columns are compared
    assert (full["score"][:100] > 0.95).all() and (full["score"][100:] < 0.95).all()
    assert np.array_equal(full["match_xpos"], b["xpos"][full["match"]])
    # every one of the five fields really changes in every record, so an unwritten one shows
    for f in dc.MATCH_FIELDS:
        assert (full[f].view(np.uint32) != a[f].view(np.uint32)).all(), f
    # 31 columns: 32 * (31 // 32) = 0 are compared.  Whatever the oracle leaves is what is asserted
    assert (n31["match"] == -1).all()
    for run, (n1, n2) in dc.MATCH_RUNS.items():
        if not (n1 and n2):
            assert dc.oracle_match(n1, n2).tobytes() == a.tobytes(), run


def test_homography_premises():
    for key, pts in dc.homography_sets().items():
        for explicit in (False, True):
            H, n, H2, numfit, ref = dc.oracle_homography(pts, explicit)
            assert n >= 8 and numfit >= 8 and not np.array_equal(H, H2), (key, explicit, n, numfit)
            assert (ref["match_error"].view(np.uint32) != pts["match_error"].view(np.uint32)).all()
            again = dc.oracle_homography(pts, explicit)
            assert np.array_equal(again[0], H) and again[1] == n        # the seed fixes the answer
    assert len(dc.homography_sets()["setA"]) == 777 and len(dc.homography_sets()["setB"]) == 40


def _distinct_record():
    r = np.zeros(1, POINT_DTYPE)
    r.view(np.uint32)[:] = np.arange(1000, 1000 + 144, dtype=np.uint32)
    return r


def test_dump_round_trip(tmp_path):
    """A dump written by NumPy in the driver's format: scalars, pixels, and a 576-byte record with every word distinct."""
    r = _distinct_record()
    recs = cc.poisoned_records(3, POINT_DTYPE)
    recs[1] = r[0]
    path = tmp_path / "x.dump"
    dc.write_dump(path, {"s1.numPts": 2, "thresh": 4.5, "img1": np.arange(6, dtype=np.float32).reshape(2, 3),
                         "flags": np.array([1, 0, -7], np.int32), "s1.host": recs.view(np.uint8), "empty": np.zeros(0, np.uint8)})
    d = dc.read_dump(path)
    assert list(d) == ["s1.numPts", "thresh", "img1", "flags", "s1.host", "empty"]
    assert dc.scalar(d, "s1.numPts") == 2 and d["s1.numPts"].dtype == np.int32
    assert dc.scalar(d, "thresh") == 4.5 and d["thresh"].dtype == np.float32
    assert d["img1"].tolist() == [0, 1, 2, 3, 4, 5] and d["flags"].tolist() == [1, 0, -7] and d["empty"].size == 0
    got = dc.records(d, "s1.host")
    assert len(got) == 3 and dc.is_poison(got[0]) and dc.is_poison(got[2]) and not dc.is_poison(got[1])
    assert cc.words(got[1:2])[0].tolist() == list(range(1000, 1144))
    # the field offsets the shim's partial copies count on
    assert got["score"].view(np.uint32)[1] == 1000 + 24 // 4 and got["match_ypos"].view(np.uint32)[1] == 1000 + 40 // 4
    assert got["match_error"].view(np.uint32)[1] == 1000 + 44 // 4 and got["data"].view(np.uint32)[1, 0] == 1000 + 64 // 4
    assert cc.words(got[1:2])[0][dc.MATCH_WORDS].tolist() == [1006, 1007, 1008, 1009, 1010] and dc.ERROR_WORD == 11
    # a dump cut short is noticed
    blob = open(path, "rb").read()
    open(path, "wb").write(blob[:-5])
    with pytest.raises(AssertionError):
        dc.read_dump(path)


def test_checkers_notice_doctored_dumps():
    """check_match and check_extraction on dumps made from the oracle's own answer pass; with one word moved they fail."""
    a, b = dc.match_sets()
    want = dc.oracle_match(200, 167)

    def match_dump(mutate=None):
        d1 = cc.poisoned_records(dc.MATCH_ALLOC[0], POINT_DTYPE)
        d1[:200] = a
        for f in dc.MATCH_FIELDS:
            d1[f][:200] = want[f]
        d2 = cc.poisoned_records(dc.MATCH_ALLOC[1], POINT_DTYPE)
        d2[:167] = b
        d = {"full.zero": np.array([0], np.int32), "full.positive": np.array([1], np.int32),
             "full.d1.numPts": np.array([200], np.int32), "full.d2.numPts": np.array([167], np.int32),
             "full.d1.host_null": np.array([0], np.int32)}
        for side in ("host", "dev"):
            d["full.d1." + side] = d1.copy().view(np.uint8)
            d["full.d2." + side] = d2.copy().view(np.uint8)
        if mutate:
            mutate(d)
        return d

    dc.check_match(match_dump(), "full", False)

    def shifted(d):               # an off-by-four in the field copy's offset: match_error arrives, score does not
        h = dc.records(d, "full.d1.host")
        w = cc.words(h)
        w[:200, 6] = cc.words(a)[:, 6]
        w[:200, 11] = 123

    def one_short(d):             # numPts - 1 records copied
        cc.words(dc.records(d, "full.d1.host"))[199, 6:11] = cc.words(a)[199, 6:11]

    def d2_written(d):
        dc.records(d, "full.d2.dev")["score"][3] = 1.0

    for m in (shifted, one_short, d2_written):
        with pytest.raises(AssertionError):
            dc.check_match(match_dump(m), "full", False)

    ref, n, cnt = dc.oracle_extract("big", 1)
    total = int(cnt[2 * 4 + 1])

    def extract_dump(copied):
        dev = cc.poisoned_records(dc.ALLOC, POINT_DTYPE)
        for f in ("xpos", "ypos", "scale", "sharpness", "edgeness", "orientation", "subsampling", "data"):
            dev[f][:total] = ref[f][:total]
        host = cc.poisoned_records(dc.ALLOC, POINT_DTYPE)
        host[:copied] = dev[:copied]
        return {"s1.numPts": np.array([n], np.int32), "s1.maxPts": np.array([dc.ALLOC], np.int32),
                "s1.host_null": np.array([0], np.int32), "s1.host": host.view(np.uint8), "s1.dev": dev.view(np.uint8)}

    assert len(dc.check_extraction(extract_dump(n), "s1", "big", False)) == n
    for copied in (n - 1, n + 1, dc.ALLOC):         # one record short, one too many, maxPts in place of numPts
        with pytest.raises(AssertionError):
            dc.check_extraction(extract_dump(copied), "s1", "big", False)
    dc.check_extraction(extract_dump(total), "s1", "big", True)          # one managed array: the device array itself


def test_print_sift_text():
    """The restatement of PrintSiftData's text on three hand-written records: two decimals, a descriptor element of exactly
    0.05 is printed (float 0.05 is above double 0.05), the next float below it is a dot."""
    recs = np.zeros(3, POINT_DTYPE)
    recs["xpos"], recs["ypos"], recs["scale"] = [1.0, 10.006, 123.456], [2.5, 0.0, 99.995], [1.6, 2.0, 3.25]
    recs["sharpness"], recs["edgeness"], recs["orientation"] = [-4.5, 7.125, 0.0], [3.0, 9.99, 1.0], [0.0, 359.99, 180.0]
    recs["score"] = [0.0, 0.987, -2.9e-16]
    below = np.nextafter(np.float32(0.05), np.float32(0))
    recs["data"][0, 0], recs["data"][0, 8], recs["data"][0, 1], recs["data"][0, 127] = 0.05, below, 0.5, 0.25
    recs["data"][1, :] = 0.0883883
    head0 = ("xpos         = 1.00\nypos         = 2.50\nscale        = 1.60\nsharpness    = -4.50\nedgeness     = 3.00\n"
             "orientation  = 0.00\nscore        = 0.00\n")
    dots = " .   "
    rows0 = ["data = 0.05 " + dots * 15, "       0.50 " + dots * 15] + ["       " + dots * 16] * 5 + \
        ["       " + dots * 15 + "0.25 "]
    head1 = ("xpos         = 10.01\nypos         = 0.00\nscale        = 2.00\nsharpness    = 7.12\nedgeness     = 9.99\n"
             "orientation  = 359.99\nscore        = 0.99\n")
    rows1 = ["data = " + "0.09 " * 16] + ["       " + "0.09 " * 16] * 7
    head2 = ("xpos         = 123.46\nypos         = 100.00\nscale        = 3.25\nsharpness    = 0.00\nedgeness     = 1.00\n"
             "orientation  = 180.00\nscore        = -0.00\n")
    rows2 = ["data = " + dots * 16] + ["       " + dots * 16] * 7
    want = head0 + "\n".join(rows0) + "\n" + head1 + "\n".join(rows1) + "\n" + head2 + "\n".join(rows2) + "\n" + \
        "Number of available points: 3\nNumber of allocated points: 8\n"
    assert dc.print_sift_text(recs, 3, 8) == want
    assert dc.print_sift_text(recs, 0, 8) == "Number of available points: 0\nNumber of allocated points: 8\n"
    assert float(np.float32(0.05)) >= 0.05 > float(below)

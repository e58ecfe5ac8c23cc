"""The CudaSift drop-in C++ API, record for record: tools/dropin_check.cpp (built against include/cudaSift.h and
include/cudaImage.h only, in both flavours of the shim) runs one scenario per child process and dumps what a caller sees;
every record, header field, homography and return value is held to the oracle here (dropin_cases.py has the case table and
the checks).  Then the mode behind every drop-in call — misift_ctx_set_early_return — in process, against the same
context with the mode off.

Children run one after another.  One that is killed by a signal or by its time limit is recorded, and every later test of
this module fails at once without starting another."""
import os
import re
import subprocess

import numpy as np
import pytest

import dropin_cases as dc
import extract_capacity_cases as cc
from cudasift_amd.capi import POINT_DTYPE

pytestmark = pytest.mark.gpu

_dead = []
_runs = {}


@pytest.fixture(autouse=True)
def _nothing_died():
    if _dead:
        pytest.fail("not run, the device may be in a bad state: %s" % _dead[0])


@pytest.fixture(scope="module")
def workroot(tmp_path_factory):
    return tmp_path_factory.mktemp("dropin")


def child(workroot, scenario, flavour="default", variant=None):
    """(dump, stdout) of one scenario in one flavour; run once, shared by the tests that look at it."""
    key = (scenario, flavour, variant)
    if key in _runs:
        return _runs[key]
    if _dead:
        pytest.fail("no further child is started: %s" % _dead[0])
    s = dc.SCENARIOS[scenario]
    assert flavour in s["flavours"] and variant in s["variants"]
    exe = dc.BINARIES[flavour]
    assert os.path.exists(exe), "%s is not built (make all)" % exe
    work = workroot / ("%s_%s_%s" % (scenario, flavour, variant))
    work.mkdir()
    dc.write_dump(work / "in.dump", s["inputs"](variant))
    # the shim's defaults are what is under test: nothing of this process's MISIFT_* settings reaches the child
    env = {k: v for k, v in os.environ.items() if not k.startswith("MISIFT_")}
    if s["quiet"]:
        env["MISIFT_QUIET"] = "1"
    env.update(s["env"])
    try:
        r = subprocess.run([exe, scenario, str(work)], env=env, capture_output=True, timeout=s["timeout"])
    except subprocess.TimeoutExpired:
        _dead.append("%s/%s/%s ran into its time limit of %d s" % (scenario, flavour, variant, s["timeout"]))
        pytest.fail(_dead[0])
    if r.returncode < 0:
        _dead.append("%s/%s/%s was killed by signal %d: %s" % (scenario, flavour, variant, -r.returncode,
                                                               r.stderr.decode(errors="replace")[-1500:]))
        pytest.fail(_dead[0])
    assert r.returncode == 0, (scenario, flavour, r.returncode, r.stderr.decode(errors="replace")[-2000:])
    d = dc.read_dump(work / "out.dump")
    assert dc.scalar(d, "done") == 1 and dc.scalar(d, "managed") == (flavour == "managed")
    assert dc.scalar(d, "poison_byte") == cc.POISON_BYTE
    _runs[key] = (d, r.stdout.decode(errors="replace"), work)
    return _runs[key]


def in_process(size, view=1, knobs=(), early=False, **kw):
    """(records cut to numPts, the context's descr_big launches) of a fresh capi.Context with reference_cap = 1."""
    from cudasift_amd import capi
    c = capi.Context(0)
    try:
        for k, v in dict(knobs).items():
            c.set_knob(k, v)
        c.set_options(reference_cap=1)
        if early:
            c.set_early_return(True)
        call = dc.CALLS[size]
        pts, n, _ = c.extract(dc.image(size, view), call["noct"], call["blur"], call["thresh"], max_pts=dc.ALLOC, **kw)
        return pts[:n], c.descr_big_fallbacks(), int(c.get_counter_block(0)[48])
    finally:
        c.close()


# ------------------------------------------------------------------ extraction
@pytest.mark.parametrize("flavour", ["default", "managed"])
def test_extract_basic(workroot, flavour):
    d, _, _ = child(workroot, "extract_basic", flavour)
    got = dc.check_extraction(d, "s1", "big", flavour == "managed", name="extract_basic/" + flavour)
    assert dc.canon(got) == dc.canon(in_process("big")[0])
    # the image: borrowed host pixels, owned device memory, the pitch of the allocator; Readback at row stride `width`
    c = dc.CALLS["big"]
    assert (dc.scalar(d, "img.width"), dc.scalar(d, "img.height"), dc.scalar(d, "img.pitch")) == (c["w"], c["h"], 256)
    assert dc.scalar(d, "img.d_internalAlloc") == 1 and dc.scalar(d, "img.h_internalAlloc") == 0
    assert dc.scalar(d, "img.h_is_pixels") == 1 and dc.scalar(d, "img.t_null") == 1
    back = d["readback"]
    n = c["w"] * c["h"]
    assert np.array_equal(back[:n].view(np.uint32), dc.image("big").ravel().view(np.uint32))
    assert dc.is_poison(back[n:]) and len(back) == n + 64


def test_extract_lazy_ctx(workroot):
    """No InitCuda, the header's default arguments (tempMemory = 0): the same records as extract_basic, byte for byte."""
    d, _, _ = child(workroot, "extract_lazy_ctx")
    got = dc.check_extraction(d, "s1", "big", False, name="extract_lazy_ctx")
    b, _, _ = child(workroot, "extract_basic")
    assert dc.canon(got) == dc.canon(dc.records(b, "s1.host")[:dc.scalar(b, "s1.numPts")])


def test_extract_options(workroot):
    """scaleUp, lowestScale, maxPts below the count and maxPts = 1, each overwriting the last in the same arrays."""
    d, _, _ = child(workroot, "extract_options")
    up = dc.check_extraction(d, "up", "big", False, scale_up=True)
    assert dc.canon(up) == dc.canon(in_process("big", scale_up=True)[0])
    low = dc.check_extraction(d, "low", "big", False, lowest_scale=dc.LOWEST_SCALE)
    assert dc.canon(low) == dc.canon(in_process("big", lowest_scale=dc.LOWEST_SCALE)[0])
    assert len(dc.check_extraction(d, "cap", "big", False, M=dc.CAP)) == dc.CAP
    assert len(dc.check_extraction(d, "one", "big", False, M=1)) == 1


def test_extract_device_only(workroot):
    """InitSiftData(host = false): ExtractSift synchronises instead of copying; PrintSiftData then allocates h_data, fills
    numPts records of it and prints them."""
    d, _, work = child(workroot, "extract_device_only")
    assert dc.scalar(d, "s1.host_null") == 1
    got = dc.check_extraction(d, "s1", "big", False, alloc=dc.DEVICE_ONLY_MAX, M=dc.DEVICE_ONLY_MAX)
    n = len(got)
    assert dc.scalar(d, "after.host_null") == 0 and dc.scalar(d, "after.numPts") == n
    assert dc.scalar(d, "after.maxPts") == dc.DEVICE_ONLY_MAX and dc.scalar(d, "freed.host_null") == 1
    host = dc.records(d, "after.host")
    assert host.tobytes() == got.tobytes()
    text = open(work / "print.txt").read()
    want = dc.print_sift_text(host, n, dc.DEVICE_ONLY_MAX)
    assert len(text) == len(want) and text == want, [(a, b) for a, b in zip(text.split("\n"), want.split("\n")) if a != b][:3]


def test_image_ownership(workroot):
    d, _, _ = child(workroot, "image_ownership")
    c = dc.CALLS["big"]
    w, h, P, off = c["w"], c["h"], dc.BORROWED_PITCH, dc.BORROWED_OFFSET
    px = dc.image("big")
    # borrowed device memory: pitch kept, nothing owned; the allocation holds the pixels at that pitch and the poison
    # everywhere else, before and after the destructor
    assert dc.scalar(d, "borrowed.pitch") == P and dc.scalar(d, "borrowed.d_is_mine") == 1
    assert dc.scalar(d, "borrowed.h_is_mine") == 1
    assert dc.scalar(d, "borrowed.d_internalAlloc") == 0 and dc.scalar(d, "borrowed.h_internalAlloc") == 0
    want = np.frombuffer(np.full(4 * len(d["pool.before"]), cc.POISON_BYTE, np.uint8).tobytes(), np.float32).copy()
    rows = want[off:off + P * h].reshape(h, P)
    rows[:, :w] = px
    assert np.array_equal(d["pool.before"].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(d["pool.after"].view(np.uint32), want.view(np.uint32)) and dc.scalar(d, "pool.free_rc") == 0
    for k in ("pixels.after", "pixels.end"):
        assert np.array_equal(d[k].view(np.uint32), px.ravel().view(np.uint32)), k
    # owned memory: the pitch passed in (7) is replaced by iAlignUp(w, 128)
    assert dc.scalar(d, "owned.pitch") == 256 and dc.scalar(d, "owned.d_internalAlloc") == 1
    assert dc.scalar(d, "owned.h_internalAlloc") == 1 and dc.scalar(d, "owned.h_null") == 0
    back = d["owned.readback"]
    assert len(back) == 256 * h and np.array_equal(back[:w * h].view(np.uint32), px.ravel().view(np.uint32))
    assert dc.is_poison(back[w * h:])
    assert dc.scalar(d, "hostmem.pitch") == 256 and dc.scalar(d, "hostmem.h_is_mine") == 1
    assert dc.scalar(d, "hostmem.d_internalAlloc") == 1 and dc.scalar(d, "hostmem.h_internalAlloc") == 0
    # the same records from the odd-pitch borrowed image as from the owned one
    a = dc.check_extraction(d, "borrowed.sift", "big", False)
    b = dc.check_extraction(d, "owned.sift", "big", False)
    assert dc.canon(a) == dc.canon(b)


@pytest.mark.parametrize("size", ["big", "small"])
@pytest.mark.parametrize("flavour", ["default", "managed"])
def test_demo_loop(workroot, flavour, size):
    """130 rounds of the demo's inner loop on one scratch arena: the export sequence passes 64, 128, 192 and 256."""
    d, _, _ = child(workroot, "demo_loop", flavour, size)
    for view, s in ((1, "s1"), (2, "s2")):
        got = [dc.check_extraction(d, "r%d.%s" % (r, s), size, flavour == "managed", M=dc.DEMO_MAX, alloc=dc.DEMO_MAX,
                                   view=view, name="demo_loop/%s/%s/r%d.%s" % (flavour, size, r, s))
               for r in (1, 64, dc.DEMO_ROUNDS)]
        assert dc.canon(got[0]) == dc.canon(got[1]) == dc.canon(got[2])


def test_big_keypoint(workroot):
    """A frame whose keypoints descr_all defers to descr_big: in early-return mode that launch is issued after the first
    completion flag and waited for by a second one."""
    d, _, _ = child(workroot, "big_keypoint")
    got = dc.check_extraction(d, "s1", "big", False, name="big_keypoint")
    mine, launches, deferred = in_process("big", knobs={"patch_reach": dc.BIG_REACH}, early=True)
    assert launches == 1 and deferred > 32, (launches, deferred)
    assert dc.canon(got) == dc.canon(mine)
    # ... and it is the knob that sends them there: without it nothing on this frame is deferred
    _, launches0, deferred0 = in_process("big", early=True)
    assert launches0 == 0 and deferred0 == 0


# ------------------------------------------------------------------ matching and geometry
@pytest.mark.parametrize("flavour", ["default", "managed"])
def test_match_fields(workroot, flavour):
    d, _, _ = child(workroot, "match_fields", flavour)
    for run in dc.MATCH_RUNS:
        if run == "nohost" and flavour == "managed":
            assert "nohost.zero" not in d
            continue
        dc.check_match(d, run, flavour == "managed")


@pytest.mark.parametrize("flavour", ["default", "managed"])
def test_homography(workroot, flavour):
    d, _, _ = child(workroot, "homography", flavour)
    for key, pts in dc.homography_sets().items():
        for explicit in (False, True):
            n, numfit = dc.check_homography(d, key, pts, explicit, flavour == "managed")
            assert n >= 8 and numfit >= 8


@pytest.mark.parametrize("flavour", ["default", "managed"])
def test_reinit(workroot, flavour):
    """InitCuda again while the image, the records and the scratch arena are alive."""
    from oracle import pyoracle as orc
    d, out, _ = child(workroot, "reinit", flavour)
    managed = flavour == "managed"
    a = dc.check_extraction(d, "first", "big", managed, name="reinit/first")
    b = dc.check_extraction(d, "second", "big", managed, name="reinit/second")
    assert dc.canon(a) == dc.canon(b)
    # the set against itself: the five fields are the oracle's on these very records, nothing else moved
    n = len(b)
    second, matched = dc.records(d, "second.host"), dc.records(d, "matched.host")
    want = second.copy()
    orc.match(want, n, second.copy(), n)
    assert dc.scalar(d, "match.positive") == 1 and (want["match"][:n] >= 0).all()
    exp = second.copy()
    for f in dc.MATCH_FIELDS:
        exp[f][:n] = want[f][:n]
    assert matched.tobytes() == exp.tobytes()
    assert dc.records(d, "matched.dev")[:n].tobytes() == exp[:n].tobytes()
    assert [dc.scalar(d, "freed." + k) for k in ("host_null", "dev_null", "numPts", "maxPts")] == [1, 1, 0, 0]
    assert out.count("Device Number: 0\n") == 2, out
    bw = [float(x) for x in re.findall(r"Peak Memory Bandwidth \(GB/s\): ([0-9.]+)", out)]
    assert len(bw) == 2 and min(bw) > 0.0, out


def test_chatty(workroot):
    """Without MISIFT_QUIET the calls print what the reference prints."""
    d, out, _ = child(workroot, "chatty")
    got = dc.check_extraction(d, "s1", "big", False, name="chatty")
    n = len(got)
    m1 = re.findall(r"^SIFT extraction time =\s+([0-9.]+) ms (\d+)$", out, re.M)
    m2 = re.findall(r"^Incl prefiltering & memcpy =\s+([0-9.]+) ms (\d+)$", out, re.M)
    m3 = re.findall(r"^MatchSiftData time =\s+([0-9.]+) ms$", out, re.M)
    assert len(m1) == 1 and len(m2) == 1 and len(m3) == 1, out
    assert int(m1[0][1]) == n and int(m2[0][1]) == n and float(m2[0][0]) >= float(m1[0][0])
    assert dc.scalar(d, "match.positive") == 1
    quiet_out = child(workroot, "extract_basic")[1]
    assert "SIFT extraction time" not in quiet_out and "Device Number: 0" in quiet_out


# ------------------------------------------------------------------ the early-return mode, in process
@pytest.fixture
def fresh(ctx):
    from cudasift_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def both_modes(c, fn):
    c.set_early_return(False)
    off = fn()
    c.set_early_return(True)
    try:
        return off, fn()
    finally:
        c.set_early_return(False)


def test_early_return_extract(fresh):
    for size in ("big", "small"):
        call = dc.CALLS[size]
        off, on = both_modes(fresh, lambda: fresh.extract(dc.image(size), call["noct"], call["blur"], call["thresh"],
                                                          max_pts=dc.ALLOC))
        assert on[1] == off[1] == dc.oracle_extract(size)[1] and np.array_equal(on[2], off[2])
        assert dc.canon(on[0][:on[1]]) == dc.canon(off[0][:off[1]])


@pytest.mark.parametrize("nframes", [1, 4, 5])
def test_early_return_extract_batch(fresh, nframes):
    """Both sides of small_frames (4): the latency-bound launch shapes and the batch ones."""
    c = dc.CALLS["big"]
    y, x = 432, 704
    left = dc._left()
    frames = np.stack([left[y:y + c["h"], x + 16 * f:x + 16 * f + c["w"]].astype(np.float32) for f in range(nframes)])
    off, on = both_modes(fresh, lambda: fresh.extract_batch(frames, c["noct"], c["blur"], c["thresh"], max_pts=1024))
    assert np.array_equal(on[1], off[1]) and on[1].min() > 64
    assert on[1][0] == dc.oracle_extract("big")[1]
    for f in range(nframes):
        assert dc.canon(on[0][f, :on[1][f]]) == dc.canon(off[0][f, :off[1][f]]), f


def test_early_return_match(fresh):
    a, b = dc.match_sets()
    off, on = both_modes(fresh, lambda: fresh.match(a, len(a), b, len(b)))
    assert on.tobytes() == off.tobytes()
    want = dc.oracle_match(len(a), len(b))
    for f in dc.MATCH_FIELDS:
        assert np.array_equal(on[f].view(np.uint32), want[f].view(np.uint32)), f


def test_early_return_find_homography(fresh):
    from oracle import pyoracle as orc
    pts = dc.homography_sets()["setA"]
    buf = fresh.upload(pts)

    def run():
        orc.srand(dc.HOMOGRAPHY["seed"])
        return fresh.find_homography(buf.ptr, len(pts), num_loops=2000, min_score=0.0, max_ambiguity=0.9, thresh=4.0)
    off, on = both_modes(fresh, run)
    assert on[1] == off[1] and np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32))
    want = dc.oracle_homography(pts, True)
    assert on[1] == want[1] and np.array_equal(on[0].view(np.uint32), want[0].view(np.uint32))


def test_early_return_130_alternating_extractions(fresh):
    """The demo's loop on the C-ABI with the mode on: the export sequence passes 64, 128, 192 and 256 (each drains the
    runtime); the last pair of record sets equals the first."""
    from cudasift_amd import capi
    call = dc.CALLS["big"]
    w, h, M = call["w"], call["h"], dc.DEMO_MAX
    imgs = [fresh.upload_image(dc.image("big", v)) for v in (1, 2)]
    scratch = capi.DevBuf(4 * capi.scratch_floats(w, h, call["noct"], False))
    pts = [capi.DevBuf(576 * M) for _ in range(2)]
    fresh.set_early_return(True)
    first = None
    for r in range(dc.DEMO_ROUNDS // 2):
        pair = []
        keep = r == 0 or r == dc.DEMO_ROUNDS // 2 - 1
        for v in range(2):
            if keep:
                capi.check(capi.lib().misift_memset(fresh.h, pts[v].ptr, cc.POISON_BYTE, 576 * M), "misift_memset")
            rc, n = fresh.extract_raw(imgs[v][0].ptr, w, h, imgs[v][1], scratch.ptr, pts[v].ptr, call["noct"], call["blur"],
                                      call["thresh"], max_pts=M)
            capi.check(rc, "misift_extract")
            if keep:
                pair.append((n, fresh.download(pts[v], (M,), POINT_DTYPE)))
        if r == 0:
            first = pair
    for v in range(2):
        ref, nref, cnt = dc.oracle_extract("big", v + 1)
        for n, rows in (first[v], pair[v]):
            cc.check_frame(ref, cnt, M, rows, noct=call["noct"], num_pts=n, name="alternating/view%d" % (v + 1))
        assert dc.canon(first[v][1][:nref]) == dc.canon(pair[v][1][:nref])

"""The CudaSift drop-in C++ API (include/cudaSift.h + include/cudaImage.h over cudasift_amd/csrc/shim_cudasift.cpp),
record for record: the case table of tools/dropin_check.cpp's scenarios, the reader / writer of its dumps, the oracle's
restatement of every scenario and the checks (test_dropin_cases_cpu.py checks the premises on the oracle and the helpers
on doctored data, test_gpu_dropin_api.py runs the driver).  No GPU in here.

What the shim adds to the C-ABI, and the scenario that fails when it breaks:
  1. early return (misift_ctx_set_early_return in make_ctx): every scenario runs in that mode; demo_loop carries the
     export sequence past 64, 128, 192 and 256 (the runtime is drained there), big_keypoint takes the deferred descr_big
     launch behind the first flag.
  2. reference_cap = 1 by default: every extraction is compared with the oracle under orc.reference_cap(1).  (No image of
     the sizes used here holds more than 32 extrema in a 30 x 8 block, so the cap never bites: see docs/LOG.md.)
  3. partial read-backs: numPts records after ExtractSift (the rest of h_data keeps the poison), 5 fields at offset 24
     after MatchSiftData, 1 field at offset 44 after ImproveHomographyGPU (every other byte keeps what was there), and the
     h_data == NULL branches (extract_device_only, match_fields 'nohost').
  4. ownership and lifetime: image_ownership, reinit, extract_lazy_ctx, extract_device_only (PrintSiftData's h_data).

A dump (in.dump written here, out.dump written by the driver) is a sequence of little-endian entries
    u32 name length | name | u32 kind (0 int32, 1 float32, 2 bytes) | u64 payload bytes | payload
read_dump returns {name: array}; records travel as bytes and are viewed through records()."""
import functools
import os
import struct

import numpy as np

import extract_capacity_cases as cc
from cudasift_amd.capi import POINT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARIES = {"default": os.path.join(ROOT, "build", "dropin_check"),
            "managed": os.path.join(ROOT, "build", "dropin_check_managed")}
KIND_I32, KIND_F32, KIND_BYTES = 0, 1, 2
_KINDS = {KIND_I32: np.dtype("<i4"), KIND_F32: np.dtype("<f4"), KIND_BYTES: np.dtype("u1")}
ALLOC = 4096                                # records the driver gives InitSiftData unless the case says otherwise
MATCH_FIELDS = ("score", "ambiguity", "match", "match_xpos", "match_ypos")      # 20 bytes at offset 24
MATCH_WORDS = np.arange(6, 11)
ERROR_WORD = 11                             # match_error, offset 44


# ------------------------------------------------------------------ dumps
def write_dump(path, entries):
    """entries: {name: int | float | ndarray}.  int -> one int32, float -> one float32, an int32 / float32 array as such,
    anything else (records, uint8) as bytes."""
    with open(path, "wb") as f:
        for name, v in entries.items():
            if isinstance(v, (int, np.integer)):
                kind, a = KIND_I32, np.array([v], "<i4")
            elif isinstance(v, (float, np.floating)):
                kind, a = KIND_F32, np.array([v], "<f4")
            else:
                a = np.ascontiguousarray(v)
                kind = KIND_I32 if a.dtype == np.int32 else KIND_F32 if a.dtype == np.float32 else KIND_BYTES
            raw = a.tobytes()
            nm = name.encode()
            f.write(struct.pack("<I", len(nm)) + nm + struct.pack("<IQ", kind, len(raw)) + raw)


def read_dump(path):
    out = {}
    with open(path, "rb") as f:
        blob = f.read()
    pos = 0
    while pos < len(blob):
        assert pos + 4 <= len(blob), "dump cut short in an entry's header"
        (ln,) = struct.unpack_from("<I", blob, pos)
        assert pos + 4 + ln + 12 <= len(blob), "dump cut short in an entry's header"
        name = blob[pos + 4:pos + 4 + ln].decode()
        kind, nbytes = struct.unpack_from("<IQ", blob, pos + 4 + ln)
        pos += 4 + ln + 12
        assert pos + nbytes <= len(blob), "dump cut short in entry %r" % name
        out[name] = np.frombuffer(blob[pos:pos + nbytes], _KINDS[kind]).copy()
        pos += nbytes
    return out


def scalar(d, name):
    a = d[name]
    assert a.shape == (1,), (name, a.shape)
    return a[0].item()


def records(d, name):
    a = d[name]
    assert a.dtype == np.uint8 and a.size % 576 == 0, (name, a.dtype, a.size)
    return a.view(POINT_DTYPE)


def is_poison(x):
    """Every byte of x is the poison."""
    return bool((np.ascontiguousarray(x).view(np.uint8) == cc.POISON_BYTE).all())


# ------------------------------------------------------------------ inputs
CALLS = {"big": dict(w=256, h=192, noct=4, blur=1.0, thresh=4.5),          # the fused single-call path
         "small": dict(w=100, h=100, noct=5, blur=1.0, thresh=4.5)}        # coarsest level 6 px: the tiny-call path
# the most textured 256 x 192 window of left.pgm on a 16-pixel grid (sum of |gradient|), and test_gpu_dropin.py's
# 100 x 100 patch; the second view is the first 7 px further right
_WINDOWS = {"big": (432, 704), "small": (500, 700)}
SHIFT = 7


@functools.lru_cache(maxsize=None)
def _left():
    return np.load(os.path.join(ROOT, "tests", "golden", "stereo_pair_u8.npz"))["left"]


def image(size, view=1):
    y, x = _WINDOWS[size]
    c = CALLS[size]
    x += SHIFT * (view - 1)
    return np.ascontiguousarray(_left()[y:y + c["h"], x:x + c["w"]].astype(np.float32))


def call_entries(size):
    c = CALLS[size]
    return {"w": c["w"], "h": c["h"], "noct": c["noct"], "blur": float(c["blur"]), "thresh": float(c["thresh"])}


@functools.lru_cache(maxsize=None)
def oracle_extract(size, view=1, scale_up=False, lowest_scale=0.0):
    """(records [ALLOC], numPts, counters [17]) of the oracle for one image under the shim's default: the reference's
    32-extrema cap on.  ALLOC records hold every call of the table uncapped."""
    from oracle import pyoracle as orc
    c = CALLS[size]
    with orc.reference_cap(1):
        pts, n, cnt = orc.extract(image(size, view), c["noct"], c["blur"], c["thresh"], lowest_scale=lowest_scale,
                                  scale_up=scale_up, max_pts=ALLOC)
    assert int(cnt[2 * c["noct"] + 1]) <= ALLOC
    pts.setflags(write=False)
    return pts, int(n), cnt


LOWEST_SCALE = 2.0
CAP = 150                                   # the oracle finds 286: row 150 lies inside octave 3's second orientations
DEVICE_ONLY_MAX = 512
BORROWED_PITCH, BORROWED_OFFSET = 259, 5    # floats: no multiple of 128 (nor of 4), d_data 20 bytes into the allocation
DEMO_ROUNDS, DEMO_MAX = 130, 512
BIG_ENV = {"MISIFT_TUNABLES": "1", "MISIFT_TEST_PATCH_REACH": "9"}      # every keypoint of scale > 1.0 goes to descr_big
BIG_REACH = 9.0


def match_sets():
    """Two record sets with every field set to something of its own, so that a byte MatchSiftData must not touch shows.
    167 columns: the matcher compares 32 * (167 // 32) = 160 of them."""
    from synth import synth_descriptors
    rng = np.random.default_rng(77)
    sets = []
    for n, seed in ((200, 1), (167, 2)):
        p = np.zeros(n, POINT_DTYPE)
        p["data"] = synth_descriptors(n, seed=seed, l2=True)
        for f in ("xpos", "ypos", "scale", "sharpness", "edgeness", "orientation", "score", "ambiguity", "match_xpos",
                  "match_ypos", "match_error", "subsampling"):
            p[f] = rng.uniform(1.0, 200.0, n).astype(np.float32)
        p["empty"] = rng.uniform(1.0, 2.0, (n, 3)).astype(np.float32)
        p["match"] = rng.integers(1000, 2000, n)
        sets.append(p)
    # half of set 1 are noisy copies of members of set 2: scores near 1 next to scores near 0.75
    src = rng.integers(0, 160, 100)
    d = sets[1]["data"][src] + rng.normal(0, 0.01, (100, 128)).astype(np.float32)
    sets[0]["data"][:100] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return sets[0], sets[1]


MATCH_ALLOC = (256, 192)
MATCH_RUNS = {"full": (200, 167), "zero1": (0, 167), "zero2": (200, 0), "n31": (200, 31), "nohost": (200, 167)}


def oracle_match(n1, n2):
    """Set 1 after MatchSiftData(set 1 cut to n1, set 2 cut to n2) by the oracle; untouched where the shim returns early."""
    from oracle import pyoracle as orc
    a, b = match_sets()
    out = a.copy()
    if n1 and n2:
        orc.match(out, n1, b.copy(), n2)
    return out


HOMOGRAPHY = dict(seed=11, loops=2000, min_score=0.0, max_ambiguity=0.9, thresh=4.0, improve_loops=5,
                  improve_min_score=0.0, improve_max_ambiguity=0.95, improve_thresh=3.5)
HOMOGRAPHY_DEFAULT = dict(loops=1000, min_score=0.85, max_ambiguity=0.95, thresh=5.0, improve_loops=5,
                          improve_min_score=0.0, improve_max_ambiguity=0.80, improve_thresh=3.0)
HOMOGRAPHY_SLACK = 16                       # records the driver allocates behind the set


def homography_sets():
    from synth import synth_matches
    return {"setA": synth_matches(777, inlier_frac=0.55, seed=2)[0], "setB": synth_matches(40, seed=3)[0]}


def oracle_homography(pts, explicit):
    """(H found, numMatches, H improved, numfit, records with match_error) by the oracle, libc rand() seeded as the
    driver seeds it."""
    from oracle import pyoracle as orc
    a = dict(HOMOGRAPHY_DEFAULT, **(HOMOGRAPHY if explicit else {}))
    ref = pts.copy()
    orc.srand(HOMOGRAPHY["seed"])
    H, n, _ = orc.find_homography(ref, len(ref), a["loops"], a["min_score"], a["max_ambiguity"], a["thresh"])
    H2, numfit = orc.improve_homography(ref, len(ref), H, a["improve_loops"], a["improve_min_score"],
                                        a["improve_max_ambiguity"], a["improve_thresh"])
    return H, n, H2, numfit, ref


def _img(size, both=False):
    e = call_entries(size)
    e["img1"] = image(size, 1)
    if both:
        e["img2"] = image(size, 2)
    return e


def _match_inputs():
    a, b = match_sets()
    return {"set1": a.view(np.uint8), "set2": b.view(np.uint8), "alloc1": MATCH_ALLOC[0], "alloc2": MATCH_ALLOC[1]}


def _homography_inputs():
    e = {k: v.view(np.uint8) for k, v in homography_sets().items()}
    for k, v in HOMOGRAPHY.items():
        e[k] = v
    return e


# Every child starts the HIP runtime, two contexts (the shim's and the driver's) and their self-tests: BASE_TIMEOUT covers
# that on a busy machine; what a scenario does on top is a handful of sub-millisecond calls, 260 of them for demo_loop.
BASE_TIMEOUT = 90
# name -> flavours, the variants it is run in (None: one run), inputs(variant), extra environment, quiet, time limit (s),
# extraction images [(size, view)] whose premises the CPU test checks
SCENARIOS = {
    "extract_basic": dict(flavours=("default", "managed"), inputs=lambda v: _img("big"), extracts=[("big", 1)]),
    "extract_lazy_ctx": dict(inputs=lambda v: _img("big"), extracts=[("big", 1)]),
    "extract_options": dict(inputs=lambda v: dict(_img("big"), lowest_scale=LOWEST_SCALE, cap=CAP), extracts=[("big", 1)]),
    "extract_device_only": dict(inputs=lambda v: dict(_img("big"), max_pts=DEVICE_ONLY_MAX), extracts=[("big", 1)]),
    "image_ownership": dict(inputs=lambda v: dict(_img("big"), borrowed_pitch=BORROWED_PITCH,
                                                  borrowed_offset=BORROWED_OFFSET), extracts=[("big", 1)]),
    "demo_loop": dict(flavours=("default", "managed"), variants=("big", "small"),
                      inputs=lambda v: dict(_img(v, both=True), max_pts=DEMO_MAX, rounds=DEMO_ROUNDS),
                      extracts=[("big", 1), ("big", 2), ("small", 1), ("small", 2)], timeout=BASE_TIMEOUT + 60),
    "big_keypoint": dict(inputs=lambda v: _img("big"), env=BIG_ENV, extracts=[("big", 1)]),
    "match_fields": dict(flavours=("default", "managed"), inputs=lambda v: _match_inputs()),
    "homography": dict(flavours=("default", "managed"), inputs=lambda v: _homography_inputs()),
    "reinit": dict(flavours=("default", "managed"), inputs=lambda v: _img("big"), extracts=[("big", 1)]),
    "chatty": dict(inputs=lambda v: _img("big"), quiet=False, extracts=[("big", 1)]),
}
for _s in SCENARIOS.values():
    _s.setdefault("flavours", ("default",))
    _s.setdefault("variants", (None,))
    _s.setdefault("env", {})
    _s.setdefault("quiet", True)
    _s.setdefault("timeout", BASE_TIMEOUT)
    _s.setdefault("extracts", [])


def scenario_names(flavour):
    return [k for k, s in SCENARIOS.items() if flavour in s["flavours"]]


# ------------------------------------------------------------------ checks
def canon(recs):
    """The fields ExtractSift writes, in a canonical record order (test_gpu_guard._canon)."""
    from test_gpu_guard import _canon
    return _canon(recs)


def check_extraction(d, prefix, size, managed, M=ALLOC, alloc=ALLOC, name="", **oracle_kw):
    """One ExtractSift call's dump (<prefix>.numPts / .host / .dev, arrays of `alloc` poisoned records, maxPts = M)
    against the oracle.  Returns the host records cut to numPts."""
    from util import compare_points
    name = name or prefix
    view = oracle_kw.pop("view", 1)
    ref, nref, cnt = oracle_extract(size, view, **oracle_kw)
    noct = CALLS[size]["noct"]
    total = int(cnt[2 * noct + 1])
    n = scalar(d, prefix + ".numPts")
    assert n == min(nref, M), "%s: numPts %d, the oracle finds %d (maxPts %d)" % (name, n, nref, M)
    assert scalar(d, prefix + ".maxPts") == M, name
    dev = records(d, prefix + ".dev")
    assert len(dev) == alloc, (name, len(dev))
    # the device array: misift_extract's capacity rule (records up to min(total, M), nothing behind them)
    cc.check_frame(ref, cnt, M, dev[:M], noct=noct, num_pts=n, name=name + "/dev")
    assert is_poison(dev[M:]), "%s: device records behind maxPts = %d were written" % (name, M)
    if scalar(d, prefix + ".host_null"):
        return dev[:n]
    host = records(d, prefix + ".host")
    assert len(host) == alloc, (name, len(host))
    assert host[:n].tobytes() == dev[:n].tobytes(), "%s: h_data[:numPts] is not d_data[:numPts]" % name
    # ExtractSift copies numPts records; one managed array is the device array (the finest octave's second orientations
    # lie behind numPts, like the reference's)
    kept = min(total, M) if managed else n
    bad = np.nonzero((cc.words(host[kept:]) != cc.POISON_U32).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d host records behind row %d were written, first %s" % (name, len(bad), kept, bad[:8] + kept)
    if M >= nref:
        compare_points(ref[:nref], host[:n], "dropin/" + name)
    return host[:n]


def check_match(d, run, managed):
    """One MatchSiftData run of match_fields against the oracle: the five fields bit for bit, every other byte as it was."""
    n1, n2 = MATCH_RUNS[run]
    a, b = match_sets()
    want = oracle_match(n1, n2)
    touched = bool(n1 and n2)
    assert scalar(d, run + ".zero") == (0 if touched else 1) and scalar(d, run + ".positive") == (1 if touched else 0), run
    assert scalar(d, run + ".d1.numPts") == n1 and scalar(d, run + ".d2.numPts") == n2, run
    before = []
    for recs, alloc in ((a, MATCH_ALLOC[0]), (b, MATCH_ALLOC[1])):
        p = cc.poisoned_records(alloc, POINT_DTYPE)
        p[:len(recs)] = recs
        before.append(p)
    exp = before[0].copy()
    for f in MATCH_FIELDS:
        exp[f][:n1] = want[f][:n1]
    sides = [("dev", exp)]
    if run == "nohost":
        assert scalar(d, run + ".d1.host_null") == 1
    else:
        assert scalar(d, run + ".d1.host_null") == 0
        sides.append(("host", exp))
    for side, e in sides:
        got = records(d, "%s.d1.%s" % (run, side))
        gw, ew = cc.words(got), cc.words(e)
        diff = np.argwhere(gw != ew)
        in_fields = np.isin(diff[:, 1], MATCH_WORDS) if len(diff) else np.zeros(0, bool)
        assert len(diff) == 0, "%s: d1 %s differs from the oracle in %d words (%d of them inside the five fields), first " \
            "(record, word) %s: got %#x, want %#x" % (run, side, len(diff), int(in_fields.sum()), diff[0],
                                                      gw[tuple(diff[0])], ew[tuple(diff[0])])
    for side in ("dev", "host"):
        assert records(d, "%s.d2.%s" % (run, side)).tobytes() == before[1].tobytes(), "%s: d2 %s was written" % (run, side)
    return want


def check_homography(d, key, pts, explicit, managed):
    """FindHomography + ImproveHomographyGPU of one set: H, numMatches, numfit and every match_error bit for bit; nothing
    but offset 44 of records [0, numPts) changes in either array."""
    H, n, H2, numfit, ref = oracle_homography(pts, explicit)
    p = "%s.%s" % (key, "explicit" if explicit else "default")
    npts, alloc = len(pts), len(pts) + HOMOGRAPHY_SLACK
    assert scalar(d, p + ".numMatches") == n, (p, scalar(d, p + ".numMatches"), n)
    assert d[p + ".H_found"].view(np.uint32).tolist() == H.reshape(9).view(np.uint32).tolist(), (p, d[p + ".H_found"], H)
    assert scalar(d, p + ".numfit") == numfit, (p, scalar(d, p + ".numfit"), numfit)
    assert d[p + ".H_improved"].view(np.uint32).tolist() == H2.reshape(9).view(np.uint32).tolist(), (p, d[p + ".H_improved"], H2)
    before = cc.poisoned_records(alloc, POINT_DTYPE)
    before[:npts] = pts
    for side in ("host", "dev"):
        got = records(d, "%s.found.%s" % (p, side))
        assert got.tobytes() == before.tobytes(), "%s: FindHomography changed the %s records" % (p, side)
        got = records(d, "%s.improved.%s" % (p, side))
        assert len(got) == alloc
        gw, bw = cc.words(got), cc.words(before)
        other = np.delete(np.arange(cc.RECORD_WORDS), ERROR_WORD)
        assert np.array_equal(gw[:, other], bw[:, other]), "%s: ImproveHomographyGPU changed more than match_error (%s)" % (p, side)
        assert np.array_equal(gw[npts:, ERROR_WORD], bw[npts:, ERROR_WORD]), "%s: match_error written behind numPts (%s)" % (p, side)
        assert np.array_equal(gw[:npts, ERROR_WORD], ref["match_error"].view(np.uint32)), \
            "%s: match_error differs from the oracle's (%s)" % (p, side)
    return n, numfit


# ------------------------------------------------------------------ PrintSiftData
_PRINT_FIELDS = (("xpos         ", "xpos"), ("ypos         ", "ypos"), ("scale        ", "scale"),
                 ("sharpness    ", "sharpness"), ("edgeness     ", "edgeness"), ("orientation  ", "orientation"),
                 ("score        ", "score"))


def print_sift_text(recs, num_pts, max_pts):
    """What PrintSiftData writes for the first num_pts records: seven fields with two decimals, the descriptor as 8 rows
    of 16 (element j + 8 k in row j, column k), elements below 0.05 as a dot, then the two counts."""
    out = []
    for r in recs[:num_pts]:
        for label, f in _PRINT_FIELDS:
            out.append("%s= %.2f\n" % (label, float(r[f])))
        desc = r["data"]
        for j in range(8):
            out.append("data = " if j == 0 else "       ")
            for k in range(16):
                v = float(desc[j + 8 * k])
                out.append(" .   " if v < 0.05 else "%.2f " % v)
            out.append("\n")
    out.append("Number of available points: %d\n" % num_pts)
    out.append("Number of allocated points: %d\n" % max_pts)
    return "".join(out)

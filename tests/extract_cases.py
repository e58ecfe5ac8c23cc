"""Inputs, oracle results and the case table of the extraction-option tests (test_extract_options_cpu.py checks the
premises on the oracle's output, test_gpu_extract_options.py runs the HIP path against it).  No GPU in here.

frames6: six 483 x 270 crops of the committed stereo pair.  Real image content — the band-limited synth_frame leaves
the finest octave nearly empty — and an odd width (the generic kernels, width % 4 != 0).  Oracle, ARGS below: numPts =
448, 904, 719, 648, 567, 486; finest-octave keypoints 174, 450, 317, 269, 240, 173.

Crop 0 was left[100:370, 60:543] at first: 152 keypoints, and in the sparse cases (init_blur 2, lowest_scale 3) 48 - 63
records of which 9 - 13 lie 19 texels inside their octave, so the content premises of test_extract_options_cpu.py failed
on it, and its upper-left quarter (sky) gave no keypoint under scale_up.  The input changed, not the bound: the crop
below holds 153 - 698 records in every case, at least 39 near a border and 65 deep inside.
"""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H = 483, 270
CROPS = [("left", 300, 200), ("left", 400, 700), ("right", 250, 333), ("right", 620, 41), ("left", 650, 380),
         ("right", 5, 790)]
ARGS = dict(num_octaves=4, thresh=3.0, max_pts=4096)

# The scale floors (searched on the oracle, finest-octave detections per frame; without a floor 174, 450, 317, 269, 240, 173):
#   lowest_scale 1.2: 150, 361, 300, 257, 204, 172   (crop 5 keeps 99 %: too little is cut)
#   lowest_scale 1.4:  95, 212, 228, 179, 126, 142
#   lowest_scale 1.5:  69, 149, 141, 107,  84,  89   <- FLOOR_PARTIAL: 33 % - 51 % of the finest octave stays on every frame
#   lowest_scale 1.6:  12,  56,  42,  34,  26,  41   (crop 0 keeps 7 %: too much is cut)
#   lowest_scale 1.8:   3,  18,  15,  17,  10,  16
#   lowest_scale 2.0: the finest octave is empty on every frame
#   lowest_scale 3.0: the finest octave is empty and the next keeps 45, 66, 50, 49, 27, 42 of 147, 252, 224, 214, 165, 178;
#                     numPts 153, 234, 197, 174, 159, 140              <- FLOOR_OCTAVES
FLOOR_PARTIAL = 1.5
FLOOR_OCTAVES = 3.0
# scale_up doubles the floor (it is applied to the up-sampled image's scales): at 1.5 the up-sampled pyramid's finest octave
# is empty and the next one keeps 4, 65, 42, 8, 35, 54 of 24, 302, 189, 34, 120, 138 on small6(); numPts 27, 229, 175, 61,
# 130, 196 (at 2.0 the second octave is empty as well: 21 - 136 records)
BLURS = (0.0, 0.5, 2.0)

# name -> the oracle's keywords on top of ARGS, each run on frames6 (or its first frames, or frame SINGLE alone)
CASES = {
    "bits8": dict(),
    "bits23": dict(fracbits=23),
    "blur0.0": dict(init_blur=0.0),
    "blur0.5": dict(init_blur=0.5),
    "blur2.0": dict(init_blur=2.0),
    "blur0.5/bits23": dict(init_blur=0.5, fracbits=23),
    "floor1.5": dict(lowest_scale=FLOOR_PARTIAL),
    "floor1.5/bits23": dict(lowest_scale=FLOOR_PARTIAL, fracbits=23),
    "floor3.0": dict(lowest_scale=FLOOR_OCTAVES),
    "floor3.0/bits23": dict(lowest_scale=FLOOR_OCTAVES, fracbits=23),
    "blur2.0/3oct": dict(init_blur=2.0, num_octaves=3),            # configuration C of the stale-state sequence
}
SINGLE = 1            # the frame the single calls use (the busiest: 904 keypoints)
# Content premises per frame: >= NEAR_MIN records within NEAR texels of a border of their octave (the clamped fetches),
# >= DEEP_MIN records at least DEEP texels inside (the clamp-free interior path), on every frame of every case.
NEAR, NEAR_MIN, DEEP, DEEP_MIN = 8, 20, 19, 20

_cache = {}


def _stereo():
    if "stereo" not in _cache:
        z = np.load(os.path.join(GOLDEN, "stereo_pair_u8.npz"))
        _cache["stereo"] = {"left": z["left"], "right": z["right"]}
    return _cache["stereo"]


def frames6_u8():
    """[6, 270, 483] uint8 (read-only)."""
    if "frames6" not in _cache:
        s = _stereo()
        f = np.stack([s[im][y:y + H, x:x + W] for im, y, x in CROPS])
        assert f.shape == (6, H, W) and f.dtype == np.uint8
        f.setflags(write=False)
        _cache["frames6"] = f
    return _cache["frames6"]


def frames6():
    """[6, 270, 483] float32 (read-only): the same pixels."""
    if "frames6f" not in _cache:
        f = frames6_u8().astype(np.float32)
        f.setflags(write=False)
        _cache["frames6f"] = f
    return _cache["frames6f"]


def small6():
    """[6, 135, 241] float32 for the scale_up runs: the upper-left quarter of each crop."""
    if "small6" not in _cache:
        s = np.ascontiguousarray(frames6()[:, :135, :241])
        s.setflags(write=False)
        _cache["small6"] = s
    return _cache["small6"]


def expected(frames, **kw):
    """The oracle's result for `frames` with ARGS overridden by kw (fracbits, init_blur, lowest_scale, num_octaves,
    scale_up), computed once per (pixels, keywords) and shared: do not write into it.
    frames [h, w]: (points, numPts, counters[17]) of pyoracle.extract.
    frames [B, h, w]: (points[B], numPts[B], counters[B, 17]) of pyoracle.extract_batch — frame by frame through extract
    with scale_up, which the oracle's batch entry does not have."""
    from oracle import pyoracle as orc
    frames = np.ascontiguousarray(frames, np.float32)
    a = dict(ARGS, **kw)
    key = (hashlib.sha1(frames.tobytes()).hexdigest(), frames.shape, tuple(sorted(a.items())))
    if key not in _cache:
        if frames.ndim == 2:
            r = orc.extract(frames, **a)
        elif a.get("scale_up"):
            rs = [orc.extract(f, **a) for f in frames]
            r = (np.stack([x[0] for x in rs]), np.array([x[1] for x in rs], np.int32), np.stack([x[2] for x in rs]))
        else:
            r = orc.extract_batch(frames, **a)
        for x in r:
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _cache[key] = r
    return _cache[key]


def gpu_args(**kw):
    """(texfrac_bits, keywords of capi.Context.extract*) for the oracle keywords kw."""
    a = dict(ARGS, **kw)
    return a.pop("fracbits", 8), a


def octave_counts(counters, num_octaves):
    """(detections, second orientations) per octave, coarsest first, from one frame's 17 counters."""
    c = np.asarray(counters, np.int64)
    det = [int(c[2 * o] - c[2 * o - 1]) for o in range(1, num_octaves + 1)]
    dup = [int(c[2 * o + 1] - c[2 * o]) for o in range(1, num_octaves + 1)]
    return det, dup


def border_distance(recs, width=W, height=H):
    """Distance of every record from the nearest border of its octave's image, in texels of that octave."""
    sub = recs["subsampling"]
    k = np.log2(sub).astype(np.int64)
    x, y = recs["xpos"] / sub, recs["ypos"] / sub
    ow, oh = width >> k, height >> k
    return np.minimum(np.minimum(x, ow - 1 - x), np.minimum(y, oh - 1 - y))

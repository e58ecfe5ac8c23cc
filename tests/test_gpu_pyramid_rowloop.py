"""The row loops of the strip prefilter (lowpass_down_kernel), LowPass and ScaleDown, pixel for pixel against the oracle.

Batches of 5 frames (above small_frames = 4) take the strip kernels.  Every pyramid level of every frame is read back from
the caller's arena through misift_test_pyramid_layout, as tests/test_gpu_source_geometry.py does, and compared bit for
bit with oracle.pyoracle's chain lowpass -> scaledown -> ...  The shapes are chosen for the paths of the row loops:

  248 x 23    width % 4 == 0; two strips, the second one mostly halo; odd height; a one-row last segment
  244 x 64    width % 4 == 0; the image's edge falls beside the last quad of a strip; even height (the decimated row
              emitted behind the loop)
  484 x 137   width % 4 == 0; three strips; many segments: the decimation's warm-up rows of an inner segment
  323 x 70    ragged last quad (width % 4 == 3)
  64 x 18     narrower than a strip

At these sizes the launch geometry cuts a frame into 8-row segments: one turn of lowpass_down_kernel's nine-row loop and
two rows behind it, in strips that all hold an edge of the image.  The LONG cases go further: with the strip_waves knob at
1 and 13 frames a segment has 24 rows — 27 with the decimation's warm-up rows and the row behind the segment: three turns,
which start on rows of both parities; row 0 peeled and a six-row rest in the first segment — on a frame wide enough for a
strip that holds no image edge (the copy of the loop without the clamp selects) between two that do."""
import functools

import numpy as np
import pytest

import geometry_util as gu

pytestmark = pytest.mark.gpu

BLUR, THRESH, MAX_PTS = 1.0, 2.5, 4096
SHAPES = [(248, 23), (244, 64), (484, 137), (323, 70), (64, 18)]
U8_SHAPES = SHAPES[:2]
LONG = [(696, 150), (695, 151)]
NFRAMES_LONG, DISTINCT_LONG = 13, 3


def _noct(w, h):
    """The deepest pyramid of at most 3 levels that the merged-octave path accepts at this size (misift_tiny_call)."""
    for n in (3, 2):
        if w >= 16 and h >= 16 and (w >> (n - 1)) >= 8 and (h >> (n - 1)) >= 8:
            return n
    raise AssertionError((w, h))


@functools.lru_cache(maxsize=None)
def _oracle_pyramid(f, w, h, u8):
    return gu.oracle_pyramid(gu.crop(f, w, h, u8), _noct(w, h), BLUR)


def _pyramids(ctx, w, h, frame_ids, u8, fused):
    """One batch extraction of the frames; returns (pyramid levels per frame, launches)."""
    frames = np.stack([gu.crop(f, w, h, u8) for f in frame_ids])
    return gu.pyramids(ctx, frames, _noct(w, h), fused, BLUR, THRESH, MAX_PTS)


def _check_launches(calls, noct, fused):
    if fused:
        assert calls.get("lowpass_down") == 1 and "lowpass" not in calls, calls
        assert calls.get("scaledown", 0) == noct - 2, calls
    else:
        assert calls.get("lowpass") == 1 and "lowpass_down" not in calls, calls
        assert calls.get("scaledown", 0) == noct - 1, calls


def _check_pixels(pyr, w, h, frame_ids, u8, what):
    gu.check_pixels(pyr, [_oracle_pyramid(f, w, h, u8) for f in frame_ids], what)


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("w,h", SHAPES)
def test_rowloop_fp32(ctx, w, h, fused):
    ids = list(range(5))
    pyr, calls = _pyramids(ctx, w, h, ids, False, fused)
    _check_launches(calls, _noct(w, h), fused)
    _check_pixels(pyr, w, h, ids, False, "fp32/%dx%d/fused%d" % (w, h, fused))


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("w,h", U8_SHAPES)
def test_rowloop_u8(ctx, w, h, fused):
    ids = list(range(5))
    pyr, calls = _pyramids(ctx, w, h, ids, True, fused)
    _check_launches(calls, _noct(w, h), fused)
    _check_pixels(pyr, w, h, ids, True, "u8/%dx%d/fused%d" % (w, h, fused))


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("w,h", LONG)
def test_rowloop_long_segments(ctx, w, h, u8):
    """24-row segments (see the module docstring): 13 frames x 3 strips = 39 items per segment row against the 256
    wavefronts that strip_waves = 1 asks for give ceil(150 / 7) = 22 -> 24 rows."""
    ids = [f % DISTINCT_LONG for f in range(NFRAMES_LONG)]
    ctx.set_knob("strip_waves", 1)
    try:
        pyr, calls = _pyramids(ctx, w, h, ids, u8, 1)
    finally:
        ctx.set_knob("strip_waves", 32)        # the context's default
    _check_launches(calls, _noct(w, h), True)
    _check_pixels(pyr, w, h, ids, u8, "long/%dx%d/u8=%d" % (w, h, u8))

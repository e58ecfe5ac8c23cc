"""Host-only checks behind tests/test_gpu_source_geometry.py: the pyramid layout hook (misift_test_pyramid_layout)
against first principles, and the placement helper of tests/geometry_util.py against itself.  No GPU."""
import numpy as np
import pytest

import geometry_util as gu

SHAPES = [(w, h) for w in (320, 321, 322, 323) for h in (250, 251)] + [(1917, 1079), (16, 16)]


def _oracle_chain_shapes(w, h, noct, scale_up):
    """Shapes of the oracle's own chain, run on a blank image as long as a level has pixels to decimate."""
    from oracle import pyoracle as orc
    img = np.zeros((h, w), np.float32)
    if scale_up:
        img = orc.scaleup(img)
    img = orc.lowpass(img, 1.0)
    shapes = []
    for _ in range(noct):
        shapes.append((img.shape[1], img.shape[0]))
        img = orc.scaledown(img) if min(img.shape) >= 2 else np.zeros((img.shape[0] // 2, img.shape[1] // 2), np.float32)
    return shapes


@pytest.mark.parametrize("scale_up", [False, True])
@pytest.mark.parametrize("w,h", SHAPES)
def test_pyramid_layout(w, h, scale_up):
    from cudasift_amd import capi
    chain = _oracle_chain_shapes(w, h, 7, scale_up)
    assert chain == gu.oracle_shapes(w, h, 7, scale_up)
    for noct in range(1, 8):
        lay = capi.pyramid_layout(w, h, noct, scale_up)
        S = capi.scratch_floats(w, h, noct, scale_up)
        assert len(lay) == noct
        assert [(lw, lh) for _, lw, lh, _ in lay] == chain[:noct], (w, h, noct, scale_up)
        W, H = chain[0]
        # in front of the pyramid: the 8 planes of the finest level's DoG space (and the up-sampled frame under scale_up)
        assert lay[0][0] >= 8 * H * ((W + 127) // 128 * 128)
        end = lay[0][0]
        for off, lw, lh, lp in lay:
            assert lp % 128 == 0 and lw <= lp < lw + 128 or (lw == 0 and lp == 0), (lw, lp)
            assert off >= end, "levels overlap or are out of order"
            assert off % 4 == 0
            end = off + lh * lp
            assert end <= S, (off, lw, lh, lp, S)
        assert all(a[0] < b[0] for a, b in zip(lay, lay[1:]) if a[2] > 0)        # increasing wherever a level has rows


def test_pyramid_layout_rejects_bad_arguments():
    from cudasift_amd import capi
    L = capi.lib()
    o = np.zeros(8, np.int64)
    a, b, c = (np.zeros(8, np.int32) for _ in range(3))
    args = (o.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data)
    assert L.misift_test_pyramid_layout(320, 250, 4, 0, *args) == 0
    assert L.misift_test_pyramid_layout(320, 250, 0, 0, *args) != 0
    assert L.misift_test_pyramid_layout(320, 250, 8, 0, *args) != 0
    assert L.misift_test_pyramid_layout(0, 250, 4, 0, *args) != 0
    assert L.misift_test_pyramid_layout(320, 250, 4, 0, None, a.ctypes.data, b.ctypes.data, c.ctypes.data) != 0


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
@pytest.mark.parametrize("name", gu.BATCH + ("pitch128",))
@pytest.mark.parametrize("w", [320, 321, 322, 323])
def test_placement_round_trip(name, w, dtype):
    """Placing frames and reading them back through (base, pitch, stride) returns the frames; everything else in the
    buffer is the hostile fill, and the fill is what it claims to be."""
    h, B = gu.height_for(w), 1 if name in ("pitch128",) else 3
    rng = np.random.default_rng(w)
    frames = rng.integers(1, 255, (B, h, w)).astype(dtype)          # (never 0 / 255 / NaN: distinguishable from the fill)
    base, pitch, stride = gu.geometry(name, w, h)
    buf = gu.place(frames, base, pitch, stride)
    assert buf.dtype == frames.dtype and buf.ndim == 1
    assert gu.same_bytes(gu.read_back(buf, base, pitch, stride, B, h, w), frames)
    rest = gu.outside(buf, base, pitch, stride, B, h, w)
    assert len(rest) == len(buf) - frames.size
    if dtype is np.float32:
        assert np.isnan(rest).all() and (rest.view(np.uint32) == gu.NAN_BITS).all()
    else:
        assert set(np.unique(rest).tolist()) <= {0, 255}
    # the table's promises
    assert gu.source_aligned(name, w, h, B) == (name in ("roi", "padded", "pitch128") or (name == "tight" and w % 4 == 0))
    if name.startswith("roi") or name.startswith("oddstride"):
        # live (hostile) elements on all four sides of every frame
        for f in range(B):
            o = base + f * stride
            assert o - pitch >= 0 and o + h * pitch + w <= len(buf)
            for idx in (o - 1, o + w, o - pitch, o + h * pitch):
                v = buf[idx]
                assert np.isnan(v) if dtype is np.float32 else v in (0, 255), (name, f, idx)


def test_crops_are_the_issue_s_pixels():
    from synth import synth_frame
    c = gu.crop(2, 323, 251)
    assert gu.same_bytes(c, synth_frame(7, 704, 420)[7:258, 8:331])
    u = gu.crop(2, 323, 251, u8=True)
    assert u.dtype == np.uint8 and np.array_equal(u, np.clip(np.rint(c), 0, 255))
    assert np.isfinite(c).all()

"""Source geometries for the extraction and stage calls: frames placed inside a larger host buffer of hostile values at
(base, pitch, frame stride), the way a caller hands over a sub-rectangle of a parent image, an odd pitch, frames with a
gap between them, or a pool carved up at an offset.  Units are source elements (floats, or bytes for 8-bit frames).

"Aligned" below means a multiple of 4 elements — 16 bytes for fp32, 4 bytes for 8-bit — which is what the launchers
test when they choose between the vector-load kernels and the generic ones."""
import functools

import numpy as np

PARENT_W, PARENT_H = 704, 420        # the parent image of the roi geometries (pitch 704: a multiple of 4)
ROI_Y0, ROI_X0 = 7, 8                # crops start here: 7 * 704 + 8 is a multiple of 4
NAN_BITS = 0x7FC00000                # the fp32 fill: quiet NaN
SINGLE = ("tight", "roi", "roi+1", "roi+2", "roi+3", "oddpitch", "padded")
BATCH = SINGLE + ("oddstride+1", "oddstride+2")


def geometry(name, w, h):
    """(base, pitch, frame_stride) of a named geometry for w x h frames."""
    roi = ROI_Y0 * PARENT_W + ROI_X0
    if name == "tight":
        return 0, w, h * w
    if name == "roi":
        return roi, PARENT_W, PARENT_H * PARENT_W
    if name.startswith("roi+"):
        return roi + int(name[4:]), PARENT_W, PARENT_H * PARENT_W
    if name == "oddpitch":
        return 0, 701, PARENT_H * 701
    if name.startswith("oddstride+"):
        return roi, PARENT_W, PARENT_H * PARENT_W + int(name[10:])
    if name == "padded":
        p = (w + 3) // 4 * 4 + 4
        return 0, p, (h + 3) * p
    if name == "pitch128":                      # what capi.upload_image makes: the tight and aligned control
        p = (w + 127) // 128 * 128
        return 0, p, h * p
    raise KeyError(name)


def source_aligned(name, w, h, nframes=1):
    """True when every row of every frame starts on a multiple of 4 elements (the launchers' vector-path condition)."""
    base, pitch, stride = geometry(name, w, h)
    return base % 4 == 0 and pitch % 4 == 0 and (nframes == 1 or stride % 4 == 0)


def hostile(n, dtype):
    """n elements of fill: quiet NaN for fp32, a 0 / 255 checkerboard for 8-bit."""
    if np.dtype(dtype) == np.uint8:
        return (np.arange(n, dtype=np.int64) % 2 * 255).astype(np.uint8)
    return np.full(n, NAN_BITS, np.uint32).view(np.float32)


def buffer_elems(base, pitch, stride, nframes, h, w, slack=0):
    return max(base + (nframes - 1) * stride + (h - 1) * pitch + w, nframes * stride if nframes > 1 else 0) + slack


def _index(base, pitch, stride, nframes, h, w):
    f = np.arange(nframes, dtype=np.int64)[:, None, None] * stride
    y = np.arange(h, dtype=np.int64)[None, :, None] * pitch
    x = np.arange(w, dtype=np.int64)[None, None, :]
    return base + f + y + x


def place(frames, base, pitch, stride, total=None):
    """One host buffer of hostile values holding frames[f, y, x] at base + f * stride + y * pitch + x.  Frames must not
    overlap (asserted).  Returns the 1-D buffer of frames.dtype."""
    frames = np.asarray(frames)
    B, h, w = frames.shape
    assert pitch >= w and (B == 1 or stride >= (h - 1) * pitch + w), (pitch, stride, frames.shape)
    n = buffer_elems(base, pitch, stride, B, h, w) if total is None else total
    buf = hostile(n, frames.dtype)
    buf[_index(base, pitch, stride, B, h, w)] = frames
    return buf


def read_back(buf, base, pitch, stride, nframes, h, w):
    """The frames a reader of (base, pitch, stride) sees in `buf`."""
    return np.asarray(buf)[_index(base, pitch, stride, nframes, h, w)]


def outside(buf, base, pitch, stride, nframes, h, w):
    """The elements of `buf` that belong to no frame, in buffer order."""
    mask = np.ones(len(buf), bool)
    mask[_index(base, pitch, stride, nframes, h, w)] = False
    return np.asarray(buf)[mask]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _parent(seed):
    from synth import synth_frame
    return synth_frame(seed, PARENT_W, PARENT_H)


def crop(f, w, h, u8=False, seed=5):
    """Frame f of the test pixels: a w x h crop of synth_frame(seed + f, 704, 420) from row 7, column 8; for 8-bit
    sources clip(rint(.)) of the same crop."""
    c = np.ascontiguousarray(_parent(seed + f)[ROI_Y0:ROI_Y0 + h, ROI_X0:ROI_X0 + w])
    return np.clip(np.rint(c), 0, 255).astype(np.uint8) if u8 else c


def height_for(w):
    """Even widths go with height 250, odd ones with 251 (both parities of both axes appear)."""
    return 250 + (w & 1)


def oracle_shapes(w, h, num_octaves, scale_up):
    """(w, h) of the levels num_octaves ... 1 of the oracle's chain lowpass -> scaledown -> ... (scaleup first)."""
    if scale_up:
        w, h = 2 * w, 2 * h
    out = []
    for _ in range(num_octaves):
        out.append((w, h))
        w, h = w // 2, h // 2
    return out


# ---- pyramid levels read back from a call's arena (test_gpu_pyramid_rowloop.py, test_gpu_many_frames.py)

ARENA_POISON = 0x7FC0BAD1            # what the arena holds before the call


def oracle_pyramid(pix, noct, blur):
    """The levels noct ... 1 of the oracle's chain lowpass -> scaledown -> ... on one frame, finest first."""
    from oracle import pyoracle
    lvl = pyoracle.lowpass(np.asarray(pix).astype(np.float32), blur)
    pyr = [lvl]
    for _ in range(noct - 1):
        lvl = pyoracle.scaledown(lvl)
        pyr.append(lvl)
    return pyr


def pyramids(ctx, frames, noct, fused, blur, thresh, max_pts):
    """One batch extraction of frames [B, h, w] (uint8 or float32) placed at pitch128; returns (pyramid levels per
    frame, launches)."""
    from cudasift_amd import capi
    frames = np.asarray(frames)
    u8 = frames.dtype == np.uint8
    B, h, w = frames.shape
    base, pitch, stride = geometry("pitch128", w, h)
    host = place(frames, base, pitch, stride)
    src = ctx.upload(host)
    S = capi.scratch_floats(w, h, noct, False)
    arena = ctx.upload(np.full(S * B, ARENA_POISON, np.uint32))
    pts = ctx.zeros(576 * max_pts * B)
    saved = ctx.get_options().fused
    ctx.set_options(fused=fused)
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        rc, _ = ctx.extract_batch_raw(src.ptr, u8, B, stride, w, h, pitch, arena.ptr, pts.ptr, num_octaves=noct,
                                      init_blur=blur, thresh=thresh, max_pts=max_pts)
        ctx.sync()
        calls = {k: v["calls"] for k, v in ctx.profile_read().items()}
    finally:
        ctx.profile_enable(False)
        ctx.set_options(fused=saved)
    assert rc == 0, (rc, capi.lib().misift_last_error())
    fl = ctx.download(arena, (S * B,), np.uint32).view(np.float32)
    lay = capi.pyramid_layout(w, h, noct, False)
    return [[fl[f * S + off:f * S + off + lh * lp].reshape(lh, lp)[:, :lw] for off, lw, lh, lp in lay] for f in range(B)], calls


def check_pixels(pyr, want, what):
    """pyr[i]: the levels read back for frame i, want[i]: the oracle's; bit for bit."""
    assert len(pyr) == len(want)
    for i, levels in enumerate(want):
        assert len(pyr[i]) == len(levels)
        for lev, (got, ref) in enumerate(zip(pyr[i], levels)):
            assert got.shape == ref.shape, (what, i, lev, got.shape, ref.shape)
            if not same_bytes(got, ref):
                bad = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != ref.view(np.uint32))
                raise AssertionError("%s: frame %d pyramid level %d differs from the oracle at %d pixels, first (y, x) = %s, "
                                     "last %s" % (what, i, lev, len(bad), bad[0].tolist(), bad[-1].tolist()))

"""Batches of hundreds to a thousand small frames: what tests/test_many_frames_cpu.py and tests/test_gpu_many_frames.py
share.  The code these batches are for changes behaviour with the frame count alone — the block tables of a balanced
launch are built in rounds of 256 frames, the counts and offsets of the packed path in rounds of 1024, the segment
height of the streaming kernels reaches its clamp once frames x strips covers the machine — so the frames are as small
as the merged-octave path takes at three octaves, and few of them are distinct:

  POOL    seven frames of 96 x 72, synth_frame(7130 + i) at amplitudes SYNTH_AMP x (3, 0, 1, 0.5, 3, 1, 0): busy, flat,
          medium and nearly flat ones, so a batch is skewed and holds empty frames
  TALL    the same recipe at 96 x 136: taller than the 128-row clamp of a segment

The oracle finds 158, 0, 86, 2, 306, 42 and 0 records in the pool's frames (second orientations included; 1 - 7 ms a
frame), 388 / 147 / 2 / 688 / 59 in their 8-bit forms under scale_up, and up to 567 in the tall ones.  (Seed 7000 gave
no frame with a handful of records: 281, 0, 47, 0, 264, 37, 0.)

Frame f of a batch is pool frame f % 7.  Seven is prime: the frames on either side of 256, 512 and 1024 differ, so a
table, count or offset that lands one round too early or too late holds another frame's figure.

A plain module: no fixtures, no hooks; cudasift_amd and the oracle are imported inside the functions."""
import functools

import numpy as np

from synth import SYNTH_AMP, synth_frame

W, H, TALL_H = 96, 72, 136
NOCT, BLUR, THRESH, MAX_PTS = 3, 1.0, 2.0, 512
SEED = 7130
AMPS = (3.0, 0.0, 1.0, 0.5, 3.0, 1.0, 0.0)
NPOOL = len(AMPS)
POOL = np.stack([synth_frame(SEED + i, W, H, amp=SYNTH_AMP * a) for i, a in enumerate(AMPS)])
TALL = np.stack([synth_frame(SEED + i, W, TALL_H, amp=SYNTH_AMP * a) for i, a in enumerate(AMPS)])
POOL.setflags(write=False)
TALL.setflags(write=False)

# the frame counts of the GPU tests and what each is for
SHARE_ROUND, COUNT_ROUND = 256, 1024          # frames per round of frame_shares_body / of export_counts_kernel
TABLE_BATCHES = (257, 600, 1030)              # two, three and five rounds of 256
PACKED_BATCHES = (1024, 1025, 1030)           # exactly one round of 1024, one frame into the second, six frames into it
PIPE_BATCHES = (1030, 1025)                   # the pipe's batch size, then a ragged batch
USED_CONTEXT = (5, 1030, 5, 257, 1025)        # frame counts of one context, call after call (the last one packed)
LARGE_FIRST = (1030, 5, 257, 5, 1025)         # ... and with the large call first
TALL_BATCH = 257                              # tall segments: the clamp needs frames x strips >= CUs (see strip_geom)
SCALE_UP_MAX_PTS = 1024                       # the 8-bit frames doubled first hold up to 688 records
# knob defaults restated (misift_host.hip, ctx_init): workgroups per CU of orient_all and descr_all, the floor of
# workgroups per frame, the cap of a batch, and the largest "frame or two" batch
ORIENT_BLOCKS, POINT_BLOCKS, MIN_BLOCKS_PER_FRAME, MAX_BLOCKS_PER_FRAME, SMALL_FRAMES = 6, 8, 8, 512, 4
STRIP_WAVES_DEFAULT = 32
PREFILTER_LANES, STREAM_LANES = 60, 62        # quads per strip of the fused prefilter / of LowPass and ScaleDown


def pool(tall=False, u8=False):
    """The seven frames; u8: clip(rint(.)) of them, as 8-bit."""
    p = TALL if tall else POOL
    return np.clip(np.rint(p), 0, 255).astype(np.uint8) if u8 else p


def batch(nframes, tall=False, u8=False):
    """[nframes, h, w]: frame f is pool frame f % 7."""
    return np.ascontiguousarray(pool(tall, u8)[np.arange(nframes) % NPOOL])


def rounds(nframes, per_round):
    return (nframes + per_round - 1) // per_round


def orc():
    from oracle import pyoracle
    return pyoracle


@functools.lru_cache(maxsize=None)
def expected(pool_index, tall=False, u8=False, scale_up=False, max_pts=MAX_PTS):
    """The oracle's (records[max_pts], numPts, counters[17]) of one pool frame.  Cached: do not write to them."""
    img = pool(tall, u8)[pool_index].astype(np.float32)
    recs, n, cnt = orc().extract(img, num_octaves=NOCT, init_blur=BLUR, thresh=THRESH, scale_up=scale_up, max_pts=max_pts)
    recs.setflags(write=False)
    cnt.setflags(write=False)
    return recs, int(n), cnt


def written(counters):
    """Records a call writes for a frame: the last octave's total with its second orientations (counter 2 * noct + 1)."""
    return int(counters[2 * NOCT + 1])


def detections(counters, max_pts=MAX_PTS):
    """n_f of the share rule: the sum over the octaves of min(detections, max_pts), from a frame's 17 counters."""
    c = [int(v) for v in counters]
    return sum(min(c[2 * o] - c[2 * o - 1], max_pts) for o in range(1, NOCT + 1))


def counts_of(nframes, **kw):
    """(numPts, written, n_f) of every frame of a batch, as int64 arrays."""
    per = [expected(i, **kw) for i in range(NPOOL)]
    idx = np.arange(nframes) % NPOOL
    mp = kw.get("max_pts", MAX_PTS)
    return (np.array([per[i][1] for i in idx], np.int64), np.array([written(per[i][2]) for i in idx], np.int64),
            np.array([detections(per[i][2], mp) for i in idx], np.int64))


def canon(records):
    """Records of one frame in a canonical order, as bytes (appends within an octave are atomic, so the order varies)."""
    k = [np.ascontiguousarray(records[f]).view(np.uint32) for f in ("orientation", "scale", "ypos", "xpos")]
    return records[np.lexsort(k)].tobytes()


def grid_x(num_cus, blocks_per_cu, nframes):
    """points_grid_x restated: workgroups per frame of a per-keypoint launch over a batch."""
    per_frame = (num_cus * blocks_per_cu + nframes - 1) // nframes
    cap = 1024 if nframes <= SMALL_FRAMES else MAX_BLOCKS_PER_FRAME
    return min(max(per_frame, MIN_BLOCKS_PER_FRAME), cap)


def table_sizes(num_cus, nframes):
    """(rows of orient_all's block table, rows of descr_all's) of a balanced batch."""
    return grid_x(num_cus, ORIENT_BLOCKS, nframes) * nframes, grid_x(num_cus, POINT_BLOCKS, nframes) * nframes


def block_tables(counts, T):
    """The table a balanced launch of T workgroups must hold for frames with counts[f] keypoints, [T, 4] int32: frame f
    gets share(f) = 1 + (T - B) * n_f // sum(n) workgroups (1 when the sum is 0), rows (f, k, share, 0) for k = 0 ..
    share - 1, frame after frame; the remaining rows are (-1, 0, 0, 0)."""
    counts = [int(c) for c in counts]
    B, total = len(counts), sum(counts)
    assert T >= B
    rows = np.zeros((T, 4), np.int32)
    rows[:, 0] = -1
    at = 0
    for f, n in enumerate(counts):
        share = 1 + ((T - B) * n // total if total else 0)
        rows[at:at + share, 0] = f
        rows[at:at + share, 1] = np.arange(share)
        rows[at:at + share, 2] = share
        at += share
    assert at <= T
    return rows


def shares_of(table, nframes):
    """The share of every frame as a table states it (column 2 of the frame's first row), for the host hook's answer."""
    first = np.flatnonzero(table[:, 1] == 0)
    first = first[table[first, 0] >= 0]
    assert np.array_equal(table[first, 0], np.arange(nframes))
    return table[first, 2]


def strip_geom(num_cus, strip_waves, small_frames, out_w, out_rows, out_lanes, nframes, strip_rows_small=6):
    """make_geom restated: (nstrips, seg_rows, nsegs) of a streaming launch that writes out_w x out_rows pixels per
    frame, out_lanes quads per strip."""
    nquads = (out_w + 3) // 4
    nstrips = max((nquads + out_lanes - 1) // out_lanes, 1)
    target = num_cus * strip_waves
    want = max((target + nframes * nstrips - 1) // (nframes * nstrips), 1)
    seg = (out_rows + want - 1) // want
    if nframes <= small_frames:
        seg = max((seg + 1) // 2 * 2, strip_rows_small)
    else:
        seg = max((seg + 7) // 8 * 8, 8)
    seg = min(seg, 128)
    return nstrips, seg, max((out_rows + seg - 1) // seg, 1)


def smallest_batch_with(num_cus, strip_waves, out_w, out_rows, out_lanes, seg_rows, nsegs, at_least=SHARE_ROUND + 1):
    """The smallest frame count >= at_least at which strip_geom gives these seg_rows and nsegs (None: none up to 4096)."""
    for b in range(at_least, 4097):
        if strip_geom(num_cus, strip_waves, SMALL_FRAMES, out_w, out_rows, out_lanes, b)[1:] == (seg_rows, nsegs):
            return b
    return None

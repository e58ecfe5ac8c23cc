"""misift_match_pairs_batch_i8 at the size README and bench.py report: one 100 000 x 100 000 pair with max_pts = 100 000,
on the descriptors and planted duplicate columns of test_gpu_match_full_size.py, every output byte checked against the
oracle's blocked core on the quantised descriptors (integer products sum to < 2^24, so its fp32 chain is exact; never a
dense 100k x 100k numpy matrix).

At this size the call takes the int8 plan no smaller case reaches: 6 column chunks of 521 tiles, each crossing a
512-tile key window, and 782 row blocks feeding every column key.  Set 2 holds exact duplicate columns on both sides of
the chunk and key-window edges, and the oracle confirms, before the GPU runs, that rows really have such a tie as their
best and that the cross-check both keeps and rejects rows."""
import numpy as np
import pytest

from batch_util import MATCH_FIELDS, i8_records, quantize_np, same_rows
from synth import descriptors_to_points, synth_descriptors
from test_gpu_match_full_size import EDGES, I8_PLAN, N, _pair_plan, _plant

pytestmark = pytest.mark.gpu

OUT_FIELDS = ("xpos", "ypos") + MATCH_FIELDS
I8_EDGES = EDGES["i8 window"] + EDGES["i8 chunk"]
POISON = 0xA5


@pytest.fixture(scope="module")
def full8():
    from cudasift_amd import capi
    from oracle import pyoracle as orc
    d1, d2 = synth_descriptors(N, 12345), synth_descriptors(N, 12346)
    _plant(d2)
    p1, p2 = descriptors_to_points(d1, capi.POINT_DTYPE), descriptors_to_points(d2, capi.POINT_DTYPE)
    q1, q2 = quantize_np(d1), quantize_np(d2)
    core = orc.match_core(q1.astype(np.float32), q2.astype(np.float32), columns=True)
    return dict(p1=p1, p2=p2, q1=q1, q2=q2, core=core, exp=i8_records(p1, p2, core))


def _expected(full8, mutual):
    exp = full8["exp"].copy()
    if mutual:
        m = exp["match"]
        rej = (m >= 0) & (full8["core"]["col_row"][np.maximum(m, 0)] != np.arange(N))
        for k in MATCH_FIELDS:
            exp[k][rej] = 0
        exp["match"][rej] = -1
    return exp


@pytest.mark.parametrize("mutual", [0, 1])
def test_match_pairs_batch_i8(ctx, full8, mutual):
    """All seven fields of all rows, the count, d_num_matched, untouched output bytes and untouched inputs."""
    from cudasift_amd import capi
    assert _pair_plan("misift_test_match_i8_plan") == I8_PLAN == [0, 782, 3125, 6, 521]
    chunks, tpc = I8_PLAN[3], I8_PLAN[4]
    for e in EDGES["i8 chunk"]:
        assert e % (32 * tpc) == 0 and 0 < e // (32 * tpc) < chunks
    for e in EDGES["i8 window"]:
        assert (e // 32) % tpc == 512                            # key windows restart at each chunk's first tile
    core = full8["core"]
    assert np.array_equal(full8["q2"][np.array(I8_EDGES) - 1], full8["q2"][np.array(I8_EDGES)])
    for e in I8_EDGES:
        tie = (core["ex_idx"] == e - 1) & (core["ex_sec"] == core["ex_best"])
        assert tie.any(), e                                      # rows whose best is the duplicate left of the edge
        assert not (core["ex_idx"] == e).any(), e
        assert core["col_row"][e - 1] == core["col_row"][e] >= 0
    m = core["ex_idx"]
    kept = (m >= 0) & (core["col_row"][np.maximum(m, 0)] == np.arange(N))
    assert 0 < kept.sum() < (m >= 0).sum()
    exp = _expected(full8, mutual)
    assert int((exp["match"] >= 0).sum()) == (int(kept.sum()) if mutual else int((m >= 0).sum()))

    recs = np.concatenate([full8["p1"], full8["p2"]])
    q = np.concatenate([full8["q1"], full8["q2"]])
    d, dq = ctx.upload(recs), ctx.upload(q)
    dc, do = ctx.upload(np.array([N, N], np.int32)), ctx.upload(np.array([0, N], np.int32))
    out = ctx.upload(np.full(N * 576, POISON, np.uint8))
    oc, nm = ctx.upload(np.full(1, -7, np.int32)), ctx.upload(np.full(1, -7, np.int32))
    ctx.match_pairs_batch_i8([(0, 1)], d, dq, 2, dc, do, 0, max_pts=N, mutual=mutual, out=out, out_counts=oc,
                             num_matched=nm)
    ctx.sync()
    got = ctx.download(out, (N,), capi.POINT_DTYPE)
    same_rows(got, exp, "misift_match_pairs_batch_i8", OUT_FIELDS)
    raw = got.view(np.uint8).reshape(N, 576).copy()
    for k in OUT_FIELDS:
        off = capi.POINT_DTYPE.fields[k][1]
        raw[:, off:off + 4] = POISON
    assert (raw == POISON).all(), "bytes outside the output fields written"
    assert ctx.download(oc, (1,), np.int32)[0] == N
    assert ctx.download(nm, (1,), np.int32)[0] == int((exp["match"] >= 0).sum())
    assert ctx.download(d, (2 * N,), capi.POINT_DTYPE).tobytes() == recs.tobytes(), "records written"
    assert ctx.download(dq, (2 * N, 128), np.int8).tobytes() == q.tobytes(), "q written"

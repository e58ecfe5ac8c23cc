"""Every matcher at the size README and bench.py report: 100 000 x 100 000 descriptors of bench.py's recipe
(synth_descriptors, seeds 12345 / 12346), every output byte checked against the oracle's blocked core (orc_match_core:
the dot128 chain per pair, so the check is bit-exact; near-ties are common at this size).

At full size the kernels take plans no smaller case reaches (17 column chunks of 92 super-tiles, 26 of 61 for a
12 500-row shard, the int8 call's 6 chunks of 521 tiles that each cross a 512-tile key window, the loopback split at
multiples of 12 500): each test asserts its plan first, so a changed plan shows.  Set 2 holds exact duplicate columns
on both sides of chunk, key-window and shard edges, and the oracle confirms that rows really have such a tie as their
best: a merge that loses a chunk or resolves a tie to the larger column fails here."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from batch_util import MATCH_FIELDS, i8_records, num_cus, quantize_np, same_rows
from synth import descriptors_to_points, synth_descriptors

pytestmark = pytest.mark.gpu

N = 100000
NUM_CUS = 256
OUT_FIELDS = ("xpos", "ypos") + MATCH_FIELDS
ROW0, NROWS = 50001, 12512              # misift_match_rows: starts inside a 128-row block
WORLD, SHARD = 8, N // 8
# (chunks, super-tiles per chunk, super-tiles) of misift_match on NUM_CUS CUs
MATCH_PLANS = {N: (17, 92, 1563), NROWS: (26, 61, 1563), SHARD: (26, 61, 1563)}
BATCH_PLAN = [0, 782, 1563, 1, 1563]    # first item, row blocks, tiles, chunks, tiles per chunk (64-column tiles)
I8_PLAN = [0, 782, 3125, 6, 521]        # the same with 32-column tiles
# column E: set 2 holds one descriptor at E - 1 and E
EDGES = {
    "fp32 chunk": [64 * 92, 64 * 92 * 16],                   # misift_match's first and last chunk edges
    "rows chunk": [64 * 61 * 13],                            # a chunk edge of the 12 512-row and 12 500-row plans
    "i8 window": [32 * 512, 32 * (521 * 5 + 512)],           # key windows restart at each chunk's first tile
    "i8 chunk": [32 * 521 * 3],
    "shard": [SHARD, SHARD * 5, SHARD * 7],
}


def _plant(d2):
    """Copy the strongest columns (largest norm: they win most rows) onto both sides of every edge; the source column
    takes the edge's old left column, so the two copies are the only ones."""
    edges = sorted(e for v in EDGES.values() for e in v)
    near = set(j for e in edges for j in (e - 1, e))
    order = [j for j in np.argsort(-np.linalg.norm(d2.astype(np.float64), axis=1), kind="stable") if j not in near]
    for e, s in zip(edges, order):
        v = d2[s].copy()
        d2[s] = d2[e - 1]
        d2[e - 1] = v
        d2[e] = v
    return edges


@pytest.fixture(scope="module")
def full():
    from cudasift_amd import capi
    from oracle import pyoracle as orc
    d1, d2 = synth_descriptors(N, 12345), synth_descriptors(N, 12346)
    edges = _plant(d2)
    p1, p2 = descriptors_to_points(d1, capi.POINT_DTYPE), descriptors_to_points(d2, capi.POINT_DTYPE)
    core = orc.match_core(d1, d2)
    q1, q2 = quantize_np(d1), quantize_np(d2)
    core8 = orc.match_core(q1.astype(np.float32), q2.astype(np.float32), columns=False)
    return dict(p1=p1, p2=p2, edges=edges, core=core, core8=core8, q1=q1, q2=q2,
                exp={ex: orc.match_records(p1, p2, core, ex) for ex in (False, True)},
                exp8=i8_records(p1, p2, core8))


class _mode:
    """The context's match options for one call, restored afterwards."""

    def __init__(self, ctx, exact):
        self.ctx, self.exact = ctx, exact

    def __enter__(self):
        o = self.ctx.get_options()
        self.saved = (o.match_full, o.match_exact_top2)
        self.ctx.set_options(match_full=int(self.exact), match_exact_top2=int(self.exact))

    def __exit__(self, *exc):
        self.ctx.set_options(match_full=self.saved[0], match_exact_top2=self.saved[1])
        return False


def _match_plan(n1, n2):
    from cudasift_amd import capi
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    capi.check(capi.lib().misift_test_match_plan(num_cus(), n1, n2, C.byref(a), C.byref(b), C.byref(c)),
               "misift_test_match_plan")
    return a.value, b.value, c.value


def _pair_plan(hook, *lead):
    from cudasift_amd import capi
    n = np.array([N], np.int32)
    plan, ni, ch, pb = np.zeros(5, np.int32), C.c_int(), C.c_int(), C.c_int()
    capi.check(getattr(capi.lib(), hook)(num_cus(), *lead, 1, n.ctypes.data, n.ctypes.data, plan.ctypes.data,
                                         C.byref(ni), C.byref(ch), C.byref(pb)), hook)
    return plan.tolist()


def test_plans_and_planted_ties(full):
    """The plans the calls below take, and the ties they meet: for every planted edge some rows' best (reference mode,
    full + exact, int8) is the duplicate left of the edge, with a runner-up of the same score; the mutual check both
    keeps and rejects rows."""
    assert num_cus() == NUM_CUS
    for n1, plan in MATCH_PLANS.items():
        assert _match_plan(n1, N) == plan, n1
        ch, tpc, _ = plan
        assert all(e % (64 * tpc) == 0 and e // (64 * tpc) < ch for e in EDGES["fp32 chunk" if n1 == N else "rows chunk"])
    for full_cols in (0, 1):
        assert _pair_plan("misift_test_match_batch_plan", full_cols) == BATCH_PLAN
    assert _pair_plan("misift_test_match_i8_plan") == I8_PLAN
    core, core8 = full["core"], full["core8"]
    for kind, edges in EDGES.items():
        for e in edges:
            # exact top-2: the smaller column wins a tie; the reference mode's class merge (matching.cu:375-390) prefers
            # the lower class, (column % 32) / 4, which is column e's when e is a multiple of 32
            cls_win = e if e % 32 == 0 else e - 1
            for what, c, pre, win in (("fp32 reference", core, "cls_", cls_win), ("fp32 exact", core, "ex_", e - 1),
                                      ("int8", core8, "ex_", e - 1)):
                tie = (c[pre + "idx"] == win) & (c[pre + "sec"] == c[pre + "best"])
                assert tie.any() or (what == "int8" and not kind.startswith("i8")), (kind, e, what)
                assert not (c[pre + "idx"] == 2 * e - 1 - win).any(), (kind, e, what)
            assert core["col_row"][e - 1] == core["col_row"][e] >= 0
    m = core["cls_idx"]
    kept = (m >= 0) & (core["col_row"][np.maximum(m, 0)] == np.arange(N))
    assert 0 < kept.sum() < (m >= 0).sum()


@pytest.mark.parametrize("exact", [False, True], ids=["reference", "full_exact"])
def test_match(ctx, full, exact):
    """misift_match, 100 000 x 100 000: every byte of every record."""
    assert _match_plan(N, N) == MATCH_PLANS[N]
    with _mode(ctx, exact):
        got = ctx.match(full["p1"], N, full["p2"], N)
    same_rows(got, full["exp"][exact], "misift_match")


@pytest.mark.parametrize("exact", [False, True], ids=["reference", "full_exact"])
def test_match_rows(ctx, full, exact):
    """misift_match_rows for 12 512 rows from row 50 001: those rows matched, every other record untouched."""
    assert _match_plan(NROWS, N) == MATCH_PLANS[NROWS]
    with _mode(ctx, exact):
        got = ctx.match(full["p1"], N, full["p2"], N, row_begin=ROW0, row_count=NROWS)
    exp = full["p1"].copy()
    exp[ROW0:ROW0 + NROWS] = full["exp"][exact][ROW0:ROW0 + NROWS]
    same_rows(got, exp, "misift_match_rows")


def _pair_set(ctx, full):
    recs = np.concatenate([full["p1"], full["p2"]])
    return recs, ctx.upload(recs), ctx.upload(np.array([N, N], np.int32)), ctx.upload(np.array([0, N], np.int32))


@pytest.mark.parametrize("exact", [False, True], ids=["reference", "full_exact"])
def test_match_batch(ctx, full, exact):
    """misift_match_batch, one 100 000 x 100 000 pair of a packed batch: frame 0 matched, frame 1 untouched."""
    from cudasift_amd import capi
    assert _pair_plan("misift_test_match_batch_plan", int(exact)) == BATCH_PLAN
    recs, d, dc, do = _pair_set(ctx, full)
    with _mode(ctx, exact):
        ctx.match_batch([(0, 1)], d, 2, dc, do, 0)
        ctx.sync()
    got = ctx.download(d, (2 * N,), capi.POINT_DTYPE)
    same_rows(got[:N], full["exp"][exact], "misift_match_batch")
    same_rows(got[N:], full["p2"], "set 2")


@pytest.mark.parametrize("exact", [False, True], ids=["reference", "full_exact"])
@pytest.mark.parametrize("mutual", [0, 1])
def test_match_pairs_batch(ctx, full, exact, mutual):
    """misift_match_pairs_batch with max_pts = 100 000: the seven output fields of every row, the counts, and no other
    byte written; with mutual a row keeps its match only if the oracle's best row of that column is the row."""
    from cudasift_amd import capi
    assert _pair_plan("misift_test_match_batch_plan", int(exact)) == BATCH_PLAN
    recs, d, dc, do = _pair_set(ctx, full)
    poison = 0xA5
    out = ctx.upload(np.full(N * 576, poison, np.uint8))
    oc, nm = ctx.upload(np.full(1, -7, np.int32)), ctx.upload(np.full(1, -7, np.int32))
    with _mode(ctx, exact):
        ctx.match_pairs_batch([(0, 1)], d, 2, dc, do, 0, max_pts=N, mutual=mutual, out=out, out_counts=oc,
                              num_matched=nm)
        ctx.sync()
    got = ctx.download(out, (N,), capi.POINT_DTYPE)
    exp = full["exp"][exact].copy()
    if mutual:
        m = exp["match"]
        rej = (m >= 0) & (full["core"]["col_row"][np.maximum(m, 0)] != np.arange(N))
        for k in MATCH_FIELDS:
            exp[k][rej] = 0
        exp["match"][rej] = -1
    same_rows(got, exp, "misift_match_pairs_batch", OUT_FIELDS)
    raw = got.view(np.uint8).reshape(N, 576).copy()
    for k in OUT_FIELDS:
        off = capi.POINT_DTYPE.fields[k][1]
        raw[:, off:off + 4] = poison
    assert (raw == poison).all(), "bytes outside the output fields written"
    assert ctx.download(oc, (1,), np.int32)[0] == N
    assert ctx.download(nm, (1,), np.int32)[0] == int((exp["match"] >= 0).sum())
    assert ctx.download(d, (2 * N,), capi.POINT_DTYPE).tobytes() == recs.tobytes(), "input written"


def test_match_batch_i8(ctx, full):
    """misift_quantize_batch + misift_match_batch_i8, one 100 000 x 100 000 pair: every q byte, every record."""
    from cudasift_amd import capi
    assert _pair_plan("misift_test_match_i8_plan") == I8_PLAN
    recs, d, dc, do = _pair_set(ctx, full)
    dq = ctx.upload(np.full((2 * N, 128), 0x5A, np.int8))
    ctx.quantize_batch(d, 2, dc, do, 0, dq)
    ctx.sync()
    q = ctx.download(dq, (2 * N, 128), np.int8)
    assert np.array_equal(q[:N], full["q1"]) and np.array_equal(q[N:], full["q2"])
    ctx.match_batch_i8([(0, 1)], d, dq, 2, dc, do, 0)
    ctx.sync()
    got = ctx.download(d, (2 * N,), capi.POINT_DTYPE)
    same_rows(got[:N], full["exp8"], "misift_match_batch_i8")
    same_rows(got[N:], full["p2"], "set 2")


def _rank(capi, rank, lw, full, out, errs):
    try:
        c = capi.Context(0)
        comm = capi.Comm(c, WORLD, rank, lw)
        rows = slice(rank * SHARD, (rank + 1) * SHARD)
        d1, d2 = c.upload(full["p1"][rows]), c.upload(full["p2"][rows])
        all2, res = c.zeros(576 * N), c.zeros(12 * N)
        comm.match_sharded(d1.ptr, SHARD, d2.ptr, SHARD, all2.ptr, res.ptr)
        out[rank] = (c.download(d1, (SHARD,), capi.POINT_DTYPE), c.download(res, (N,), capi.RESULT_DTYPE))
        comm.close()
        c.close()
    except Exception as e:                         # noqa: BLE001
        import traceback
        errs.append("rank %d: %s\n%s" % (rank, e, traceback.format_exc()))


@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "no_overlap"])
def test_match_sharded_loopback(ctx, full, overlap):
    """misift_match_sharded on a loopback world of 8: 12 500 rows and a 12 500-column shard per rank; every rank's
    rows and the all-gathered 12-byte results of all 100 000 rows (reference mode)."""
    from cudasift_amd import capi
    assert _match_plan(SHARD, N) == MATCH_PLANS[SHARD]
    if not overlap:
        os.environ["MISIFT_MATCH_NO_OVERLAP"] = "1"
    try:
        lw = capi.LoopbackWorld(WORLD)
        out, errs = {}, []
        ts = [threading.Thread(target=_rank, args=(capi, r, lw, full, out, errs)) for r in range(WORLD)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=300)
    finally:
        os.environ.pop("MISIFT_MATCH_NO_OVERLAP", None)
    assert not any(t.is_alive() for t in ts), "a loopback rank is stuck"
    assert not errs, "\n".join(errs)
    lw.close()
    exp = full["exp"][False]
    for r in range(WORLD):
        rows, res = out[r]
        same_rows(rows, exp[r * SHARD:(r + 1) * SHARD], "rank %d rows" % r)
        same_rows(res, exp, "rank %d results" % r, ("score", "ambiguity", "match"))


@pytest.mark.parametrize("exact", [False, True], ids=["reference", "full_exact"])
def test_match_l2_sample(ctx, exact):
    """misift_match on the L2-normalised sets at 100 000 x 100 000: 2048 rows in four windows (first, two inside,
    last row block) against orc.match_rows."""
    from cudasift_amd import capi
    from oracle import pyoracle as orc
    p1 = descriptors_to_points(synth_descriptors(N, 12345, l2=True), capi.POINT_DTYPE)
    p2 = descriptors_to_points(synth_descriptors(N, 12346, l2=True), capi.POINT_DTYPE)
    with _mode(ctx, exact):
        got = ctx.match(p1, N, p2, N)
    for r0 in (0, 31000, 64001, N - 512):
        exp = p1.copy()
        orc.match_rows(exp, r0, 512, p2, N, full=exact, exact=exact)
        same_rows(got[r0:r0 + 512], exp[r0:r0 + 512], "L2 rows %d.." % r0)

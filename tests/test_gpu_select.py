"""misift_select_pairs_batch on the device, held byte for byte to the numpy restatement of select_cases.py (which
test_select_cpu.py holds to the host hook and to a brute force): all six outputs at exactly their stated sizes on
poisoned buffers, the inputs unwritten, on a guarded context; the argument errors; a context other calls have used; V
against the device's own pair matcher; and the chain quantize -> select -> read the pairs -> match -> link."""
import numpy as np
import pytest

import select_cases as SC
import used_context as U
from batch_util import OUT_FIELDS, POISON_WORD, guarded_context, num_cus

pytestmark = pytest.mark.gpu

EINVAL = -1
INPUTS = ("recs", "q", "counts", "offs")


@pytest.fixture(scope="module")
def gctx():
    with guarded_context(1) as g:
        yield g


sizes_of, tmp_bytes, SelectStep = U.select_sizes, U.select_tmp_bytes, U.SelectStep         # in the form of used_context.py


def upload(ctx, case):
    dev = {k: ctx.upload(case[k]) for k in INPUTS if case[k] is not None}
    dev["offs"] = dev.get("offs")
    for k, words in sizes_of(case).items():
        dev[k] = ctx.upload(U.poisoned(words))
    return dev


def enqueue(ctx, case, dev):
    ctx.select_pairs_batch(dev["recs"], dev["q"], len(case["counts"]), dev["counts"], dev["offs"], case["stride"],
                           **{k: case[k] for k in SC.ARGS}, **{k: dev[k] for k in SC.OUTPUTS})


def download(ctx, case, dev):
    got = {k: ctx.download(dev[k], (max(w, 1),), np.int32) for k, w in sizes_of(case).items()}
    for k in INPUTS:
        if case[k] is not None:
            back = ctx.download(dev[k], (case[k].nbytes,), np.uint8)
            assert back.tobytes() == np.ascontiguousarray(case[k]).tobytes(), "input %s was written" % k
    return got


def same(got, exp, what):
    for k in SC.OUTPUTS:
        bad = np.nonzero(got[k] != exp[k])[0]
        assert len(bad) == 0, "%s: %s differs in %d words, first %s: got %s, expected %s" % (
            what, k, len(bad), bad[:6], got[k][bad[:6]], exp[k][bad[:6]])


def run(ctx, case):
    dev = upload(ctx, case)
    enqueue(ctx, case, dev)
    return download(ctx, case, dev)


@pytest.mark.parametrize("name", sorted(SC.all_cases()))
def test_every_case_byte_for_byte(gctx, name):
    case = SC.all_cases()[name]
    same(run(gctx, case), SC.expected(case), name)


def test_two_runs_give_the_same_bytes(gctx):
    for name in ("sizes_top256", "strips_100", "duplicates"):
        case = SC.all_cases()[name]
        a, b = run(gctx, case), run(gctx, case)
        for k in SC.OUTPUTS:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


def test_guards_stay_intact_at_the_largest_shapes():
    """A context of its own: the temp is allocated for these shapes and no other, so a write past it meets a band."""
    from cudasift_amd import capi
    for name in ("sizes_top256", "frames_65_top33", "strips_100", "sizes_top1"):
        with guarded_context(1) as g:
            case = SC.all_cases()[name]
            same(run(g, case), SC.expected(case), name)
            assert g.test_state(0) == tmp_bytes(case)
            capi.check_guards()


# ---- a context other calls have used

def test_on_a_context_other_calls_have_used():
    """Between calls that leave the shared temp full of their own partials, keys and labels: large, small, large again,
    nothing read until all are enqueued; the temp holds what each call predicts."""
    sel, ncu = SelectStep(), num_cus()
    others = [U.step("match_pairs_batch_i8"), U.step("link_tracks_batch"), U.step("export_tracks_batch")]
    plan = [(others[0], "large"), (sel, "large"), (others[1], "large"), (sel, "small"), (others[2], "small"),
            (others[0], "small"), (sel, "large"), (sel, "small")]
    with guarded_context(1) as g:
        bufs = [U.Bufs(g, s, size) for s, size in plan]
        tmp = g.test_state(0)
        for b in bufs:
            b.enqueue()
            now = g.test_state(0)
            assert now == max(tmp, b.step.tmp_bytes(b.case, ncu)), (b.step.name, b.size, tmp, now)
            tmp = now
        for i, b in enumerate(bufs):
            b.check("call %d" % i)


# ---- argument errors

def test_argument_errors_enqueue_nothing(gctx):
    from cudasift_amd import capi
    L = capi.lib()
    case = SC.all_cases()["ring_small"]
    padded = SC.all_cases()["votes"]
    for c in (case, padded):
        dev = upload(gctx, c)
        n = len(c["counts"])
        base = dict(ctx=gctx.h, recs=dev["recs"].ptr, q=dev["q"].ptr, nframes=n, counts=dev["counts"].ptr,
                    offs=dev["offs"].ptr if dev["offs"] else None, stride=c["stride"], top=c["top"],
                    min_score=c["min_score"], max_ambiguity=c["max_ambiguity"], min_votes=c["min_votes"], k=c["k"],
                    max_pairs=c["max_pairs"], **{k: dev[k].ptr for k in SC.OUTPUTS})
        order = ("ctx", "recs", "q", "nframes", "counts", "offs", "stride") + SC.ARGS + SC.OUTPUTS

        def call(**kw):
            a = dict(base, **kw)
            return L.misift_select_pairs_batch(*[a[k] for k in order])

        bad = [dict(ctx=None), dict(recs=None), dict(q=None), dict(counts=None)]
        bad += [{k: None} for k in SC.OUTPUTS]
        bad += [dict(q=dev["q"].ptr + 8), dict(nframes=-1), dict(nframes=SC.MAX_FRAMES + 1), dict(top=0),
                dict(top=SC.MAX_TOP + 1), dict(k=0), dict(min_votes=0), dict(max_pairs=-1),
                dict(min_score=float("nan")), dict(max_ambiguity=float("nan")), dict(offs=None, stride=-1)]
        # every output on every other output, at its start and on its last word
        w = sizes_of(c)
        for a in SC.OUTPUTS:
            for b in SC.OUTPUTS:
                if a != b and w[a] and w[b]:
                    bad += [{a: dev[b].ptr}, {a: dev[b].ptr + 4 * (w[b] - 1)}]
        # every output on every input; the records and q of a packed layout are known by their first byte only
        for a in SC.OUTPUTS:
            bad += [{a: dev["counts"].ptr + 4 * (n - 1)}, {a: dev["recs"].ptr}, {a: dev["q"].ptr}]
            if dev["offs"]:
                bad.append({a: dev["offs"].ptr + 4 * (n - 1)})
            else:
                bad += [{a: dev["recs"].ptr + 576 * (n * c["stride"] - 1)}, {a: dev["q"].ptr + 128 * (n * c["stride"] - 1)}]
        for kw in bad:
            assert call(**kw) == EINVAL, kw
        gctx.sync()
        for k, words in w.items():
            assert (gctx.download(dev[k], (max(words, 1),), np.uint32) == POISON_WORD).all(), k
        assert call() == 0                                       # the same arguments, unbroken, are accepted
        same(download(gctx, c, dev), SC.expected(c), "after the errors")


# ---- V against the device's own pair matcher

def test_votes_equal_the_pair_matcher_under_the_link_gate(gctx):
    """Eight frames: the chosen records of every frame gathered on the host into a packed batch, matched pair by pair by
    misift_match_pairs_batch_i8(mutual = 1) and gated by misift_link_tracks_batch (max_error = +inf) on the device; the
    accepted rows of pair (a, b) are V[a][b]."""
    case = SC.frames_case(8, top=16, seed=13)
    got = run(gctx, case)
    same(got, SC.expected(case), "frames_8")
    n, top = 8, case["top"]
    sel = got["sel"][:n * top].reshape(n, top)
    sub = [SC.frame_records(case, f) for f in range(n)]
    sub = [(p[sel[f, :got["sel_counts"][f]]], q[sel[f, :got["sel_counts"][f]]]) for f, (p, q) in enumerate(sub)]
    counts = np.array([len(p) for p, _ in sub], np.int32)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    recs, q = np.concatenate([p for p, _ in sub]), np.concatenate([x for _, x in sub])
    pairs = np.array([(a, b) for a in range(n) for b in range(a + 1, n)], np.int32)
    d = {k: gctx.upload(v) for k, v in dict(recs=recs, q=q, counts=counts, offs=offs).items()}
    rows, row_counts, _ = gctx.match_pairs_batch_i8(pairs, d["recs"], d["q"], n, d["counts"], d["offs"], 0,
                                                    max_pts=top, mutual=True)
    V = got["votes"][:n * n].reshape(n, n)
    h_rows = gctx.download(rows, (len(pairs), top * 576), np.uint8)
    h_counts = gctx.download(row_counts, (len(pairs),), np.int32)
    seen = 0
    for i, (a, b) in enumerate(pairs.tolist()):
        one_rows, one_counts = gctx.upload(h_rows[i]), gctx.upload(h_counts[i:i + 1])
        out = gctx.link_tracks_batch(pairs[i:i + 1], one_rows, one_counts, top, n, d["counts"], d["offs"], 0,
                                     max_records=int(offs[-1]), min_score=case["min_score"],
                                     max_ambiguity=case["max_ambiguity"])
        accepted = int(gctx.download(out[3], (8,), np.int32)[0])
        assert accepted == V[a, b] == V[b, a], (a, b, accepted, V[a, b])
        seen += accepted
    assert seen > 0


# ---- the chain

def test_chain_quantize_select_match_link(gctx):
    from test_match_pairs_i8_cpu import expected_pair_i8
    from test_tracks_cpu import expected_tracks
    case, seen = SC.small_ring_case()
    n, mp = len(case["counts"]), int(case["counts"].max())
    d = {k: gctx.upload(case[k]) for k in ("recs", "counts", "offs")}
    q = gctx.quantize_batch(d["recs"], n, d["counts"], d["offs"], 0)
    assert gctx.download(q, case["q"].shape, np.int8).tobytes() == case["q"].tobytes()
    out = gctx.select_pairs_batch(d["recs"], q, n, d["counts"], d["offs"], 0, **{k: case[k] for k in SC.ARGS})
    pairs = gctx.read_selected_pairs(out[3], out[5])             # the one host read of the chain's `pairs` convention
    exp = SC.expected(case)
    P = int(exp["summary"][1])
    assert pairs.tolist() == exp["pairs"][:2 * P].reshape(-1, 2).tolist()
    have = set(map(tuple, pairs.tolist()))
    for f in range(n):
        a, b = sorted((f, (f + 1) % n))
        assert (a, b) in have, (a, b)
    assert all(seen[a] & seen[b] for a, b in have)
    rows, row_counts, _ = gctx.match_pairs_batch_i8(pairs, d["recs"], q, n, d["counts"], d["offs"], 0, max_pts=mp,
                                                    mutual=True)
    got = gctx.download(rows, (len(pairs) * mp,), gctx_point_dtype())
    erows = np.zeros(len(pairs) * mp, got.dtype)
    for i, (a, b) in enumerate(pairs.tolist()):
        (pa, qa), (pb, qb) = SC.frame_records(case, a), SC.frame_records(case, b)
        e, _ = expected_pair_i8(pa, qa, pb, qb, True)
        for fld in OUT_FIELDS:
            assert np.array_equal(np.ascontiguousarray(got[fld][i * mp:i * mp + len(pa)]).view(np.uint32),
                                  np.ascontiguousarray(e[fld]).view(np.uint32)), (a, b, fld)
            erows[fld][i * mp:i * mp + len(pa)] = e[fld]
    total = int(case["offs"][-1] + case["counts"][-1])
    tr = gctx.link_tracks_batch(pairs, rows, row_counts, mp, n, d["counts"], d["offs"], 0, max_records=total)
    et = expected_tracks([tuple(p) for p in pairs.tolist()], erows, case["counts"][pairs[:, 0]], mp, case["counts"],
                         case["offs"], 0, total, (0.85, 0.95, float("inf")))
    for g, e in zip(tr, et):
        assert gctx.download(g, e.shape, np.int32).tobytes() == e.tobytes()
    assert et[3][1] > 0                                          # tracks of two and more records came out


def gctx_point_dtype():
    from cudasift_amd import capi
    return capi.POINT_DTYPE

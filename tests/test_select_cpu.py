"""misift_select_pairs_batch without a GPU: the numpy restatement of select_cases.py against the library's host hook
(misift_test_select_pairs: the rules of select_core.hpp, which the kernels compile too, applied with plain loops), byte
for byte on every case; against a brute force in plain Python on tiny cases; that every case hits what it is built for;
and the quality condition on the planted ring, which must hold for the restatement alone."""
import numpy as np
import pytest

import select_cases as SC
from batch_util import POISON_WORD


def hook(case, fill=POISON_WORD):
    from cudasift_amd import capi
    got = capi.select_pairs_host(case["recs"], case["q"], case["counts"], case["offs"], case["stride"],
                                 *[case[k] for k in SC.ARGS], fill=fill)
    return dict(zip(SC.OUTPUTS, got))


def test_library_exports_the_call_and_the_hook():
    from cudasift_amd import capi
    L = capi.lib()
    assert L.misift_select_pairs_batch and L.misift_test_select_pairs
    assert capi.Context.select_pairs_batch and capi.Context.read_selected_pairs


@pytest.mark.parametrize("name", sorted(SC.all_cases()))
def test_restatement_equals_the_hook(name):
    case = SC.all_cases()[name]
    exp, got = SC.expected(case), hook(case)
    for k in SC.OUTPUTS:
        bad = np.nonzero(exp[k] != got[k])[0]
        assert len(bad) == 0, (name, k, bad[:6], exp[k][bad[:6]], got[k][bad[:6]])


def test_hook_rejects_bad_arguments():
    from cudasift_amd import capi
    case = SC.all_cases()["frames_3"]
    for bad in (dict(top=0), dict(top=SC.MAX_TOP + 1), dict(k=0), dict(min_votes=0), dict(max_pairs=-1),
                dict(min_score=float("nan")), dict(max_ambiguity=float("nan"))):
        with pytest.raises(capi.MisiftError):
            hook(SC.variant(case, **bad))


# ---- the restatement against a brute force

def tiny_cases():
    rng = np.random.default_rng(5)
    out = []
    for i, (sizes, top, k) in enumerate((([6, 0, 5, 7], 4, 1), ([3, 9, 9, 2, 8], 5, 2), ([12, 12, 12], 12, 3))):
        fr = SC.pool_scene(sizes, 300 + i, 10)
        for p in fr:                                             # equal scales and equal descriptors: every tie rule
            if len(p) > 4:
                p["scale"][rng.integers(0, len(p), 3)] = p["scale"][0]
                p["data"][1] = p["data"][0]
        counts = list(sizes)
        if i == 1:
            counts[3] = -1
        out.append(SC.make_case(fr, counts, bool(i % 2), top=top, k=k, min_votes=1, max_ambiguity=1.5))
    return out


@pytest.mark.parametrize("i", range(3))
def test_restatement_equals_brute_force(i):
    case = tiny_cases()[i]
    n, top = len(case["counts"]), case["top"]
    sel, V, pairs = SC.brute(case)
    exp = SC.expected(case)
    esel = exp["sel"][:n * top].reshape(n, top)
    for f in range(n):
        assert esel[f, :len(sel[f])].tolist() == sel[f] and (esel[f, len(sel[f]):] == -1).all(), f
        assert exp["sel_counts"][f] == len(sel[f])
    assert exp["votes"][:n * n].reshape(n, n).tolist() == V
    assert exp["summary"][0] == len(pairs) and len(pairs) > 0
    assert exp["pairs"][:2 * len(pairs)].reshape(-1, 2).tolist() == [list(p) for p in pairs]
    assert sum(map(sum, V)) > 0


# ---- every case hits what it is built for

def outputs(case):
    n, top = len(case["counts"]), case["top"]
    e = SC.expected(case)
    return e, e["sel"][:n * top].reshape(n, top), e["votes"][:n * n].reshape(n, n)


@pytest.mark.parametrize("top", (1, 31, 32, 33, 64, 65, 255, 256))
def test_size_cases_cover_the_counts(top):
    case = SC.size_case(top, False)
    e, sel, V = outputs(case)
    assert case["counts"].tolist() == [-1, 0, 1, top - 1, top, top + 1, 3 * top]
    assert e["sel_counts"][:7].tolist() == [0, 0, 1, top - 1, top, top, top]
    assert e["summary"][3] == 2                                  # top + 1 and 3 top records: more than top
    assert (sel[0] == -1).all() and (sel[1] == -1).all()
    if top >= 31:
        assert V[5, 6] >= 2 and e["summary"][0] >= 1             # the large frames share their largest features


def test_frame_count_cases():
    for n in (0, 1, 2, 3, 65):
        e = SC.expected(SC.frames_case(n, padded=n == 3))
        assert len(e["votes"]) == max(n * n, 1)
    assert SC.expected(SC.frames_case(0))["summary"].tolist() == [0] * 8
    assert SC.expected(SC.frames_case(65))["summary"][0] > 65 // 2
    e = SC.expected(SC.strip_case())
    assert 100 * 99 // 2 > 8 * 2 * 256 and e["summary"][0] > 50  # more pairs than strips of one frame on 256 CUs


def test_long_frame_chooses_beyond_the_cached_keys():
    case = SC.long_frame_case()
    _, sel, _ = outputs(case)
    first = sel[0]
    assert first[:30].tolist() == list(range(8500, 8530)) and first[30:40].tolist() == list(range(8200, 8210))
    rest = SC.frame_records(case, 0)[0]["scale"][first[40:]]
    assert (first[40:] < 8192).all() and len(set(rest.tolist()[-5:])) == 1       # the threshold is a tie, cut by index
    assert (SC.frame_records(case, 0)[0]["scale"] == rest[-1]).sum() > (rest == rest[-1]).sum()


def test_scale_cases():
    case = SC.scale_case("equal")
    _, sel, _ = outputs(case)
    for f, n in enumerate(case["counts"]):
        h = min(n, case["top"])
        assert sel[f, :h].tolist() == list(range(h))             # equal keys: the lower index wins
    case = SC.scale_case("special")
    _, sel, _ = outputs(case)
    for f in (0, 1, 3):
        p, _ = SC.frame_records(case, f)
        s = p["scale"][sel[f, :case["top"]]]
        with np.errstate(invalid="ignore"):
            pos = int((p["scale"] > 0).sum())
            assert pos < case["top"] < len(p)                    # keys of 0 are chosen too, by index
            assert s[0] == np.inf and (s[:pos] > 0).all() and not (s[pos:] > 0).any()
        kinds = p["scale"][sel[f, pos:case["top"]]]
        assert np.isnan(kinds).any() or (kinds <= 0).any()
        assert (np.diff(sel[f, pos:case["top"]]) > 0).all()
        tiny = p["scale"][(p["scale"] > 0) & (p["scale"] < 1e-38)]
        assert len(tiny) and set(tiny.tolist()) <= set(s.tolist())          # subnormals are positive keys


def test_duplicate_case_ties_rows_and_columns():
    case = SC.duplicate_case()
    _, _, V = outputs(case)
    (pa, qa), (pb, qb) = SC.frame_records(case, 0), SC.frame_records(case, 1)
    S = qa.astype(np.int64) @ qb.astype(np.int64).T
    row_ties = sum(int((S[i] == S[i].max()).sum() > 1 and S[i].max() > 0) for i in range(len(S)))
    col_ties = sum(int((S[:, j] == S[:, j].max()).sum() > 1 and S[:, j].max() > 0) for j in range(S.shape[1]))
    assert row_ties >= 3 and col_ties >= 3
    assert (qa == 0).all(1).any() and (qb == 0).all(1).any()
    assert 0 < V[0, 1] < len(pa)
    strict = SC.variant(case, max_ambiguity=0.95, memo={})       # under the usual gate the tied rows do not vote
    assert outputs(strict)[2][0, 1] < V[0, 1]


def test_gate_cases_sit_on_the_thresholds():
    g = SC.gate_cases()
    V = {k: outputs(c)[2][0, 1] for k, c in g.items()}
    assert V == dict(score_at=0, score_below=1, ambiguity_at=0, ambiguity_above=1)


def test_vote_cases():
    base = SC.vote_case()
    e, _, V = outputs(base)
    assert (V[:, 3] == V[:, 6]).sum() >= 7 and (V[:, 1] == V[:, 3]).sum() >= 7         # ties between neighbours
    v = SC.vote_variants()
    at = v["min_votes_at"]["min_votes"]
    tri = V[np.triu_indices(len(V), 1)]
    assert (tri == at).any() and (tri == at - 1).any()           # pairs exactly at min_votes, and one below
    P_at, P_above = SC.expected(v["min_votes_at"])["summary"][0], SC.expected(v["min_votes_above"])["summary"][0]
    assert P_above < P_at
    P = [int(SC.expected(v[k])["summary"][0]) for k in ("k1", "k2", "k_all")]
    assert P[0] < P[1] < P[2] == 36                              # k = nframes: every pair with a vote
    # k = 1 among tied neighbours: the smaller frame is taken
    pairs1 = SC.expected(v["k1"])["pairs"][:2 * P[0]].reshape(-1, 2).tolist()
    for f in range(len(V)):
        best = SC.neighbours_np(V, f, 1, 1)
        tied = [g for g in range(len(V)) if g != f and V[f, g] == V[f, best[0]]]
        assert best[0] == min(tied) and sorted((f, int(best[0]))) in pairs1
    want = int(e["summary"][0])
    for name, written in (("none", 0), ("short", want - 1), ("exact", want), ("room", want)):
        s = SC.expected(v["max_pairs_" + name])
        assert s["summary"][:2].tolist() == [want, written]
        assert (s["pairs"][2 * written:] == np.int32(POISON_WORD)).all()


# ---- the quality condition

def test_planted_ring_selects_the_ring():
    """24 frames on a ring, top 64, k 4: every ring-adjacent pair is selected, and no pair whose frames share no scene
    point."""
    case, seen = SC.ring_case()
    assert case["top"] == 64 and case["k"] == 4 and len(seen) == 24
    e = SC.expected(case)
    P = int(e["summary"][0])
    pairs = set(map(tuple, e["pairs"][:2 * P].reshape(-1, 2).tolist()))
    for f in range(24):
        assert tuple(sorted((f, (f + 1) % 24))) in pairs, f
    for a, b in pairs:
        assert seen[a] & seen[b], (a, b)
    assert 24 <= P <= 48 and e["summary"][2] == 0 and e["summary"][3] == 24
    shared_none = [(a, b) for a in range(24) for b in range(a + 1, 24) if not seen[a] & seen[b]]
    assert len(shared_none) > 150                                # most pairs share nothing: exhaustive would match them all

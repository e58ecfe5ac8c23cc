"""misift_match_guided_batch and misift_match_epipolar_batch on the hostile scenes of guided_cases.py: offset and huge
bounding boxes, non-finite records, degenerate boxes, outliers that blow the cells up, one row that fills the candidate
queue round after round, projections and lines that leave the box, radius extremes and records on which a fused gate
would decide otherwise.

Every comparison is byte equality against the restatements of test_gpu_guided_match.py and test_gpu_epipolar_match.py
(the gate in numpy float32, then the oracle's exact full matcher on the candidates), computed once per scene by
guided_cases.expected; test_guided_cases_cpu.py asserts that the scenes hold what they are built for."""
import numpy as np
import pytest

import guided_cases as gc
from batch_util import MATCH_FIELDS, guarded_context, layout, same_bytes

pytestmark = pytest.mark.gpu


def _run(kind):
    if kind == "guided":
        from test_gpu_guided_match import _run as run
    else:
        from test_gpu_epipolar_match import _run as run
    return run


def _check(c, kind, name, padded, runs=2):
    s, r1, o1, r2, o2, ef, enf = gc.expected(kind, name)
    s1 = s2 = 0
    exp = np.concatenate(ef)
    if padded:
        r1, o1, s1 = layout(s.fr1, s.counts1, True, min_stride=0, pad_error=0.0)
        r2, o2, s2 = layout(s.fr2, s.counts2, True, min_stride=0, pad_error=0.0)
        exp, _, _ = layout(ef, s.counts1, True, min_stride=0, pad_error=0.0)
    first = None
    for k in range(runs):
        got1, got2, nf = _run(kind)(c, s.pairs, s.mats, s.radius, r1, s.counts1, o1, s1, r2, s.counts2, o2, s2)
        same_bytes(got1, exp, "%s %s: set 1, run %d" % (kind, name, k))
        same_bytes(got2, r2, "%s %s: set 2 (read only), run %d" % (kind, name, k))
        assert np.array_equal(nf, enf), (kind, name, k, nf, enf)
        if first is not None:
            same_bytes(got1, first, "%s %s: two runs" % (kind, name))
        first = got1
    return first


@pytest.mark.parametrize("name", gc.NAMES)
@pytest.mark.parametrize("kind", gc.KINDS)
def test_scene(ctx, kind, name):
    _check(ctx, kind, name, False)


@pytest.mark.parametrize("name", ["offset", "nonfinite"])
@pytest.mark.parametrize("kind", gc.KINDS)
def test_scene_padded(ctx, kind, name):
    _check(ctx, kind, name, True)


@pytest.mark.parametrize("kind,name", [("guided", "greedy"), ("epipolar", "leaving")])
def test_scene_on_a_guarded_context(ctx, kind, name):
    """A fresh guarded context (temp and plan buffers start NaN-poisoned, 64 KiB guard bands): no band damaged, and the
    restatement's bytes."""
    from cudasift_amd import capi
    with guarded_context(3) as g:
        _check(g, kind, name, False, runs=1)
    assert capi.check_guards() >= 0


@pytest.mark.parametrize("kind", gc.KINDS)
def test_outlier_with_unbounded_radius_equals_exact_full_match(ctx, kind):
    """radius = +inf: every finite row has the same candidates, all records but the outliers the gate rejects, so its five
    fields are misift_match's in exact, full mode against those records alone."""
    got = _check(ctx, kind, "outlier_inf", False, runs=1)
    s, r1, o1, r2, o2, ef, enf = gc.expected(kind, "outlier_inf")
    ctx.set_options(match_full=1, match_exact_top2=1)
    try:
        for i, (f1, f2) in enumerate(s.pairs):
            a, b = s.fr1[f1], s.fr2[f2]
            g = gc.gate(kind, s.mats[i], gc.xy(a), gc.xy(b), s.radius)
            live = np.nonzero(g.any(1))[0]
            adm = np.nonzero(g[live[0]])[0]
            assert (g[live] == g[live[0]]).all() and len(b) - 2 <= len(adm) <= len(b)
            exp = ctx.match(a[live].copy(), len(live), b[adm].copy(), len(adm))
            exp["match"] = adm[exp["match"]]
            rows = got[int(o1[f1]):int(o1[f1]) + len(a)][live]
            for k in MATCH_FIELDS:
                assert np.array_equal(exp[k].view(np.uint32), rows[k].view(np.uint32)), (kind, i, k)
            assert enf[i] == len(live)
    finally:
        ctx.set_options(match_full=0, match_exact_top2=0)

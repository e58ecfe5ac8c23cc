"""misift_link_poses_batch on the device: a ratio per link, the scales, a camera per image.

Every comparison is byte equality with posegraph_cases.expected_link_poses (pinned in test_posegraph_cpu.py to the
library's host hooks and to float64, where the premises of the cases are asserted too): d_link_ratio, d_link_common,
d_pair_scale, d_cam, d_cam_pair, d_summary, and every byte of the rows, the poses, the votes and d_xyz, which the call must
not write.  The rows are planted directly; no images are needed.  The outputs have exactly the stated capacity and are
poisoned first; all allocations of the module are guarded.  The sample counts are the ones at which the kernels can go
wrong: none, both parities of the lower median, either side of min_common, the workgroup's 256 threads and one more, and
either side of what the ratio kernel stages on chip and of what the second kernel stages on chip."""
import numpy as np
import pytest

import posegraph_cases as G
from batch_util import POISON_WORD, guarded_context
from test_fundamental_cpu import GATES, f32

pytestmark = pytest.mark.gpu

MISIFT_OK, MISIFT_EINVAL = 0, -1
OUTPUTS = ("link_ratio", "link_common", "pair_scale", "cam", "cam_pair", "summary")


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


def _poisoned(ctx, words):
    return ctx.upload(np.full(max(words, 1), POISON_WORD, np.uint32))


def _sizes(case):
    nl, npairs = len(case["links"]), len(case["pairs"])
    return dict(link_ratio=nl, link_common=nl, pair_scale=npairs, cam=12 * case["nimages"], cam_pair=case["nimages"],
                summary=8)


def _link(ctx, case):
    """The call on poisoned outputs of exactly the stated sizes; returns them as uint32 arrays of those sizes (a size of 0
    is one word, which must stay poisoned).  The inputs must come back as they went in."""
    from cudasift_amd import capi
    ins = dict(rows=ctx.upload(case["rows"]), row_counts=ctx.upload(case["row_counts"]),
               pose=ctx.upload(np.ascontiguousarray(case["pose"], f32)), num_front=ctx.upload(case["num_front"]),
               xyz=ctx.upload(np.ascontiguousarray(case["xyz"], f32)))
    sizes = _sizes(case)
    outs = {k: _poisoned(ctx, n) for k, n in sizes.items()}
    ctx.link_poses_batch(case["pairs"], case["nimages"], ins["rows"], ins["row_counts"], case["max_pts"], ins["pose"],
                         ins["num_front"], ins["xyz"], case["links"], case["seed_pair"], case["root_image"],
                         case["walk"], min_common=case["min_common"], min_score=GATES[0], max_ambiguity=GATES[1],
                         max_error=case["max_error"], **outs)
    ctx.sync()
    assert ctx.download(ins["rows"], (len(case["rows"]),), capi.POINT_DTYPE).tobytes() == case["rows"].tobytes()
    for k, dt in (("row_counts", np.int32), ("pose", f32), ("num_front", np.int32), ("xyz", f32)):
        want = np.ascontiguousarray(case[k], dt)
        assert ctx.download(ins[k], (want.size,), dt).tobytes() == want.tobytes(), (k, "was written")
    return {k: ctx.download(outs[k], (max(n, 1),), np.uint32) for k, n in sizes.items()}


def _compare(got, case, what):
    with np.errstate(all="ignore"):
        e = G.expected_link_poses(case)
    for k, n in _sizes(case).items():
        want = np.ascontiguousarray(e[k]).reshape(-1).view(np.uint32)
        if n == 0:
            assert got[k][0] == POISON_WORD, (what, k, "written without an entry")
            continue
        bad = np.nonzero(got[k] != want)[0]
        assert len(bad) == 0, (what, k, "%d words differ, first %s" % (len(bad), bad[:8]),
                               got[k][bad[:4]].view(e[k].dtype), want[bad[:4]].view(e[k].dtype))
    return e


def test_every_sample_count(g):
    case = G.count_case()
    e = _compare(_link(g, case), case, "sample counts")
    assert sorted(set(e["link_common"].tolist())) == sorted(G.SMALL_COUNTS) and case["max_pts"] % 16


def test_either_side_of_the_staged_rows(g):
    cap = G.capacity(0)
    case = G.capacity_case(cap)
    e = _compare(_link(g, case), case, "staging capacity")
    assert sorted(set(e["link_common"].tolist())) == [cap - 1, cap, cap + 1]


def test_row_counts_and_ties(g):
    for name in ("row_count", "tie"):
        case = getattr(G, name + "_case")()
        _compare(_link(g, case), case, name)


@pytest.mark.parametrize("max_error", [2.0, G.INF], ids=["finite max_error", "max_error inf"])
def test_hostile_rows(g, max_error):
    case = G.hostile_case(max_error)
    e = _compare(_link(g, case), case, "hostile rows")
    assert (e["link_common"] >= 60).all()


def test_graphs(g):
    """Propagation and walk: outward, too early, backward, a cycle, unusable pairs, two ways, self pairs, repeats, no
    links, no walk, and more links than the second kernel stages on chip."""
    cases = G.graph_cases(G.capacity(1))
    assert 3 * len(cases[-1][1]["links"]) > G.capacity(1)
    for name, case, facts in cases:
        e = _compare(_link(g, case), case, name)
        assert e["summary"][1] == facts["scaled"] and e["summary"][2] == facts["cams"], (name, e["summary"])


def test_two_runs_are_identical(g):
    case = G.hostile_case()
    a, b = _link(g, case), _link(g, case)
    for k in OUTPUTS:
        assert a[k].tobytes() == b[k].tobytes(), k
    case = G.planted_scene()["case"]
    a, b = _link(g, case), _link(g, case)
    for k in OUTPUTS:
        assert a[k].tobytes() == b[k].tobytes(), k
    _compare(a, case, "planted scene, rows from the restatements")


def test_find_improve_recover_link(g):
    """The chain on the 8-camera scene, nothing read in between: byte-equal to the restatements, and within the CPU
    file's recorded bounds of the planted cameras."""
    from test_posegraph_cpu import (SCENE_R_MEASURED, SCENE_RATIO_MEASURED, SCENE_T_MEASURED, scene_errors)
    sc = G.planted_scene()
    case, S = sc["case"], sc["S"]
    n, npairs = S["n"], len(sc["pairs"])
    sel = list(range(npairs))
    d, dc = g.upload(np.concatenate(sc["raw"])), g.upload(np.full(npairs, n, np.int32))
    dfit, dpose, dfront, dxyz = (_poisoned(g, k) for k in (npairs, 12 * npairs, npairs, 4 * n * npairs))
    outs = {k: _poisoned(g, m) for k, m in _sizes(case).items()}
    gates = dict(min_score=GATES[0], max_ambiguity=GATES[1], thresh=S["thresh"])
    dF, _ = g.find_fundamental_batch(sel, sc["seeds"], d, npairs, dc, None, n, max_pts=n, num_loops=S["find_loops"],
                                     **gates)
    g.improve_fundamental_batch(sel, d, npairs, dc, dF, None, n, num_fit=dfit, num_loops=S["improve_loops"], **gates)
    g.recover_pose_batch(sel, np.tile(sc["K8"], (npairs, 1)), d, npairs, dc, dF, None, n, pose=dpose, num_front=dfront,
                         xyz=dxyz, **gates)
    g.link_poses_batch(case["pairs"], case["nimages"], d, dc, n, dpose, dfront, dxyz, case["links"], case["seed_pair"],
                       case["root_image"], case["walk"], min_common=case["min_common"], min_score=GATES[0],
                       max_ambiguity=GATES[1], max_error=case["max_error"], **outs)
    g.sync()
    assert g.download(dF, (npairs, 9), f32).tobytes() == sc["F"].tobytes()
    assert g.download(dpose, (npairs, 12), f32).tobytes() == case["pose"].tobytes()
    assert g.download(dxyz, (npairs * n, 4), np.uint32).tobytes() == case["xyz"].view(np.uint32).tobytes()
    got = {k: g.download(outs[k], (m,), np.uint32) for k, m in _sizes(case).items()}
    e = _compare(got, case, "chain")
    dev = dict(link_ratio=got["link_ratio"].view(f32), cam=got["cam"].view(f32).reshape(-1, 12))
    errs, ref = scene_errors(sc, dev)
    for v, r, m in zip(errs, ref, (SCENE_RATIO_MEASURED, SCENE_R_MEASURED, SCENE_T_MEASURED)):
        assert v <= 2 * r and v <= 2 * m, (errs, ref)
    assert e["summary"].tolist()[:3] == [len(case["links"]), npairs, case["nimages"]]


def test_argument_errors_enqueue_nothing(g):
    from cudasift_amd import capi
    L = capi.lib()
    case = G.graph_cases()[0][1]                                 # five pairs in a row, four CHAIN links
    pairs, links = np.ascontiguousarray(case["pairs"], np.int32), np.ascontiguousarray(case["links"], np.int32)
    walk = np.ascontiguousarray(case["walk"], np.int32)
    npairs, nl, nimg = len(pairs), len(links), case["nimages"]
    dev = dict(rows=g.upload(case["rows"]), counts=g.upload(case["row_counts"]), pose=g.upload(case["pose"]),
               front=g.upload(case["num_front"]), xyz=g.upload(case["xyz"]))
    outs = {k: _poisoned(g, m) for k, m in _sizes(case).items()}
    good = dict(ctx=g.h, npairs=npairs, pairs=pairs.ctypes.data, nimages=nimg, rows=dev["rows"].ptr,
                counts=dev["counts"].ptr, max_pts=case["max_pts"], min_score=0.85, max_ambiguity=0.95, max_error=2.0,
                pose=dev["pose"].ptr, front=dev["front"].ptr, xyz=dev["xyz"].ptr, nlinks=nl, links=links.ctypes.data,
                seed_pair=0, root_image=0, min_common=8, nwalk=len(walk), walk=walk.ctypes.data,
                **{k: outs[k].ptr for k in OUTPUTS})

    def link(**kw):
        a = dict(good, **kw)
        return L.misift_link_poses_batch(*[a[k] for k in good])

    nan = float("nan")
    bad = [dict(ctx=None), dict(npairs=-1), dict(nimages=0), dict(nimages=-2), dict(nlinks=-1), dict(nwalk=-1),
           dict(root_image=-1), dict(root_image=nimg), dict(min_common=0), dict(min_common=-4), dict(max_pts=0),
           dict(seed_pair=-1), dict(seed_pair=npairs), dict(min_score=nan), dict(max_ambiguity=nan), dict(max_error=nan),
           dict(max_error=0.0), dict(max_error=-1.0), dict(nimages=nimg - 1)]
    bad += [{k: None} for k in ("pairs", "rows", "counts", "pose", "front", "xyz", "links", "walk") + OUTPUTS]
    lists = []                                                   # kept alive until the calls are made

    def broken(which, src, at, value):
        v = src.copy()
        v.reshape(-1)[at] = value
        lists.append(v)
        return {which: v.ctypes.data}

    bad += [broken("pairs", pairs, 3, -1), broken("pairs", pairs, 4, nimg)]
    bad += [broken("links", links, 0, -1), broken("links", links, 3, npairs), broken("links", links, 4, -1),
            broken("links", links, 1, npairs), broken("links", links, 5, 2), broken("links", links, 2, -1),
            broken("links", links, 4, 3),                        # CHAIN (1, 3): image 2 is not image 3
            broken("links", links, 2, 1)]                        # FAN (0, 1): images 0 and 1 differ
    bad += [broken("walk", walk, 0, -1), broken("walk", walk, 2, npairs)]
    for kw in bad:
        assert link(**kw) == MISIFT_EINVAL, kw
    g.sync()
    for k, m in _sizes(case).items():
        assert (g.download(outs[k], (m,), np.uint32) == POISON_WORD).all(), k
    # no pairs: the root alone, with every input NULL; then the same arguments, unbroken
    assert link(npairs=0, pairs=None, rows=None, counts=None, pose=None, front=None, xyz=None, nlinks=0, links=None,
                link_ratio=None, link_common=None, nwalk=0, walk=None, seed_pair=77, root_image=3) == MISIFT_OK
    g.sync()
    cam_pair = g.download(outs["cam_pair"], (nimg,), np.int32)
    assert cam_pair.tolist() == [G.UNSET] * 3 + [G.ROOT] + [G.UNSET] * (nimg - 4)
    cam = g.download(outs["cam"], (nimg, 12), f32)
    assert cam[3].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] and not np.delete(cam, 3, 0).any()
    assert g.download(outs["summary"], (8,), np.int32).tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    for k in ("link_ratio", "link_common", "pair_scale"):
        assert (g.download(outs[k], (_sizes(case)[k],), np.uint32) == POISON_WORD).all(), k
    assert link() == MISIFT_OK
    g.sync()
    _compare({k: g.download(outs[k], (m,), np.uint32) for k, m in _sizes(case).items()}, case, "unbroken")


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0

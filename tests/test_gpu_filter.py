"""misift_filter_tracks_batch on the device: the observation lists gated against the points and cameras and written out
again in export's format.

Every comparison is byte equality with filter_cases.expected_filter (pinned in test_filter_cpu.py to the library's host
hook and to float64, where the premises of the cases are asserted too): all nine outputs at exactly their stated sizes,
poisoned first, so the regions the call must leave alone show, and every byte of the seven inputs, which the call must not
write.  The scenes are planted directly; no images are needed.  All allocations of the module are guarded.  The shapes are
the ones at which the kernels can go wrong: track counts around the four wavefronts of a workgroup, around one wavefront
and around the 2048-track tile of the scan, T and O from the device below, beyond and under their capacities, tracks of
1 to 301 views and one beyond the staging, duplicates at the chunk boundary of the ranking, both gates at equality."""
import numpy as np
import pytest

import bundle_cases as BC
import filter_cases as FC
import posegraph_cases as G
import pose_cases as PC
import refine_cases as RC
import triangulate_cases as TC
from batch_util import POISON_WORD, guarded_context
from test_filter_cpu import CASE_NAMES
from test_fundamental_cpu import GATES, f32

pytestmark = pytest.mark.gpu

MISIFT_OK, MISIFT_EINVAL = 0, -1
INPUTS = (("track_offsets", np.int32), ("obs", TC.OBS_DTYPE), ("export_summary", np.int32), ("points", f32),
          ("point_status", np.int32), ("cam", f32), ("cam_pair", np.int32))


@pytest.fixture(scope="module")
def g():
    assert POISON_WORD == FC.POISON_WORD
    with guarded_context(1) as c:
        yield c


@pytest.fixture(scope="module")
def cases():
    return FC.cpu_cases()


def _poisoned(ctx, words):
    return ctx.upload(np.full(max(words, 1), POISON_WORD, np.uint32))


def _download(ctx, outs, case):
    return {k: (ctx.download(outs[k], (m,), np.uint32) if outs[k] is not None else np.full(m, POISON_WORD, np.uint32))
            for k, m in FC.sizes(case).items()}


def _filter(ctx, case, obs_map=True):
    """The call on poisoned outputs of exactly the stated sizes; returns them as uint32 arrays.  The inputs must come back
    as they went in."""
    ins = FC.inputs(case)
    dev = {k: ctx.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(ctx, n) for k, n in FC.sizes(case).items()}
    if not obs_map:
        outs["obs_map"] = None
    ctx.filter_tracks_batch(case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"],
                            dev["points"], dev["point_status"], case["nimages"], dev["cam"], dev["cam_pair"],
                            case["intrinsics"], max_error=case["max_error"], max_cos=case["max_cos"],
                            min_views=case["min_views"], unique_frames=case["unique_frames"], **outs)
    ctx.sync()
    for k, dt in INPUTS:
        assert ctx.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    return _download(ctx, outs, case)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_case(g, cases, name):
    """The cases of filter_cases.cpu_cases (what each is built to hit is asserted in test_filter_cpu.py)."""
    case = cases[name]
    FC.compare(_filter(g, case), FC.expected_filter(case), name)


def test_two_runs_give_the_same_bytes_and_obs_map_may_be_null(g, cases):
    for name in ("hostile gated", "views over 8 images, unique 1", "outliers, angle"):
        case = cases[name]
        e = FC.expected_filter(case)
        first, again, without = _filter(g, case), _filter(g, case), _filter(g, case, obs_map=False)
        FC.compare(first, e, name)
        for k in FC.OUTPUTS:
            assert first[k].tobytes() == again[k].tobytes(), (name, k)
        FC.compare(without, e, name + ", no d_obs_map", [k for k in FC.OUTPUTS if k != "obs_map"])


def test_idempotent_on_the_device(g, cases):
    """The call on its own outputs, as the device wrote them, keeps everything."""
    for name in ("views over 8 images, unique 1", "hostile gated", "outliers, angle"):
        case = cases[name]
        first = _filter(g, case)
        Tn, On = first["summary"].view(np.int32)[:2]
        again = _filter(g, FC.filtered_case(case, first))
        assert again["summary"].view(np.int32).tolist() == [Tn, On, 0, 0, 0, 0, 0, 0], name
        for k, n in (("track_offsets_out", Tn + 1), ("obs_out", 4 * On), ("points_out", 4 * Tn), ("point_views_out", Tn),
                     ("point_status_out", Tn)):
            assert again[k][:n].tobytes() == first[k][:n].tobytes(), (name, k)


def test_one_context_after_a_refine_with_more_and_with_less_temp(g, cases):
    """The temp of the context is shared: the call after a refine that left it larger (8 bytes x 100 000 slots), and in a
    fresh context after one that left it smaller."""
    small = RC.spread_case(257)
    big = RC.variant(small, max_obs=100000, obs=np.concatenate([small["obs"], np.zeros(100000 - 257, TC.OBS_DTYPE)]))

    def refine(ctx, rc):
        dev = {k: ctx.upload(v) for k, v in FC.inputs(rc).items()}
        ctx.refine_cameras_batch(rc["max_tracks"], rc["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"],
                                 dev["points"], dev["point_status"], rc["nimages"], dev["cam"], dev["cam_pair"],
                                 rc["intrinsics"], hold=rc["hold"], min_obs=rc["min_obs"], num_loops=1,
                                 max_error=rc["max_error"], orthonormalise=0)

    case = cases["outliers, angle"]
    refine(g, big)
    FC.compare(_filter(g, case), FC.expected_filter(case), "after a larger temp")
    with guarded_context(1) as fresh:
        refine(fresh, RC.spread_case(1))
        case = cases["views over 8 images, unique 1"]
        FC.compare(_filter(fresh, case), FC.expected_filter(case), "after a smaller temp")


def test_argument_errors_enqueue_nothing(g, cases):
    from cudasift_amd import capi
    L = capi.lib()
    case = cases["duplicates, unique 1"]
    ins = FC.inputs(case)
    dev = {k: g.upload(v) for k, v in ins.items()}
    sizes = FC.sizes(case)
    outs = {k: _poisoned(g, n) for k, n in sizes.items()}
    K = np.ascontiguousarray(case["intrinsics"], f32)
    n, mt, mo = case["nimages"], case["max_tracks"], case["max_obs"]
    good = dict(ctx=g.h, max_tracks=mt, max_obs=mo, track_offsets=dev["track_offsets"].ptr, obs=dev["obs"].ptr,
                export_summary=dev["export_summary"].ptr, points=dev["points"].ptr, point_status=dev["point_status"].ptr,
                nimages=n, cam=dev["cam"].ptr, cam_pair=dev["cam_pair"].ptr, intrinsics=K.ctypes.data, max_error=np.inf,
                max_cos=np.inf, min_views=2, unique_frames=1, **{k: outs[k].ptr for k in FC.OUTPUTS})

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_filter_tracks_batch(*[a[k] for k in good])

    bad = [dict(ctx=None), dict(max_tracks=0), dict(max_tracks=-1), dict(max_obs=0), dict(max_obs=-7), dict(nimages=0),
           dict(nimages=-1), dict(min_views=1), dict(min_views=0), dict(min_views=-2), dict(unique_frames=2),
           dict(unique_frames=-1), dict(max_error=np.nan), dict(max_error=0.0), dict(max_error=-1.0),
           dict(max_error=-np.inf), dict(max_cos=np.nan), dict(obs=dev["obs"].ptr + 4), dict(obs=dev["obs"].ptr + 8),
           dict(obs_out=outs["obs_out"].ptr + 4), dict(obs_out=outs["obs_out"].ptr + 8)]
    bad += [{k: None} for k in good if k != "obs_map" and k not in ("max_tracks", "max_obs", "nimages", "max_error",
                                                                   "max_cos", "min_views", "unique_frames", "ctx")]
    # in place and every other overlap: an output on an input, at its start, its last word and one word before it
    bad += [dict(obs_out=dev["obs"].ptr), dict(track_offsets_out=dev["track_offsets"].ptr),
            dict(points_out=dev["points"].ptr), dict(point_status_out=dev["point_status"].ptr),
            dict(export_summary_out=dev["export_summary"].ptr), dict(summary=dev["export_summary"].ptr + 28),
            dict(summary=dev["export_summary"].ptr - 28), dict(track_map=dev["point_status"].ptr + 4 * mt - 4),
            dict(obs_map=dev["obs"].ptr + 16 * mo - 4), dict(obs_map=dev["obs"].ptr - 4 * mo + 4),
            dict(point_views_out=dev["cam_pair"].ptr), dict(track_map=dev["cam"].ptr + 48 * n - 4),
            dict(points_out=dev["obs"].ptr + 16), dict(obs_out=dev["points"].ptr)]
    # an output on another output
    bad += [dict(track_map=outs["point_views_out"].ptr), dict(point_status_out=outs["point_views_out"].ptr + 4 * mt - 4),
            dict(summary=outs["export_summary_out"].ptr), dict(summary=outs["export_summary_out"].ptr + 16),
            dict(obs_map=outs["obs_out"].ptr + 16), dict(track_offsets_out=outs["track_map"].ptr - 4 * mt)]
    lists = []                                                   # kept alive until the calls are made
    for at in (0, 1, 4 * n - 4, 4 * n - 3):
        for v in (0.0, -1500.0, np.nan, np.inf, -np.inf):        # fx, fy of the first and the last image
            lists.append(K.copy())
            lists[-1].reshape(-1)[at] = v
            bad.append(dict(intrinsics=lists[-1].ctypes.data))
    for at in (2, 3, 4 * n - 1):
        for v in (np.nan, np.inf, -np.inf):                      # cx, cy
            lists.append(K.copy())
            lists[-1].reshape(-1)[at] = v
            bad.append(dict(intrinsics=lists[-1].ctypes.data))
    for kw in bad:
        assert call(**kw) == MISIFT_EINVAL, kw
    g.sync()
    for k, m in sizes.items():
        assert (g.download(outs[k], (m,), np.uint32) == POISON_WORD).all(), k
    for k, dt in INPUTS:
        assert g.download(dev[k], ins[k].shape, dt).tobytes() == ins[k].tobytes(), (k, "was written")
    # the same arguments, unbroken; then a gate that nothing passes
    assert call() == MISIFT_OK
    g.sync()
    FC.compare(_download(g, outs, case), FC.expected_filter(case), "unbroken")
    assert call(max_cos=-np.inf, max_error=1e-30) == MISIFT_OK
    g.sync()


def test_export_triangulate_adjust_filter_adjust_triangulate(g):
    """The chain on the 8-camera scene of posegraph_cases, nothing read in between: the cameras of find -> improve ->
    recover_pose -> link_poses, the observation lists of link_tracks -> export_tracks, then triangulate -> adjust -> filter
    -> adjust on the filter's outputs -> triangulate on them.  Each of the last four calls is byte-equal to its
    restatement fed the device's own buffers."""
    from cudasift_amd import capi
    sc = G.planted_scene()
    pc, S = sc["case"], sc["S"]
    n, npairs, nimg = S["n"], len(sc["pairs"]), pc["nimages"]
    sel = list(range(npairs))
    d, dc = g.upload(np.concatenate(sc["raw"])), g.upload(np.full(npairs, n, np.int32))
    dfit, dpose, dfront, dxyz = (_poisoned(g, k) for k in (npairs, 12 * npairs, npairs, 4 * n * npairs))
    gates = dict(min_score=GATES[0], max_ambiguity=GATES[1], thresh=S["thresh"])
    dF, _ = g.find_fundamental_batch(sel, sc["seeds"], d, npairs, dc, None, n, max_pts=n, num_loops=S["find_loops"],
                                     **gates)
    g.improve_fundamental_batch(sel, d, npairs, dc, dF, None, n, num_fit=dfit, num_loops=S["improve_loops"], **gates)
    g.recover_pose_batch(sel, np.tile(sc["K8"], (npairs, 1)), d, npairs, dc, dF, None, n, pose=dpose, num_front=dfront,
                         xyz=dxyz, **gates)
    _, _, _, dcam, dcam_pair, _ = g.link_poses_batch(pc["pairs"], nimg, d, dc, n, dpose, dfront, dxyz, pc["links"],
                                                     pc["seed_pair"], pc["root_image"], pc["walk"],
                                                     min_common=pc["min_common"], min_score=GATES[0],
                                                     max_ambiguity=GATES[1], max_error=pc["max_error"])
    recs = np.zeros(nimg * n, capi.POINT_DTYPE)
    for i in range(nimg - 1):
        assert tuple(sc["pairs"][i]) == (i, i + 1)
        recs[i * n:(i + 1) * n] = sc["raw"][i]
    last = sc["raw"][nimg - 2]
    for k, mk in (("xpos", "match_xpos"), ("ypos", "match_ypos")):
        recs[k][(nimg - 1) * n + last["match"]] = last[mk]
    total = nimg * n
    d_recs, d_cnt = g.upload(recs), g.upload(np.full(nimg, n, np.int32))
    lab = g.link_tracks_batch(pc["pairs"], d, dc, n, nimg, d_cnt, None, n, max_records=total, min_score=GATES[0],
                              max_ambiguity=GATES[1], max_error=pc["max_error"])
    mt, mo = total // 3 + 1, total
    doff, _, dobs, _, dsum = g.export_tracks_batch(d_recs, nimg, d_cnt, None, n, max_records=total, track=lab[0],
                                                   track_len=lab[1], track_frames=lab[2], min_len=3, consistent_only=1,
                                                   max_tracks=mt, max_obs=mo, record_obs=None)
    K = np.tile(np.array(PC.K_A, f32), (nimg, 1))
    hold = [i for i in pc["pairs"][pc["seed_pair"]] if i != pc["root_image"]]
    args = dict(min_views=2, min_obs=6, num_loops=3, cg_iters=10, max_error=RC.INF, lambda0=1e-3, orthonormalise=0)
    fargs = dict(max_error=6.0, max_cos=0.99999, min_views=2, unique_frames=1)
    bsizes = BC.sizes(dict(nimages=nimg, max_tracks=mt, num_loops=3))
    fsizes = FC.sizes(dict(max_tracks=mt, max_obs=mo))
    tri1 = g.triangulate_tracks_batch(mt, mo, doff, dobs, dsum, nimg, dcam, dcam_pair, K, min_views=2, num_loops=5)
    adj1 = {k: _poisoned(g, m) for k, m in bsizes.items()}
    g.adjust_bundle_batch(mt, mo, doff, dobs, dsum, tri1[0], tri1[2], nimg, dcam, dcam_pair, K, hold=hold, **args, **adj1)
    flt = {k: _poisoned(g, m) for k, m in fsizes.items()}
    g.filter_tracks_batch(mt, mo, doff, dobs, dsum, adj1["points_out"], tri1[2], nimg, adj1["cam_out"], dcam_pair, K,
                          **fargs, **flt)
    lists = (flt["track_offsets_out"], flt["obs_out"], flt["export_summary_out"])
    adj2 = {k: _poisoned(g, m) for k, m in bsizes.items()}
    g.adjust_bundle_batch(mt, mo, *lists, flt["points_out"], flt["point_status_out"], nimg, adj1["cam_out"], dcam_pair, K,
                          hold=hold, **args, **adj2)
    tri2 = g.triangulate_tracks_batch(mt, mo, *lists, nimg, adj2["cam_out"], dcam_pair, K, min_views=2, num_loops=5)
    g.sync()

    def get(outs, sizes):
        return {k: g.download(outs[k], (m,), np.uint32) for k, m in sizes.items()}

    pair = g.download(dcam_pair, (nimg,), np.int32)
    base = dict(max_tracks=mt, max_obs=mo, track_offsets=g.download(doff, (mt + 1,), np.int32),
                obs=g.download(dobs, (mo,), TC.OBS_DTYPE), export_summary=g.download(dsum, (8,), np.int32),
                nimages=nimg, intrinsics=K, cam_pair=pair, hold=tuple(hold))
    st1 = g.download(tri1[2], (mt,), np.int32)
    got1, gotf, got2 = get(adj1, bsizes), get(flt, fsizes), get(adj2, bsizes)
    case1 = dict(base, cam=g.download(dcam, (nimg, 12), f32), points=g.download(tri1[0], (mt, 4), f32), point_status=st1,
                 **args)
    BC.compare(got1, BC.expected_bundle(case1), "chain, first adjust")
    casef = dict(base, cam=got1["cam_out"].view(f32).reshape(-1, 12), points=got1["points_out"].view(f32).reshape(-1, 4),
                 point_status=st1, **fargs)
    ef = FC.expected_filter(casef)
    FC.compare(gotf, ef, "chain, filter")
    case2 = dict(FC.filtered_case(casef, gotf), **args)
    e2 = BC.expected_bundle(case2)
    BC.compare(got2, e2, "chain, second adjust")
    tc = dict(case2, cam=got2["cam_out"].view(f32).reshape(-1, 12), min_views=2, num_loops=5, memo={})
    with np.errstate(all="ignore"):
        x = TC.expected_triangulate(tc)
    got3 = dict(points=g.download(tri2[0], (4 * mt,), np.uint32), point_views=g.download(tri2[1], (mt,), np.uint32),
                point_status=g.download(tri2[2], (mt,), np.uint32), obs_error=g.download(tri2[3], (mo,), np.uint32),
                summary=g.download(tri2[4], (8,), np.uint32))
    for k in got3:
        written = x[k] != POISON_WORD                            # what the call leaves alone was zeroed here, not poisoned
        assert (got3[k][written] == x[k][written]).all(), k
    s, T = ef["summary"].view(np.int32), int(base["export_summary"][2])
    print("chain: T %d -> %d, summary %s; cost %s -> %s" % (T, s[0], s.tolist(), got1["cost"].view(f32), got2["cost"].view(f32)))
    assert T >= 100 and s[0] > 0


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0

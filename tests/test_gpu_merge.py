"""misift_merge_scenes_batch on the device: two exported scenes in one gauge written out as one.

Every comparison is byte equality with merge_cases.expected_merge (pinned in test_merge_cpu.py to the library's host hook,
where the premises of the cases are asserted too): all thirteen outputs at exactly their stated sizes, poisoned first, so
the regions the call must leave alone show, and every byte of the inputs, which the call must not write.  The scenes are
fabricated directly; no images are needed.  All allocations of the module are guarded.  The shapes are the ones at which
the kernels can go wrong: track counts around one wavefront, the four wavefronts of a workgroup and the 2048-track tile of
both scans, unions of 0 to 602 elements and beyond the staging, 70 partners of one track, T and O from the device below,
beyond and under their capacities, the capacity cut in either part."""
import numpy as np
import pytest

import align_cases as AC
import filter_cases as FC
import merge_cases as MC
import posegraph_cases as G
import pose_cases as PC
import triangulate_cases as TC
from batch_util import POISON_WORD, guarded_context
from test_fundamental_cpu import GATES, f32
from test_merge_cpu import CASE_NAMES, bad_argument_table

pytestmark = pytest.mark.gpu

MISIFT_OK, MISIFT_EINVAL = 0, -1


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


@pytest.fixture(scope="module")
def cases():
    return MC.gpu_cases()


def _poisoned(ctx, words):
    return ctx.upload(np.full(max(words, 1), POISON_WORD, np.uint32))


def _scene_dev(ctx, S, ins):
    dev = {k: (None if v is None else ctx.upload(v)) for k, v in ins.items()}
    return dict(dev, max_tracks=S["max_tracks"], max_obs=S["max_obs"], nimages=S["nimages"],
                max_records=int(S.get("max_records") or 0))


def _merge(ctx, case):
    """The call on poisoned outputs of exactly the stated sizes; returns them as uint32 arrays (an output that was not
    passed: all poison).  The inputs must come back as they went in."""
    ins = MC.inputs(case)
    a, b = _scene_dev(ctx, case["a"], ins["a"]), _scene_dev(ctx, case["b"], ins["b"])
    dmap = ctx.upload(ins["map"])
    dacc = None if ins["accept"] is None else ctx.upload(ins["accept"])
    sizes = MC.sizes(case)
    outs = {k: (None if k in MC.OPTIONAL and not case["want"][k] else _poisoned(ctx, n)) for k, n in sizes.items()}
    ctx.merge_scenes_batch(a, b, dmap, case["nimages_out"], case["max_tracks_out"], case["max_obs_out"], accept=dacc,
                           fshift_a=case["fshift_a"], fshift_b=case["fshift_b"], rshift_a=case["rshift_a"],
                           rshift_b=case["rshift_b"], max_records_out=case["max_records_out"], **outs)
    ctx.sync()
    for s, dev in (("a", a), ("b", b)):
        for k, dt in MC.SCENE_ARRAYS:
            if ins[s][k] is not None:
                assert ctx.download(dev[k], ins[s][k].shape, dt).tobytes() == ins[s][k].tobytes(), (s, k, "was written")
    assert ctx.download(dmap, ins["map"].shape, np.int32).tobytes() == ins["map"].tobytes()
    if dacc is not None:
        assert ctx.download(dacc, ins["accept"].shape, np.int32).tobytes() == ins["accept"].tobytes()
    return {k: (ctx.download(outs[k], (m,), np.uint32) if outs[k] is not None else np.full(m, POISON_WORD, np.uint32))
            for k, m in sizes.items()}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_case(g, cases, name):
    """The cases of merge_cases.gpu_cases (what each is built to hit is asserted in test_merge_cpu.py)."""
    MC.compare(_merge(g, cases[name]), MC.expected_merge(cases[name]), name)


def test_merging_an_empty_scene_returns_the_other(g):
    case = MC.empty_a_case()
    MC.compare(_merge(g, case), MC.expected_merge(case), "empty A")


def test_two_runs_give_the_same_bytes(g, cases):
    for name in ("partners", "hostile", "unions, duplicates inside", "T 2049 2047"):
        first, again = _merge(g, cases[name]), _merge(g, cases[name])
        for k in MC.OUTPUTS:
            assert first[k].tobytes() == again[k].tobytes(), (name, k)


def test_one_context_after_other_calls_and_more_and_less_temp(g, cases):
    """The temp of the context is shared: the call after a filter that left it larger (24 bytes x 100 000 slots), after
    the other calls this module's context has made, and in a fresh context after a filter that left it smaller."""
    small = FC.two_view_case(3)
    big = FC.variant(small, max_obs=100000,
                     obs=np.concatenate([small["obs"], np.zeros(100000 - len(small["obs"]), TC.OBS_DTYPE)]))

    def filt(ctx, fc):
        dev = {k: ctx.upload(v) for k, v in FC.inputs(fc).items()}
        ctx.filter_tracks_batch(fc["max_tracks"], fc["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"],
                                dev["points"], dev["point_status"], fc["nimages"], dev["cam"], dev["cam_pair"],
                                fc["intrinsics"])

    filt(g, big)
    for name in ("unions", "hostile"):
        MC.compare(_merge(g, cases[name]), MC.expected_merge(cases[name]), name + ", after a larger temp")
    with guarded_context(1) as fresh:
        filt(fresh, small)
        for name in ("T 2047 2049", "partners"):
            MC.compare(_merge(fresh, cases[name]), MC.expected_merge(cases[name]), name + ", after a smaller temp")


def test_argument_errors_enqueue_nothing(g, cases):
    from cudasift_amd import capi
    L = capi.lib()
    case = cases["T 5 0"]
    held = []

    def ptr_of(a):
        if a is None:
            return None
        held.append(g.upload(a))
        return held[-1].ptr

    def alloc_out(words):
        buf = _poisoned(g, words)
        return buf, buf.ptr

    names, good, keep = bad_argument_table(case, ptr_of, alloc_out)

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_merge_scenes_batch(g.h, *[a[k] for k in names])

    for kw in keep["bad"]:
        assert call(**kw) == MISIFT_EINVAL, kw
    assert L.misift_merge_scenes_batch(None, *[good[k] for k in names]) == MISIFT_EINVAL
    g.sync()
    sizes = MC.sizes(case)
    for k, m in sizes.items():
        assert (g.download(keep["out"][k], (m,), np.uint32) == POISON_WORD).all(), k
    # the same arguments, unbroken (accept all ones)
    assert call() == MISIFT_OK
    g.sync()
    got = {k: g.download(keep["out"][k], (m,), np.uint32) for k, m in sizes.items()}
    MC.compare(got, MC.expected_merge(MC.variant(case, accept=np.ones(case["a"]["max_tracks"], np.int32))), "unbroken")


def test_correspond_align_transform_merge_triangulate(g):
    """The chain on the 8-camera scene of posegraph_cases, nothing read in between.  Scene A links and exports the pairs
    inside images 0 .. 4 and holds the cameras 0 .. 4, scene B the pairs inside images 3 .. 7 and the cameras 3 .. 7 moved
    into another gauge (a planted similarity transform); each is triangulated.  Then correspond -> align -> transform(A)
    -> merge(A into B) -> triangulate on the merged scene.  Every step is byte-equal to its restatement fed the device's
    own buffers; the merged scene holds all eight cameras, A's root among them as MISIFT_CAM_MERGED, and its points
    triangulate."""
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
    in_a = np.array([b <= 4 for a, b in sc["pairs"]])
    in_b = np.array([a >= 3 for a, b in sc["pairs"]])
    mt, mo = total // 3 + 1, total
    K = np.tile(np.array(PC.K_A, f32), (nimg, 1))
    g.sync()
    cam_all, pair_all = g.download(dcam, (nimg, 12), f32), g.download(dcam_pair, (nimg,), np.int32)
    assert (pair_all != AC.UNSET).all() and pair_all[0] == -1
    planted = AC.transform_case()["sim"]
    pair_a, pair_b = pair_all.copy(), pair_all.copy()
    pair_a[5:], pair_b[:3] = AC.UNSET, AC.UNSET
    cams = dict(a=(dcam, g.upload(pair_a)), b=(g.upload(AC.one_nan(AC.transform_cameras(planted, cam_all))), g.upload(pair_b)))
    scenes = {}
    for which, member in (("a", in_a), ("b", in_b)):
        lab = g.link_tracks_batch(pc["pairs"], d, g.upload(np.where(member, n, 0).astype(np.int32)), n, nimg, d_cnt, None,
                                  n, max_records=total, min_score=GATES[0], max_ambiguity=GATES[1],
                                  max_error=pc["max_error"])
        rec_obs = g.upload(np.full(total, -1, np.int32))         # the precondition of correspond
        doff, _, dobs, _, dsum = g.export_tracks_batch(d_recs, nimg, d_cnt, None, n, max_records=total, track=lab[0],
                                                       track_len=lab[1], track_frames=lab[2], min_len=3,
                                                       consistent_only=1, max_tracks=mt, max_obs=mo, record_obs=rec_obs)
        tri = g.triangulate_tracks_batch(mt, mo, doff, dobs, dsum, nimg, cams[which][0], cams[which][1], K, min_views=2,
                                         num_loops=5)
        scenes[which] = dict(max_tracks=mt, max_obs=mo, track_offsets=doff, obs=dobs, export_summary=dsum, points=tri[0],
                             point_views=tri[1], point_status=tri[2], nimages=nimg, cam=cams[which][0],
                             cam_pair=cams[which][1], max_records=total, record_obs=rec_obs)
    A, B = scenes["a"], scenes["b"]
    # the five steps, nothing read in between
    outs = dict(track_map=_poisoned(g, mt), csum=_poisoned(g, 8), sim=_poisoned(g, 16), cand=_poisoned(g, 1),
                inl=_poisoned(g, 1), st=_poisoned(g, 1), asum=_poisoned(g, 8), inlier=_poisoned(g, mt),
                pts=_poisoned(g, 4 * mt), cam=_poisoned(g, 12 * nimg))
    g.correspond_tracks_batch(total, A["record_obs"], mt, mo, A["track_offsets"], A["export_summary"], total,
                              B["record_obs"], mt, mo, B["track_offsets"], B["export_summary"],
                              track_map=outs["track_map"], summary=outs["csum"])
    aargs = dict(num_loops=128, thresh=0.25, min_inliers=8, refit_loops=3)
    ranges, seeds = np.array([[0, mt, 0, mt]], np.int32), np.array([77], np.uint32)
    g.align_points_batch(A["points"], B["points"], outs["track_map"], ranges, seeds, src_status=A["point_status"],
                         dst_status=B["point_status"], count=A["export_summary"].ptr + 8, count_stride=8, sim=outs["sim"],
                         align_cand=outs["cand"], align_inliers=outs["inl"], align_status=outs["st"],
                         inlier=outs["inlier"], summary=outs["asum"], **aargs)
    g.transform_scene_batch(outs["sim"], mt, A["export_summary"], A["points"], A["point_status"], nimg, A["cam"],
                            A["cam_pair"], sim_status=outs["st"], points_out=outs["pts"], cam_out=outs["cam"])
    moved = dict(A, points=outs["pts"], cam=outs["cam"])
    case_dims = dict(fshift_a=0, fshift_b=0, nimages_out=nimg, rshift_a=0, rshift_b=0, max_records_out=total,
                     max_tracks_out=2 * mt, max_obs_out=2 * mo)
    msizes = MC.sizes(dict(case_dims, a=dict(max_tracks=mt, max_obs=mo), b=dict(max_tracks=mt, max_obs=mo)))
    mouts = {k: _poisoned(g, m) for k, m in msizes.items()}
    g.merge_scenes_batch(moved, B, outs["track_map"], nimg, 2 * mt, 2 * mo, accept=outs["inlier"], max_records_out=total,
                         **mouts)
    tri_m = g.triangulate_tracks_batch(2 * mt, 2 * mo, mouts["track_offsets_out"], mouts["obs_out"],
                                       mouts["export_summary_out"], nimg, mouts["cam_out"], mouts["cam_pair_out"], K,
                                       min_views=2, num_loops=5)
    g.sync()

    def scene_host(s):
        return dict(max_tracks=mt, max_obs=mo, nimages=nimg, max_records=total,
                    track_offsets=g.download(s["track_offsets"], (mt + 1,), np.int32),
                    obs=g.download(s["obs"], (mo,), TC.OBS_DTYPE),
                    export_summary=g.download(s["export_summary"], (8,), np.int32),
                    points=g.download(s["points"], (mt, 4), f32), point_views=g.download(s["point_views"], (mt,), np.int32),
                    point_status=g.download(s["point_status"], (mt,), np.int32), cam=g.download(s["cam"], (nimg, 12), f32),
                    cam_pair=g.download(s["cam_pair"], (nimg,), np.int32),
                    record_obs=g.download(s["record_obs"], (total,), np.int32))

    ha, hb, hm = scene_host(A), scene_host(B), scene_host(moved)
    TA, TB = int(ha["export_summary"][2]), int(hb["export_summary"][2])
    # correspond
    ec = AC.expected_correspond(dict(a=ha, b=hb, shift=0))
    got_map = g.download(outs["track_map"], (mt,), np.uint32)
    assert got_map.tobytes() == ec["map"].tobytes()
    assert g.download(outs["csum"], (8,), np.uint32).tobytes() == ec["summary"].tobytes()
    cs = ec["summary"].view(np.int32)
    print("chain: T_A %d T_B %d ties %d mapped %d conflicts %d" % tuple(cs[:5]))
    assert TA > 20 and TB > 20 and cs[3] >= 10
    # align
    acase = dict(src=ha["points"], dst=hb["points"], map=got_map.view(np.int32), ranges=ranges, seeds=seeds,
                 src_status=ha["point_status"], dst_status=hb["point_status"], count=ha["export_summary"][2:],
                 count_stride=8, want_inlier=True, **aargs)
    ea = AC.expected_align(acase)
    got = dict(sim=g.download(outs["sim"], (16,), np.uint32), align_cand=g.download(outs["cand"], (1,), np.uint32),
               align_inliers=g.download(outs["inl"], (1,), np.uint32), align_status=g.download(outs["st"], (1,), np.uint32),
               summary=g.download(outs["asum"], (8,), np.uint32), inlier=g.download(outs["inlier"], (mt,), np.uint32))
    for k in got:
        assert got[k].tobytes() == ea[k].tobytes(), k
    sim = got["sim"].view(f32)
    assert ea["entries"][0]["status"] == AC.OK
    assert np.abs(sim[:9] - planted[:9]).max() < 1e-2 and abs(sim[12] - planted[12]) < 1e-2 * planted[12]
    # transform
    et = AC.expected_transform(dict(sim=sim, sim_status=0, max_tracks=mt, export_summary=ha["export_summary"],
                                    points=ha["points"], point_status=ha["point_status"], nimages=nimg, cam=ha["cam"],
                                    cam_pair=ha["cam_pair"]))
    assert hm["points"].view(np.uint32).reshape(-1).tobytes() == et["points_out"].tobytes()
    assert hm["cam"].view(np.uint32).reshape(-1).tobytes() == et["cam_out"].tobytes()
    # merge
    mcase = dict(case_dims, a=hm, b=hb, map=got_map.view(np.int32), accept=got["inlier"].view(np.int32),
                 want=dict(obs_map_a=True, obs_map_b=True, record_obs_out=True))
    em = MC.expected_merge(mcase)
    gotm = {k: g.download(mouts[k], (m,), np.uint32) for k, m in msizes.items()}
    MC.compare(gotm, em, "chain, merge")
    ms = em["summary"].view(np.int32)
    print("chain: merged T' %d O' %d, summary %s" % (ms[0], ms[1], ms.tolist()))
    assert ms[2] >= 10 and ms[3] > 0 and ms[5] > 0 and ms[6] == 0 and ms[7] == 3
    pair_m = gotm["cam_pair_out"].view(np.int32)
    assert (pair_m[:3] == MC.CAM_MERGED).all() and (pair_m[3:] == pair_b[3:]).all() and (pair_m == -1).sum() == 0
    # triangulate on the merged scene
    merged = MC.merged_scene(mcase, gotm)
    base = dict(max_tracks=2 * mt, max_obs=2 * mo, track_offsets=merged["track_offsets"], obs=merged["obs"],
                export_summary=merged["export_summary"], nimages=nimg, intrinsics=K, cam=merged["cam"],
                cam_pair=merged["cam_pair"], min_views=2, num_loops=5, memo={})
    with np.errstate(all="ignore"):
        xt = TC.expected_triangulate(base)
    gt = dict(points=g.download(tri_m[0], (8 * mt,), np.uint32), point_views=g.download(tri_m[1], (2 * mt,), np.uint32),
              point_status=g.download(tri_m[2], (2 * mt,), np.uint32), obs_error=g.download(tri_m[3], (2 * mo,), np.uint32),
              summary=g.download(tri_m[4], (8,), np.uint32))
    for k in gt:
        written = xt[k] != POISON_WORD
        assert (gt[k][written] == xt[k][written]).all(), k
    # The two scenes lie in one gauge.  A partner that align accepted has its transformed point within thresh of B's, so
    # the point triangulated from both lists under the merged cameras lies near B's own: half of them within thresh.
    tm = gotm["track_map_a"].view(np.int32)[:TA]
    both = np.nonzero((got["inlier"].view(np.int32)[:TA] == 1) & (tm >= 0))[0]
    ok = both[(gt["point_status"].view(np.int32)[tm[both]] == 0) & (hb["point_status"][tm[both]] == 0)]
    dist = np.linalg.norm(gt["points"].view(f32).reshape(-1, 4)[tm[ok], :3] - hb["points"][tm[ok], :3], axis=1)
    print("chain: %d accepted partners, distance to B's point median %.4g max %.4g" % (len(ok), np.median(dist), dist.max()))
    assert len(ok) >= 8 and np.median(dist) < aargs["thresh"]


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0

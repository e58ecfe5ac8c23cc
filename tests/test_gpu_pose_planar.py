"""misift_recover_pose_planar_batch on the device: the pose of every planar or rotation-only frame pair from its
homography, written over what misift_recover_pose_batch left, and nothing of any other entry.

Every comparison is byte equality with pose_planar_cases.expected_planar (pinned in test_pose_planar_cpu.py to the
library's host hooks and to float64): d_model, d_hf_counts, d_pose, d_num_front, d_votes, d_xyz, d_pose_alt, d_plane, and
every byte of the records and of H and F, which the call must not write.  The outputs have exactly the stated capacity
and are poisoned first, so what an entry of model 0 or -1 and a frame that is not selected keep is visible; all
allocations of the module are guarded.  The frame counts are the ones at which the kernel can go wrong: no records,
fewer than min_inliers, fewer than a wave, the workgroup's 256 threads and one more, and a third record per thread."""
import numpy as np
import pytest

import pose_cases as PC
import pose_planar_cases as PP
from batch_util import POISON_WORD, guarded_context, layout, orc, span
from test_fundamental_cpu import GATES, expected_find, f32

pytestmark = pytest.mark.gpu

MISIFT_OK, MISIFT_EINVAL = 0, -1
OPTIONAL = ("votes", "xyz", "pose_alt", "plane")


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


def _poisoned(ctx, words):
    return ctx.upload(np.full(max(words, 1), POISON_WORD, np.uint32))


def _planar(ctx, sel, K, recs, counts, offs, stride, H, F, skip=(), **kw):
    """The call on outputs of exactly the stated sizes, poisoned; those named in `skip` are NULL.  Returns a dict of the
    outputs as uint32 arrays (None for a skipped one) and the records afterwards."""
    from cudasift_amd import capi
    ns = len(sel)
    p = dict(PP.PARAMS, **kw)
    d = ctx.upload(recs)
    dc = ctx.upload(np.asarray(counts, np.int32))
    do = ctx.upload(np.asarray(offs, np.int32)) if offs is not None else None
    H, F = np.ascontiguousarray(H, f32).reshape(ns, 9), None if F is None else np.ascontiguousarray(F, f32).reshape(ns, 9)
    dH, dF = ctx.upload(H), None if F is None else ctx.upload(F)
    sizes = dict(model=ns, hf=2 * ns, pose=12 * ns, num_front=ns, votes=4 * ns, xyz=4 * len(recs), pose_alt=12 * ns,
                 plane=4 * ns)
    o = {k: (None if k in skip else _poisoned(ctx, m)) for k, m in sizes.items()}
    ctx.recover_pose_planar_batch(sel, np.stack(K), d, len(counts), dc, dH, dF, do, stride, model=o["model"],
                                  hf_counts=o["hf"], pose=o["pose"], num_front=o["num_front"], votes=o["votes"],
                                  xyz=o["xyz"], pose_alt=o["pose_alt"], plane=o["plane"], min_score=GATES[0],
                                  max_ambiguity=GATES[1], **p)
    ctx.sync()
    assert ctx.download(dH, (ns, 9), f32).tobytes() == H.tobytes()
    assert F is None or ctx.download(dF, (ns, 9), f32).tobytes() == F.tobytes()
    got = {k: (None if o[k] is None else ctx.download(o[k], (max(m, 1),), np.uint32)[:m]) for k, m in sizes.items()}
    got["recs"] = ctx.download(d, (len(recs),), capi.POINT_DTYPE)
    return got


def _expected(sel, frames, counts, H, F, K, **kw):
    with np.errstate(all="ignore"):
        return [PP.expected_planar(frames[f], counts[f], H[i], None if F is None else F[i], K[i], **kw)
                for i, f in enumerate(sel)]


def _compare(got, sel, recs, counts, offs, stride, expected, what):
    ns = len(sel)
    want = dict(model=np.array([e["model"] for e in expected], np.int32).view(np.uint32),
                hf=np.stack([e["hf"] for e in expected]).reshape(-1).view(np.uint32),
                pose=np.full((ns, 12), POISON_WORD, np.uint32), num_front=np.full(ns, POISON_WORD, np.uint32),
                votes=np.full((ns, 4), POISON_WORD, np.uint32), xyz=np.full((len(recs), 4), POISON_WORD, np.uint32),
                pose_alt=np.full((ns, 12), POISON_WORD, np.uint32), plane=np.full((ns, 4), POISON_WORD, np.uint32))
    for i, (f, e) in enumerate(zip(sel, expected)):
        if e["model"] <= 0:                                      # general or invalid: everything keeps the poison
            continue
        want["pose"][i] = e["pose"].astype(f32).view(np.uint32)
        want["pose_alt"][i] = e["pose_alt"].astype(f32).view(np.uint32)
        want["plane"][i] = e["plane"].astype(f32).view(np.uint32)
        want["num_front"][i] = e["num_front"]
        want["votes"][i] = e["votes"].view(np.uint32)
        want["xyz"][span(offs, stride, f, max(counts[f], 0))] = e["xyz"].view(np.uint32)
    for k, w in want.items():
        if got[k] is None:
            continue
        a, b = got[k].reshape(-1), w.reshape(-1)
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, (what, k, "%d words differ, first at %s" % (len(bad), bad[:8]), a[bad[:8]].view(f32),
                               b[bad[:8]].view(f32), [e["model"] for e in expected])
    assert got["recs"].tobytes() == recs.tobytes(), (what, "the records were written")


# ---- frames of every count

SIZES = [40, 0, 3, 4, 255, 256, 257, 513, 30, 7, 8]


@pytest.fixture(scope="module")
def batch():
    """frame -> records held, device count, H, F, K8.  Frame 0 holds 40 records under count -1; frame 8 is in no entry.
    The records are the first of a planted planar scene with a tenth of the points off the plane; a tenth fail the gate
    from 10 records on."""
    frames, Hs, Fs, Ks = [], [], [], []
    for f, n in enumerate(SIZES):
        s = PP.planar_scene(seed=300 + f, n=max(n, 8), baseline=0.5 if f % 2 else 0.1, off=0.1,
                            k2=PC.K_B if f % 2 else PC.K_A)
        frames.append(PC.records(s["xy"], 300 + f, fail=0.1 if n >= 10 else 0.0)[:n])
        Hs.append(s["H"])
        Fs.append(PC.planted(seed=300 + f, k2=PC.K_B if f % 2 else PC.K_A)["F"])     # some F: counted, nothing else
        Ks.append(s["K8"])
    counts = [-1] + SIZES[1:]
    sel = [7, 3, 0, 5, 1, 10, 4, 2, 6, 9]                        # not in frame order, without frame 8
    return dict(frames=frames, counts=counts, Hs=Hs, Fs=Fs, Ks=Ks, sel=sel)


def _laid_out(batch, padded):
    recs, offs, stride = layout(batch["frames"], batch["counts"], padded, min_stride=0, pad_error=-7.0)
    sel = batch["sel"]
    return (recs, offs, stride, [batch["Hs"][f] for f in sel], [batch["Fs"][f] for f in sel],
            [batch["Ks"][f] for f in sel])


@pytest.mark.parametrize("with_f", [False, True], ids=["F NULL", "F given"])
@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
def test_every_frame_count(g, batch, padded, with_f):
    recs, offs, stride, H, F, K = _laid_out(batch, padded)
    sel, counts = batch["sel"], batch["counts"]
    kw = dict(min_inliers=4, planar_ratio=0.0) if with_f else dict(min_inliers=4)
    F = F if with_f else None
    exp = _expected(sel, batch["frames"], counts, H, F, K, **kw)
    got = _planar(g, sel, K, recs, counts, offs, stride, H, F, **kw)
    _compare(got, sel, recs, counts, offs, stride, exp, "padded %s F %s" % (padded, with_f))
    by_frame = {f: e for f, e in zip(sel, exp)}
    for f in (0, 1, 2):                                          # count -1, 0 and 3: below min_inliers
        assert by_frame[f]["model"] == PP.GENERAL and by_frame[f]["hf"][0] == max(counts[f], 0) * (f == 2)
    for f in (3, 4, 5, 6, 7, 10):
        assert by_frame[f]["model"] == PP.PLANE, (f, by_frame[f]["model"], by_frame[f]["hf"])
    if with_f:
        assert any(e["hf"][1] > 0 for e in exp)


def test_optional_outputs_and_two_runs(g, batch):
    """Each optional output NULL, one at a time and all four: the other outputs do not change; two runs are identical."""
    recs, offs, stride, H, F, K = _laid_out(batch, False)
    sel, counts = batch["sel"], batch["counts"]
    exp = _expected(sel, batch["frames"], counts, H, None, K, min_inliers=4)
    full = _planar(g, sel, K, recs, counts, offs, stride, H, None, min_inliers=4)
    again = _planar(g, sel, K, recs, counts, offs, stride, H, None, min_inliers=4)
    for k in full:
        assert full[k].tobytes() == again[k].tobytes(), k
    for skip in [(k,) for k in OPTIONAL] + [OPTIONAL]:
        got = _planar(g, sel, K, recs, counts, offs, stride, H, None, skip=skip, min_inliers=4)
        _compare(got, sel, recs, counts, offs, stride, exp, "without %s" % (skip,))


# ---- the four models in one call

def mixed_case():
    """Five entries: planar, general (a cloud under a fitted H), invalid (a rank-1 H that every record fits), rotation
    only, planar again; a sixth frame is not selected."""
    a, b = PP.scene(0.5, 0.1, 3), PP.scene(0.1, 0.0, 4)
    gen = PP.planar_scene(seed=7, general=True, n=300)
    rot = PP.planar_scene(seed=7, baseline=0.0, n=257)
    xy = PC.coordinates(a["recs"], 60).copy()
    xy[:, 2:] = [3, 2]                                           # every match at (3, 2): the rank-1 H takes them all
    flat = PC.records(xy, 41)
    rank1 = np.array([0, 0, 3, 0, 0, 2, 0, 0, 1], f32)
    frames = [a["recs"][:300], gen["recs"], flat, rot["recs"], b["recs"][:100], a["recs"][:50]]
    H = [a["H"], gen["H"], rank1, rot["H"], b["H"]]
    K = [a["K8"], gen["K8"], a["K8"], rot["K8"], b["K8"]]
    with np.errstate(all="ignore"):
        F = [expected_find(frames[i], len(frames[i]), 5 + i, 64, *GATES, PP.THRESH_F, max_pts=513)[0] for i in range(5)]
    return frames, H, F, K


def test_four_models_in_one_call(g):
    frames, H, F, K = mixed_case()
    counts = [len(f) for f in frames]
    sel = [0, 1, 2, 3, 4]
    for with_f, padded in ((True, False), (False, True)):
        recs, offs, stride = layout(frames, counts, padded, min_stride=0, pad_error=0.0)
        Fs = F if with_f else None
        exp = _expected(sel, frames, counts, H, Fs, K)
        models = [e["model"] for e in exp]
        assert models == [PP.PLANE, PP.GENERAL, PP.INVALID, PP.ROTATION, PP.PLANE], (models, [e["hf"] for e in exp])
        got = _planar(g, sel, K, recs, counts, offs, stride, H, Fs)
        _compare(got, sel, recs, counts, offs, stride, exp, "mixed, F %s" % with_f)
        rot = span(offs, stride, 3, counts[3])
        assert (got["xyz"].reshape(-1, 4)[rot] == PC.NAN_BITS).all() and got["num_front"][3] == 0
        for f in (1, 2, 5):                                      # general, invalid, not selected: the poison stays
            assert (got["xyz"].reshape(-1, 4)[span(offs, stride, f, counts[f])] == POISON_WORD).all()


def test_decision_at_the_thresholds(g):
    """(float)nH exactly planar_ratio * nF (8 against 16 at 0.5) is planar, one ulp of planar_ratio above is general; nH
    one below, at and above min_inliers.  Byte for byte, d_model first."""
    r16, H, F, K8 = PP.ratio_frame()
    tie = PP.tie_frame()[0]
    th = dict(thresh_h=1e-3, thresh_f=1e-3)
    above = float(np.nextafter(f32(0.5), f32(1)))
    for frames, counts, Fs, kw, models, hf in (
            ([r16], [16], [F], dict(planar_ratio=0.5, **th), [PP.PLANE], [[8, 16]]),
            ([r16], [16], [F], dict(planar_ratio=above, **th), [PP.GENERAL], [[8, 16]]),
            ([r16, r16.copy()], [16, 15], [F, F], dict(planar_ratio=0.5, **th), [PP.PLANE, PP.PLANE], [[8, 16], [8, 15]]),
            ([tie[:7], tie[:8], tie[:9]], [7, 8, 9], None, dict(min_inliers=8, **th),
             [PP.GENERAL, PP.PLANE, PP.PLANE], [[7, 0], [8, 0], [9, 0]])):
        ns = len(frames)
        sel = list(range(ns))
        recs, offs, stride = layout(frames, counts, False, min_stride=0, pad_error=0.0)
        exp = _expected(sel, frames, counts, [H] * ns, Fs, [K8] * ns, **kw)
        assert [e["model"] for e in exp] == models and [e["hf"].tolist() for e in exp] == hf, (kw, exp)
        got = _planar(g, sel, [K8] * ns, recs, counts, offs, stride, [H] * ns, Fs, **kw)
        assert got["model"].view(np.int32).tolist() == models and got["hf"].view(np.int32).reshape(-1, 2).tolist() == hf
        _compare(got, sel, recs, counts, offs, stride, exp, "decision %s" % (kw,))


def test_hostile_inputs(g):
    """The CPU file's hostile H and K, each over the same 70 records, then its hostile record sets."""
    cases = PP.hostile_matrices() + PP.baseline_edges()
    s = PP.scene(0.5, 0.0, 0)
    fr = [s["recs"][:70].copy() for _ in cases]
    counts = [70] * len(cases)
    recs, offs, stride = layout(fr, counts, False, min_stride=0, pad_error=0.0)
    sel = list(range(len(cases)))[::-1]
    H, K = [cases[f][1] for f in sel], [cases[f][2] for f in sel]
    for mb in sorted({float(c[3]) for c in cases}):              # one call per min_baseline; min_inliers 4 and a huge
        mine = [i for i, f in enumerate(sel) if float(cases[f][3]) == mb]          # thresh_h let every finite H through
        kw = dict(min_baseline=mb, min_inliers=4, thresh_h=1e18)
        sub = [sel[i] for i in mine]
        exp = _expected(sub, fr, counts, [H[i] for i in mine], None, [K[i] for i in mine], **kw)
        got = _planar(g, sub, [K[i] for i in mine], recs, counts, offs, stride, [H[i] for i in mine], None, **kw)
        _compare(got, sub, recs, counts, offs, stride, exp, "hostile H, min_baseline %g" % mb)
        for f, e in zip(sub, exp):
            want = cases[f][4]
            if e["hf"][0] >= 4 and want is not None:
                assert e["model"] == want, (cases[f][0], e["model"], e["hf"])
    seen = set()
    for name, (recs1, H1, K1), kw in (("non-finite positions", PP.hostile_frame(), {}),
                                      ("deno = 0", PP.deno0_frame(), dict(thresh_h=1e-3, thresh_f=1e-3, min_inliers=4)),
                                      ("a tie", PP.tie_frame(), dict(thresh_h=1e-3, thresh_f=1e-3))):
        counts1 = [len(recs1)]
        r, offs, stride = layout([recs1], counts1, True, min_stride=0, pad_error=0.0)
        exp = _expected([0], [recs1], counts1, [H1], None, [K1], **kw)
        got = _planar(g, [0], [K1], r, counts1, offs, stride, [H1], None, **kw)
        _compare(got, [0], r, counts1, offs, stride, exp, name)
        seen.add(exp[0]["model"])
    assert PP.PLANE in seen


def test_on_a_used_context(batch):
    """The call on a context that other batch calls have used before: find_fundamental, improve_fundamental and
    recover_pose over a larger batch first."""
    c = PC.expected_chain()
    s, n = c["scene"], PC.CHAIN["n"]
    with guarded_context(1) as ctx:
        d, dc = ctx.upload(s["recs"]), ctx.upload(np.array([n], np.int32))
        gates = dict(min_score=GATES[0], max_ambiguity=GATES[1], thresh=1.0)
        dF, _ = ctx.find_fundamental_batch([0], [9], d, 1, dc, None, n, max_pts=n, num_loops=64, **gates)
        ctx.improve_fundamental_batch([0], d, 1, dc, dF, None, n, num_loops=2, **gates)
        ctx.recover_pose_batch([0], s["K8"], d, 1, dc, dF, None, n, **gates)
        recs, offs, stride, H, F, K = _laid_out(batch, False)
        sel, counts = batch["sel"], batch["counts"]
        exp = _expected(sel, batch["frames"], counts, H, None, K, min_inliers=4)
        got = _planar(ctx, sel, K, recs, counts, offs, stride, H, None, min_inliers=4)
        _compare(got, sel, recs, counts, offs, stride, exp, "used context")


# ---- the chain

CHAIN = dict(n=400, find_loops=256, improve_loops=5, thresh=1.0, h_loops=256, h_thresh=3.0)


def chain_scene():
    """Three images of 400 points, half of them on a plane, each point with a descriptor of its own.  Camera 1 is camera
    0 moved, camera 2 is camera 1 turned about its centre.  Images 0 and 2 hold all points, image 1 the plane's alone, each
    in an order of its own.  Pair 0 = (0, 2) sees all points; pair 1 = (0, 1), the middle one, matches the plane alone
    (the other rows of image 0 find no descriptor above the gate); pair 2 = (1, 2) rotates only.
    dict(images: the records of each image, pairs, cams, K8)."""
    from cudasift_amd import capi
    rng = np.random.default_rng(77)
    n = CHAIN["n"]
    K = PC.kmat(PC.K_A)
    N = PC.rodrigues([1, 0.5, 0], 0.3) @ np.array([0, 0, 1.0])
    px = np.stack([rng.uniform(300, 1620, n), rng.uniform(150, 930, n), np.ones(n)], 1)
    rays = (np.linalg.inv(K) @ px.T).T
    X = rays * (6.0 * N[2] / (rays @ N))[:, None]
    on = np.arange(n) < n // 2
    X[~on] = rays[~on] * rng.uniform(4, 9, (~on).sum())[:, None]
    R1, c1 = PC.rodrigues([0.1, 1, 0.2], 0.08), np.array([1.2, 0.2, 0.3])
    R2 = PC.rodrigues([0.2, 1, -0.1], 0.12) @ R1
    cams = [(np.eye(3), np.zeros(3)), (R1, -R1 @ c1), (R2, -R2 @ c1)]
    desc = rng.normal(0, 1, (n, 128))
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(f32)
    images = []
    for i, (R, t) in enumerate(cams):
        x = (K @ ((R @ X.T).T + t).T).T
        o = x[:, :2] / x[:, 2:] + rng.normal(0, 0.5, (n, 2))
        points = rng.permutation(np.nonzero(on)[0] if i == 1 else np.arange(n))     # record j holds points[j]
        r = np.zeros(len(points), capi.POINT_DTYPE)
        r["data"], r["xpos"], r["ypos"], r["match"] = desc[points], o[points, 0], o[points, 1], -2
        images.append(r)
    return dict(images=images, pairs=[(0, 2), (0, 1), (1, 2)], cams=cams, K8=np.array(PC.K_A + PC.K_A, f32))


def test_chain_upgrades_the_planar_pair(g):
    """match_pairs -> find_homography -> improve_homography and find_fundamental -> improve_fundamental -> recover_pose
    -> recover_pose_planar -> link_poses on the three-image scene, nothing read in between.  Each step equals its
    restatement (the oracle's matcher for the match, the single-frame homography calls for the two homography steps);
    the planar pair's camera in d_cam is the upgraded one; the linker skips the rotation-only pair."""
    import posegraph_cases as G
    from batch_util import OUT_FIELDS, expected_pair
    from cudasift_amd import capi
    from test_fundamental_refine_cpu import expected_improve
    from test_gpu_posegraph import _sizes
    from test_pose_cpu import direction_error, rotation_error
    sc = chain_scene()
    mp, npairs, C = CHAIN["n"], 3, CHAIN
    sel, seeds = [0, 1, 2], [11, 12, 13]
    K8 = np.tile(sc["K8"], (npairs, 1))
    hg = dict(min_score=GATES[0], max_ambiguity=GATES[1], thresh=C["h_thresh"])
    fg = dict(min_score=GATES[0], max_ambiguity=GATES[1], thresh=C["thresh"])
    pk = dict(PP.PARAMS, thresh_h=C["h_thresh"], thresh_f=C["thresh"])
    sizes = [len(r) for r in sc["images"]]
    counts = [sizes[a] for a, _ in sc["pairs"]]                  # a row per set-1 record
    # the restatements, pair by pair; the rows start as zeros, the matcher writes seven fields of each
    all_rows = np.zeros(npairs * mp, capi.POINT_DTYPE)
    Hs, Fs, poses, planar = [], [], [], []
    for p, (a, b) in enumerate(sc["pairs"]):
        n = counts[p]
        m, _ = expected_pair(sc["images"][a], sc["images"][b], False, False, False)
        r = np.zeros(n, capi.POINT_DTYPE)
        for k in OUT_FIELDS:
            r[k] = m[k]
        d1 = g.upload(r)
        orc().srand(seeds[p])
        H0, _ = g.find_homography(d1.ptr, n, num_loops=C["h_loops"], **hg)
        H, _ = g.improve_homography(d1.ptr, n, H0, 5, **hg)
        r = g.download(d1, (n,), capi.POINT_DTYPE)
        with np.errstate(all="ignore"):
            F0, _ = expected_find(r, n, seeds[p], C["find_loops"], *GATES, C["thresh"], max_pts=mp)
            r, F, _, _ = expected_improve(r, n, F0, C["improve_loops"], *GATES, C["thresh"])
            poses.append(PC.expected_pose(r, n, F, sc["K8"], *GATES, C["thresh"]))
            planar.append(PP.expected_planar(r, n, np.asarray(H, f32).reshape(9), F, sc["K8"], **pk))
        all_rows[p * mp:p * mp + n] = r
        Hs.append(np.asarray(H, f32).reshape(9)), Fs.append(F)
    assert [e["model"] for e in planar] == [PP.GENERAL, PP.PLANE, PP.ROTATION], [(e["model"], e["hf"]) for e in planar]
    final = [e if e["model"] > 0 else q for e, q in zip(planar, poses)]
    pose = np.stack([e["pose"] for e in final]).astype(f32)
    front = np.array([e["num_front"] for e in final], np.int32)
    xyz = np.full((npairs * mp, 4), POISON_WORD, np.uint32)
    for p, e in enumerate(final):
        xyz[p * mp:p * mp + counts[p]] = e["xyz"].view(np.uint32)
    case = dict(pairs=np.array(sc["pairs"], np.int32), nimages=3, rows=all_rows, row_counts=np.array(counts, np.int32),
                max_pts=mp, max_error=2.0, pose=pose, num_front=front, xyz=xyz.view(f32),
                links=np.array([(0, 1, G.FAN), (1, 2, G.CHAIN)], np.int32), seed_pair=0, root_image=0,
                min_common=G.MIN_COMMON, walk=np.array([1, 0, 2], np.int32))
    with np.errstate(all="ignore"):
        e = G.expected_link_poses(case)
    # the device
    recs, offs, _ = layout(sc["images"], sizes, False, min_stride=0, pad_error=0.0)
    dimg, dic, dio = g.upload(recs), g.upload(np.array(sizes, np.int32)), g.upload(np.asarray(offs, np.int32))
    d = g.upload(np.zeros(npairs * mp, capi.POINT_DTYPE))
    dc = _poisoned(g, npairs)
    dpose, dfront, dxyz, dmodel, dhf, dalt, dplane = (_poisoned(g, k) for k in (36, 3, 4 * mp * npairs, 3, 6, 36, 12))
    outs = {k: _poisoned(g, m) for k, m in _sizes(case).items()}
    g.match_pairs_batch(sc["pairs"], dimg, 3, dic, dio, 0, max_pts=mp, out=d, out_counts=dc)
    dH, _ = g.find_homography_batch(sel, seeds, d, npairs, dc, None, mp, max_pts=mp, num_loops=C["h_loops"], **hg)
    g.improve_homography_batch(sel, d, npairs, dc, dH, None, mp, num_loops=5, **hg)
    dF, _ = g.find_fundamental_batch(sel, seeds, d, npairs, dc, None, mp, max_pts=mp, num_loops=C["find_loops"], **fg)
    g.improve_fundamental_batch(sel, d, npairs, dc, dF, None, mp, num_loops=C["improve_loops"], **fg)
    g.recover_pose_batch(sel, K8, d, npairs, dc, dF, None, mp, pose=dpose, num_front=dfront, xyz=dxyz, **fg)
    g.recover_pose_planar_batch(sel, K8, d, npairs, dc, dH, dF, None, mp, model=dmodel, hf_counts=dhf, pose=dpose,
                                num_front=dfront, xyz=dxyz, pose_alt=dalt, plane=dplane, min_score=GATES[0],
                                max_ambiguity=GATES[1], **pk)
    g.link_poses_batch(case["pairs"], 3, d, dc, mp, dpose, dfront, dxyz, case["links"], 0, 0, case["walk"],
                       min_common=case["min_common"], min_score=GATES[0], max_ambiguity=GATES[1], max_error=2.0, **outs)
    g.sync()
    assert g.download(dc, (npairs,), np.int32).tolist() == counts
    assert g.download(dH, (npairs, 9), f32).tobytes() == np.stack(Hs).tobytes()
    assert g.download(dF, (npairs, 9), f32).tobytes() == np.stack(Fs).tobytes()
    assert g.download(d, (mp * npairs,), capi.POINT_DTYPE).tobytes() == all_rows.tobytes()
    assert g.download(dmodel, (3,), np.int32).tolist() == [e2["model"] for e2 in planar]
    assert g.download(dhf, (3, 2), np.int32).tolist() == [e2["hf"].tolist() for e2 in planar]
    assert g.download(dpose, (npairs, 12), f32).tobytes() == pose.tobytes()
    assert g.download(dfront, (npairs,), np.int32).tolist() == front.tolist()
    assert g.download(dxyz, (npairs * mp, 4), np.uint32).tobytes() == xyz.tobytes()
    assert (g.download(dalt, (3, 12), np.uint32)[0] == POISON_WORD).all()
    assert g.download(dalt, (3, 12), f32)[1].tobytes() == planar[1]["pose_alt"].astype(f32).tobytes()
    for k, m in _sizes(case).items():
        got = g.download(outs[k], (max(m, 1),), np.uint32)[:m]
        assert got.tobytes() == np.ascontiguousarray(e[k]).view(np.uint32).reshape(-1).tobytes(), k
    # what the chain is for
    (R1, t1) = sc["cams"][1]
    tdir = t1 / np.linalg.norm(t1)
    old, new = poses[1]["pose"], planar[1]["pose"]
    print("planar pair: %s H- and F-inliers; F path rotation %.3g direction %.3g; planar call %.3g %.3g, votes %s" % (
        planar[1]["hf"].tolist(), rotation_error(old[:9], R1), direction_error(old[9:], tdir),
        rotation_error(new[:9], R1), direction_error(new[9:], tdir), planar[1]["votes"].tolist()))
    assert direction_error(old[9:], tdir) > 0.5                  # the F path's confident wrong pose (CPU file)
    assert rotation_error(new[:9], R1) < 0.01 and direction_error(new[9:], tdir) < 0.05
    cam = g.download(outs["cam"], (3, 12), f32)                  # image 1 is placed by the planar pair from the root
    assert rotation_error(cam[1, :9], R1) < 0.01
    assert direction_error(cam[1, 9:] / np.linalg.norm(cam[1, 9:].astype(np.float64)), tdir) < 0.05
    summary = g.download(outs["summary"], (8,), np.int32)
    cam_pair = g.download(outs["cam_pair"], (3,), np.int32)
    assert cam_pair.tolist() == [-1, 1, 0] and front[2] == 0     # image 2 by pair 0: the rotation-only pair is skipped
    assert summary[1] == 2 and summary[2] == 3 and e["pair_scale"][2] == 0, summary


# ---- argument errors

def test_argument_errors_enqueue_nothing(g, batch):
    from cudasift_amd import capi
    L = capi.lib()
    fa, fb = batch["frames"][10], batch["frames"][4]             # two frames of 8 and 255 records
    recs = np.concatenate([fa, fb])
    nr = len(recs)
    d, dc = g.upload(recs), g.upload(np.array([8, 255], np.int32))
    do = g.upload(np.array([0, 8, nr], np.int32))
    dH = g.upload(np.stack([batch["Hs"][10], batch["Hs"][4]]))
    dF = g.upload(np.stack([batch["Fs"][10], batch["Fs"][4]]))
    sizes = dict(model=2, hf=4, pose=24, front=2, votes=8, xyz=4 * nr, alt=24, plane=8)
    o = {k: _poisoned(g, m) for k, m in sizes.items()}
    fr = np.array([0, 1], np.int32)
    K = np.stack([batch["Ks"][10], batch["Ks"][4]])
    good = dict(ctx=g.h, nsel=2, frames=fr.ctypes.data, K=K.ctypes.data, recs=d.ptr, nframes=2, counts=dc.ptr,
                offsets=do.ptr, stride=0, min_score=0.85, max_ambiguity=0.95, thresh_h=3.0, thresh_f=3.0,
                planar_ratio=0.0, min_inliers=4, min_baseline=0.02, H=dH.ptr, F=dF.ptr,
                **{k: o[k].ptr for k in sizes})

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_recover_pose_planar_batch(*[a[k] for k in good])

    nan = float("nan")
    lists = [np.array(v, np.int32) for v in ([0, 2], [-1, 1], [1, 1])]
    bad = [dict(ctx=None), dict(nsel=-1), dict(recs=None), dict(counts=None), dict(offsets=None, stride=-1),
           dict(frames=None), dict(nframes=0), dict(K=None)]
    bad += [dict(frames=v.ctypes.data) for v in lists]
    bad += [{k: None} for k in ("H", "model", "hf", "pose", "front")]
    bad += [{k: v} for k in ("thresh_h", "thresh_f") for v in (nan, 0.0, -1.0)]
    bad += [dict(planar_ratio=nan), dict(planar_ratio=-0.5), dict(min_inliers=3), dict(min_inliers=0),
            dict(min_inliers=-1), dict(min_baseline=nan), dict(min_baseline=-1e-3)]
    broken = []
    for entry in (0, 1):
        for col in range(8):
            for v in ((0.0, -1.0, np.nan, np.inf, -np.inf) if col % 4 < 2 else (np.nan, np.inf, -np.inf)):
                k = K.copy()
                k[entry, col] = v
                broken.append(k)
    bad += [dict(K=k.ctypes.data) for k in broken]
    for kw in bad:
        assert call(**kw) == MISIFT_EINVAL, kw
    assert call(nsel=0) == MISIFT_OK                             # nothing happens
    assert call(nsel=0, K=None, H=None, model=None, hf=None, pose=None, front=None) == MISIFT_OK
    g.sync()
    for k, m in sizes.items():
        assert (g.download(o[k], (m,), np.uint32) == POISON_WORD).all(), k
    assert g.download(d, (nr,), capi.POINT_DTYPE).tobytes() == recs.tobytes()
    # the edges that are allowed, then the same arguments, unbroken
    assert call(planar_ratio=0.0, min_baseline=0.0, F=None, votes=None, xyz=None, alt=None, plane=None) == MISIFT_OK
    assert call() == MISIFT_OK
    g.sync()
    model = g.download(o["model"], (2,), np.int32)
    assert model.tolist() == [PP.PLANE, PP.PLANE], model
    hf = g.download(o["hf"], (2, 2), np.int32)
    assert hf[0, 0] >= 6 and hf[1, 0] >= 150, hf
    assert (g.download(o["xyz"], (4 * nr,), np.uint32) != POISON_WORD).all()


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0

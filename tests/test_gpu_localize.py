"""misift_describe_points_batch and misift_localize_frames_batch on the device: a descriptor per track point as a frame
the int8 matcher takes, and the camera of a new image by batch RANSAC over 2-D/3-D matches, its inliers emitted as a scene
for misift_merge_scenes_batch.

Every comparison is byte equality with localize_cases.expected_describe / expected_localize (pinned in
test_localize_cpu.py to the library's host hooks, where the premises of the cases are asserted too).  The outputs have
exactly the stated sizes and are poisoned first, so what the call must leave untouched is compared as well; every input is
compared after the call; all allocations of the module are guarded.  The scenes are planted directly; no images are
needed."""
import numpy as np
import pytest

import batch_util as BU
import localize_cases as L
import merge_cases as MC
import refine_cases as RC
import resect_cases as C
import triangulate_cases as TC
from batch_util import POISON_WORD, guarded_context
from test_fundamental_cpu import f32

pytestmark = pytest.mark.gpu

MISIFT_OK, MISIFT_EINVAL = 0, -1
assert POISON_WORD == L.POISON_WORD


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


def _poisoned(ctx, words):
    return ctx.upload(np.full(max(words, 1), POISON_WORD, np.uint32))


def _same(got, e, keys, what):
    for k in keys:
        bad = np.nonzero(got[k] != e[k])[0]
        assert len(bad) == 0, (what, k, "%d words differ, first %s" % (len(bad), bad[:8]), got[k][bad[:4]], e[k][bad[:4]])


# ---- describe

def _describe(ctx, case):
    """The call on poisoned outputs of exactly the stated sizes, as uint32 arrays; the inputs must come back as they went."""
    ins = L.describe_inputs(case)
    dev = {k: ctx.upload(v) for k, v in ins.items()}
    outs = {k: _poisoned(ctx, n) for k, n in L.describe_sizes(case).items()}
    ctx.describe_points_batch(case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"],
                              dev["points"], dev["point_status"], dev["q"], case["nframes"], dev["counts"],
                              dev["offsets"] if case["offsets"] is not None else None, case["stride"],
                              case["max_records"], **outs)
    ctx.sync()
    for k, v in ins.items():
        assert ctx.download(dev[k], v.shape, v.dtype).tobytes() == v.tobytes(), (k, "was written")
    return {k: ctx.download(outs[k], (n,), np.uint32) for k, n in L.describe_sizes(case).items()}


@pytest.mark.parametrize("name", L.DESCRIBE_GPU_CASES)
def test_describe_case(g, name):
    case = L.describe_gpu_cases()[name]
    got = _describe(g, case)
    _same(got, L.expected_describe(case), L.DESCRIBE_OUTPUTS, name)
    print(name, "summary", got["summary"].view(np.int32).tolist())


def test_describe_two_runs_same_bytes(g):
    case = L.describe_gpu_cases()["hostile packed"]
    a, b = _describe(g, case), _describe(g, case)
    for k in L.DESCRIBE_OUTPUTS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_describe_argument_errors_enqueue_nothing(g):
    from cudasift_amd import capi
    lib = capi.lib()
    case = L.describe_gpu_cases()["lengths packed"]
    ins = L.describe_inputs(case)
    dev = {k: g.upload(v) for k, v in ins.items()}
    sizes = L.describe_sizes(case)
    outs = {k: _poisoned(g, n) for k, n in sizes.items()}
    names = ("ctx", "max_tracks", "max_obs", "track_offsets", "obs", "export_summary", "points", "point_status", "q",
             "nframes", "counts", "offsets", "stride", "max_records") + L.DESCRIBE_OUTPUTS
    good = dict(ctx=g.h, max_tracks=case["max_tracks"], max_obs=case["max_obs"], nframes=case["nframes"],
                stride=case["stride"], max_records=case["max_records"], **{k: dev[k].ptr for k in ins},
                **{k: outs[k].ptr for k in outs})

    def call(**kw):
        a = dict(good, **kw)
        return lib.misift_describe_points_batch(*[a[k] for k in names])

    bad = [dict(ctx=None), dict(max_tracks=0), dict(max_tracks=-1), dict(max_obs=0), dict(max_obs=-3), dict(max_records=0),
           dict(max_records=-1), dict(nframes=-1), dict(offsets=None, stride=-1)]
    bad += [{k: None} for k in ("track_offsets", "obs", "export_summary", "points", "point_status", "q", "counts") +
            L.DESCRIBE_OUTPUTS]
    bad += [{k: good[k] + d} for k in ("obs", "q", "scene_q", "scene_recs") for d in (4, 8)]
    # every output over every input and every other output, at the first and at the last byte of the other
    spans = dict(scene_q=128 * case["max_tracks"], scene_recs=576 * case["max_tracks"], scene_count=4,
                 point_members=4 * case["max_tracks"], summary=32, track_offsets=4 * (case["max_tracks"] + 1),
                 obs=16 * case["max_obs"], export_summary=32, points=16 * case["max_tracks"],
                 point_status=4 * case["max_tracks"], q=128 * case["max_records"], counts=4 * case["nframes"],
                 offsets=4 * case["nframes"])
    for o in L.DESCRIBE_OUTPUTS:
        for other, n in spans.items():
            if other == o:
                continue
            bad.append({o: good[other]})
            bad.append({o: good[other] + (n - 16 if n > 16 else 0)})
    for kw in bad:
        assert call(**kw) == MISIFT_EINVAL, kw
    g.sync()
    for k, n in sizes.items():
        assert (g.download(outs[k], (n,), np.uint32) == POISON_WORD).all(), k
    assert call() == MISIFT_OK
    g.sync()
    got = {k: g.download(outs[k], (n,), np.uint32) for k, n in sizes.items()}
    _same(got, L.expected_describe(case), L.DESCRIBE_OUTPUTS, "unbroken")


# ---- localise

LOC_INPUTS = ("rows", "counts", "offsets", "export_summary", "points", "point_status")


def _loc_inputs(case):
    ins = dict(rows=np.ascontiguousarray(case["rows"]), counts=np.ascontiguousarray(case["counts"], np.int32),
               offsets=np.ascontiguousarray(case["offsets"] if case["offsets"] is not None else [0], np.int32),
               export_summary=np.ascontiguousarray(case["export_summary"], np.int32),
               points=np.ascontiguousarray(case["points"], f32).reshape(-1, 4),
               point_status=np.ascontiguousarray(case["point_status"], np.int32),
               cam=np.ascontiguousarray(case["cam"], f32).reshape(-1, 12),
               cam_pair=np.ascontiguousarray(case["cam_pair"], np.int32))
    assert len(ins["points"]) == case["max_tracks"] == len(ins["point_status"]) and len(ins["cam"]) == case["nimages"]
    return ins


def _loc_call(ctx, case, dev, outs):
    return ctx.localize_frames_batch(
        dev["rows"], case["nframes_rows"], dev["counts"], dev["offsets"] if case["offsets"] is not None else None,
        case["stride"], case["max_tracks"], dev["export_summary"], dev["points"], dev["point_status"], case["nimages"],
        case["intrinsics"], case["frames"], case["images"], case["seeds"], case["max_pts"], case["max_found"],
        min_score=case["min_score"], max_ambiguity=case["max_ambiguity"], num_loops=case["num_loops"],
        thresh=case["thresh"], min_inliers=case["min_inliers"], only_unset=case["only_unset"], install=case["install"],
        cam=dev["cam"], cam_pair=dev["cam_pair"], **outs)


def _localize(ctx, case):
    ins = _loc_inputs(case)
    dev = {k: ctx.upload(v) for k, v in ins.items()}
    sizes = L.localize_sizes(case)
    outs = {k: _poisoned(ctx, n) for k, n in sizes.items()}
    _loc_call(ctx, case, dev, outs)
    ctx.sync()
    for k in LOC_INPUTS:
        assert ctx.download(dev[k], ins[k].shape, ins[k].dtype).tobytes() == ins[k].tobytes(), (k, "was written")
    got = {k: ctx.download(outs[k], (n,), np.uint32) if n else np.zeros(0, np.uint32) for k, n in sizes.items()}
    for k, n in sizes.items():
        if n == 0:
            assert ctx.download(outs[k], (1,), np.uint32)[0] == POISON_WORD, k
    got["cam"] = ctx.download(dev["cam"], (12 * case["nimages"],), np.uint32)
    got["cam_pair"] = ctx.download(dev["cam_pair"], (case["nimages"],), np.uint32)
    return got


@pytest.mark.parametrize("name", L.LOCALIZE_GPU_CASES)
def test_localize_case(g, name):
    case = L.localize_gpu_cases()[name]
    e = L.expected_localize(case)
    _same(_localize(g, case), e, L.LOCALIZE_OUTPUTS + ("cam", "cam_pair"), name)
    print(name, "status", [x["status"] for x in e["entries"]], "candidates", [x["cand"] for x in e["entries"]],
          "inliers", [x["inliers"] for x in e["entries"]], "finds", e["N"])


def _device_resect(ctx, rcase):
    dev = {k: ctx.upload(np.ascontiguousarray(rcase[k])) for k in ("track_offsets", "obs", "export_summary", "points",
                                                                   "point_status", "cam", "cam_pair")}
    res = ctx.resect_cameras_batch(rcase["max_tracks"], rcase["max_obs"], dev["track_offsets"], dev["obs"],
                                   dev["export_summary"], dev["points"], dev["point_status"], rcase["nimages"],
                                   rcase["intrinsics"], rcase["images"], rcase["seeds"], rcase["max_cand"],
                                   num_loops=rcase["num_loops"], thresh=rcase["thresh"], min_inliers=rcase["min_inliers"],
                                   only_unset=rcase["only_unset"], install=rcase["install"], cam=dev["cam"],
                                   cam_pair=dev["cam_pair"])
    ctx.sync()
    n = len(rcase["images"])
    return [ctx.download(res[j], (m,), np.uint32) for j, m in enumerate((12 * n, n, n, n))]


def test_same_camera_as_resect_on_the_device(g):
    """A frame whose rows are the candidates resect gathers: the device's localise and the device's resect give the same
    twelve floats, candidates, inliers and status."""
    for name in ("candidates 513 1025", "seed a", "tie"):
        case = L.localize_gpu_cases()["resect: " + name]
        res = _device_resect(g, case["resect"])
        got = _localize(g, case)
        for k, r in zip(("res_cam", "res_cand", "res_inliers", "res_status"), res):
            assert got[k].tobytes() == r.tobytes(), (name, k)


def test_shared_temp_behind_other_calls():
    """The temp is the context's: sized as the header states on a fresh context, and the same bytes behind a larger and
    behind a smaller resection that left it dirty."""
    cases = L.localize_gpu_cases()
    case = cases["hostile packed"]
    with guarded_context(1) as ctx:
        first = _localize(ctx, case)
        nsel, cap, lp = len(case["frames"]), -(-case["max_pts"] // 16) * 16, -(-case["num_loops"] // 16) * 16
        assert ctx.test_state(0) == nsel * (24 * cap + 76 * lp + 24)
        _same(first, L.expected_localize(case), L.LOCALIZE_OUTPUTS, "fresh")
        big, small = C.gpu_cases()["candidates 513 1025"], C.gpu_cases()["num_loops 1"]
        _device_resect(ctx, big)
        assert ctx.test_state(0) > nsel * (24 * cap + 76 * lp + 24)
        second = _localize(ctx, case)
        _device_resect(ctx, small)
        third = _localize(ctx, case)
        other = cases["max_pts 1030"]
        _same(_localize(ctx, other), L.expected_localize(other), L.LOCALIZE_OUTPUTS, "other strides")
        fourth = _localize(ctx, case)
        for k in first:
            assert first[k].tobytes() == second[k].tobytes() == third[k].tobytes() == fourth[k].tobytes(), k


def test_localize_argument_errors_enqueue_nothing(g):
    from cudasift_amd import capi
    lib = capi.lib()
    case = L.localize_gpu_cases()["resect: only_unset, install 1"]
    ins = _loc_inputs(case)
    dev = {k: g.upload(v) for k, v in ins.items()}
    sizes = L.localize_sizes(case)
    outs = {k: _poisoned(g, n) for k, n in sizes.items()}
    K = np.ascontiguousarray(case["intrinsics"], f32)
    n, nf = case["nimages"], case["nframes_rows"]
    frames, images = np.ascontiguousarray(case["frames"], np.int32), np.ascontiguousarray(case["images"], np.int32)
    seeds = np.ascontiguousarray(case["seeds"], np.uint32)
    names = ("ctx", "rows", "nframes_rows", "counts", "offsets", "stride", "max_tracks", "export_summary", "points",
             "point_status", "nimages", "intrinsics", "nsel", "frames", "images", "seeds", "max_pts", "min_score",
             "max_ambiguity", "num_loops", "thresh", "min_inliers", "only_unset", "install", "cam", "cam_pair") + \
        C.OUTPUTS + ("max_found",) + L.LOCALIZE_OUTPUTS[len(C.OUTPUTS):]
    good = dict(ctx=g.h, nframes_rows=nf, stride=case["stride"], max_tracks=case["max_tracks"], nimages=n,
                intrinsics=K.ctypes.data, nsel=len(frames), frames=frames.ctypes.data, images=images.ctypes.data,
                seeds=seeds.ctypes.data, max_pts=case["max_pts"], min_score=case["min_score"],
                max_ambiguity=case["max_ambiguity"], num_loops=case["num_loops"], thresh=case["thresh"],
                min_inliers=case["min_inliers"], only_unset=1, install=1, max_found=case["max_found"],
                **{k: dev[k].ptr for k in ins}, **{k: outs[k].ptr for k in outs})
    if case["offsets"] is None:
        good["offsets"] = None
    assert sorted(good) == sorted(names)

    def call(**kw):
        a = dict(good, **kw)
        return lib.misift_localize_frames_batch(*[a[k] for k in names])

    bad = [dict(ctx=None), dict(max_tracks=0), dict(max_tracks=-1), dict(nimages=0), dict(nframes_rows=0),
           dict(nframes_rows=-1), dict(max_pts=0), dict(max_pts=-1), dict(max_found=0), dict(max_found=-1),
           dict(offsets=None, stride=-1), dict(nsel=-1), dict(frames=None), dict(images=None), dict(seeds=None),
           dict(num_loops=0), dict(num_loops=-1), dict(thresh=np.nan), dict(thresh=0.0), dict(thresh=-1.0),
           dict(min_score=np.nan), dict(max_ambiguity=np.nan), dict(min_inliers=5), dict(min_inliers=0),
           dict(only_unset=2), dict(only_unset=-1), dict(install=2), dict(install=-1), dict(cam=None),
           dict(cam_pair=None), dict(cam_pair=None, install=0), dict(cam_pair=None, only_unset=0),
           dict(found_obs=good["found_obs"] + 4), dict(found_obs=good["found_obs"] + 8),
           # one launch holds 2^31 - 1 workgroups: 3 entries x 2^25 hypothesis blocks x 24 chunks do not fit
           dict(nsel=3, num_loops=2 ** 31 - 16, max_pts=12000), dict(num_loops=2 ** 31 - 15), dict(max_pts=2 ** 31 - 15)]
    bad += [{k: None} for k in ("rows", "counts", "export_summary", "points", "point_status", "intrinsics") +
            L.LOCALIZE_OUTPUTS]
    lists = []                                                   # kept alive until the calls are made
    nsel = len(frames)
    for which, hi in (("frames", nf), ("images", n)):
        base = (frames if which == "frames" else images).copy()
        for at, v in ((0, -1), (nsel - 1, hi), (1, 2 ** 31 - 1), (1, int(base[0]))):
            lists.append(base.copy())
            lists[-1][at] = v
            bad.append({which: lists[-1].ctypes.data})
    for at in (0, 1, 4 * n - 4, 4 * n - 3):
        for v in (0.0, -1500.0, np.nan, np.inf):                 # fx, fy of the first and the last image
            lists.append(K.copy())
            lists[-1].reshape(-1)[at] = v
            bad.append(dict(intrinsics=lists[-1].ctypes.data))
    for at in (2, 4 * n - 1):
        for v in (np.nan, -np.inf):                              # cx, cy
            lists.append(K.copy())
            lists[-1].reshape(-1)[at] = v
            bad.append(dict(intrinsics=lists[-1].ctypes.data))
    for kw in bad:
        assert call(**kw) == MISIFT_EINVAL, kw
    g.sync()
    for k, m in sizes.items():
        assert (g.download(outs[k], (m,), np.uint32) == POISON_WORD).all(), k
    for k in ins:
        assert g.download(dev[k], ins[k].shape, ins[k].dtype).tobytes() == ins[k].tobytes(), (k, "was written")
    # nsel == 0 writes the two summaries and d_found_offsets[0] alone; then the same arguments, unbroken
    assert call(nsel=0, frames=None, images=None, seeds=None) == MISIFT_OK
    g.sync()
    for k, m in sizes.items():
        w = g.download(outs[k], (m,), np.uint32)
        if k == "summary":
            assert w.view(np.int32).tolist() == [RC.counts(dict(case, max_obs=1))[0]] + [0] * 7
        elif k == "found_summary":
            assert (w == 0).all()
        elif k == "found_offsets":
            assert w[0] == 0 and (w[1:] == POISON_WORD).all()
        else:
            assert (w == POISON_WORD).all(), k
    assert call() == MISIFT_OK
    g.sync()
    got = {k: g.download(outs[k], (m,), np.uint32) for k, m in sizes.items()}
    got["cam"] = g.download(dev["cam"], (12 * n,), np.uint32)
    got["cam_pair"] = g.download(dev["cam_pair"], (n,), np.uint32)
    _same(got, L.expected_localize(case), L.LOCALIZE_OUTPUTS + ("cam", "cam_pair"), "unbroken")


# ---- the chain

def test_describe_match_localize_merge_triangulate_refine(g):
    """Two new images against a window of seven: describe -> misift_match_pairs_batch_i8 (two query frames against the
    scene frame) -> localise (only_unset, install) -> merge -> triangulate -> refine, nothing read in between; every
    stage is byte-equal to its restatement fed the device's own buffers."""
    from cudasift_amd import capi
    w = L.window(ncams=9, nq=2)
    d, npts, nimg, nb = w["describe"], w["npts"], w["nimages"], w["nb"]
    ins = L.describe_inputs(d)
    dev = {k: g.upload(v) for k, v in ins.items()}
    mt, mo = d["max_tracks"], d["max_obs"]
    douts = {k: _poisoned(g, n) for k, n in L.describe_sizes(d).items()}
    g.describe_points_batch(mt, mo, dev["track_offsets"], dev["obs"], dev["export_summary"], dev["points"],
                            dev["point_status"], dev["q"], d["nframes"], dev["counts"], None, d["stride"],
                            d["max_records"], **douts)
    # the query frames: a record batch of their own, quantised rows as given
    qrecs = np.concatenate(w["query"])
    d_qrecs, d_qq = g.upload(qrecs), g.upload(np.ascontiguousarray(np.concatenate(w["query_q"])))
    d_qcnt = g.upload(np.full(2, npts, np.int32))
    rows = _poisoned(g, 144 * 2 * npts)
    row_counts, matched = _poisoned(g, 2), _poisoned(g, 2)
    g.match_pairs_batch_i8([(0, 0), (1, 0)], d_qrecs, d_qq, 2, d_qcnt, None, npts, recs2=douts["scene_recs"],
                           q2=douts["scene_q"], nframes2=1, counts2=douts["scene_count"], offsets2=None, stride2=mt,
                           max_pts=npts, out=rows, out_counts=row_counts, num_matched=matched)
    K = w["K"]
    d_cam, d_pair = g.upload(np.ascontiguousarray(w["cam"], f32)), g.upload(w["cam_pair"])
    proto = L.window_localize_case(w, np.zeros(2 * npts, capi.POINT_DTYPE))
    louts = {k: _poisoned(g, n) for k, n in L.localize_sizes(proto).items()}
    g.localize_frames_batch(rows, 2, row_counts, None, npts, mt, dev["export_summary"], dev["points"],
                            dev["point_status"], nimg, K, proto["frames"], proto["images"], proto["seeds"], npts,
                            proto["max_found"], min_score=proto["min_score"], max_ambiguity=proto["max_ambiguity"],
                            num_loops=proto["num_loops"], thresh=proto["thresh"], min_inliers=proto["min_inliers"],
                            only_unset=1, install=1, cam=d_cam, cam_pair=d_pair, **louts)
    mf = proto["max_found"]
    views_b = g.upload(np.full(mt, nb, np.int32))
    a = dict(max_tracks=mf, max_obs=mf, track_offsets=louts["found_offsets"], obs=louts["found_obs"],
             export_summary=louts["found_summary"], points=louts["found_points"], point_views=louts["found_views"],
             point_status=louts["found_status"], nimages=nimg, cam=d_cam, cam_pair=d_pair, max_records=0, record_obs=None)
    b = dict(max_tracks=mt, max_obs=mo, track_offsets=dev["track_offsets"], obs=dev["obs"],
             export_summary=dev["export_summary"], points=dev["points"], point_views=views_b,
             point_status=dev["point_status"], nimages=nimg, cam=d_cam, cam_pair=d_pair, max_records=0, record_obs=None)
    mto, moo = mf + mt, mf + mo
    msizes = dict(track_offsets_out=mto + 1, obs_out=4 * moo, export_summary_out=8, points_out=4 * mto,
                  point_views_out=mto, point_status_out=mto, cam_out=12 * nimg, cam_pair_out=nimg, track_map_a=mf,
                  obs_map_a=mf, obs_map_b=mo, summary=8)
    mouts = {k: _poisoned(g, n) for k, n in msizes.items()}
    g.merge_scenes_batch(a, b, louts["found_map"], nimg, mto, moo, **mouts)
    tri = g.triangulate_tracks_batch(mto, moo, mouts["track_offsets_out"], mouts["obs_out"], mouts["export_summary_out"],
                                     nimg, mouts["cam_out"], mouts["cam_pair_out"], K, min_views=2, num_loops=5)
    ref_sizes = dict(cam_out=12 * nimg, cam_obs=nimg, cam_rms=2 * nimg, cam_steps=nimg, cam_status=nimg, summary=8)
    routs = {k: _poisoned(g, n) for k, n in ref_sizes.items()}
    g.refine_cameras_batch(mto, moo, mouts["track_offsets_out"], mouts["obs_out"], mouts["export_summary_out"], tri[0],
                           tri[2], nimg, mouts["cam_out"], mouts["cam_pair_out"], K, min_obs=6, num_loops=5,
                           max_error=4.0, orthonormalise=1, **routs)
    g.sync()

    # describe
    got_d = {k: g.download(douts[k], (n,), np.uint32) for k, n in L.describe_sizes(d).items()}
    _same(got_d, L.expected_describe(d), L.DESCRIBE_OUTPUTS, "chain, describe")
    # the match, against the numpy int8 matcher fed the device's scene
    recs2, q2 = L.scene_records(d, got_d)
    got_rows = g.download(rows, (2 * npts,), capi.POINT_DTYPE)
    assert g.download(row_counts, (2,), np.int32).tolist() == [npts, npts]
    for i in range(2):
        BU.fields_equal(got_rows[i * npts:(i + 1) * npts], BU.match_np(w["query"][i], w["query_q"][i], recs2, q2),
                        "chain, match %d" % i)
        assert (got_rows["match"][i * npts:(i + 1) * npts] == w["perm"][nb + i]).all()
    # localise, fed the device's rows
    lcase = L.window_localize_case(w, got_rows)
    got_l = {k: g.download(louts[k], (n,), np.uint32) for k, n in L.localize_sizes(lcase).items()}
    got_l["cam"], got_l["cam_pair"] = g.download(d_cam, (12 * nimg,), np.uint32), g.download(d_pair, (nimg,), np.uint32)
    el = L.expected_localize(lcase)
    _same(got_l, el, L.LOCALIZE_OUTPUTS + ("cam", "cam_pair"), "chain, localise")
    assert [x["status"] for x in el["entries"]] == [C.OK, C.OK]
    assert got_l["cam_pair"].view(np.int32).tolist()[nb:] == [C.RESECTED] * 2
    for i in range(2):
        eR, eC = C.pose_error(got_l["res_cam"].view(f32)[12 * i:12 * i + 12], w["true"][nb + i])
        print("chain: image %d, %d finds, rotation %.2e rad, centre %.2e" % (nb + i, el["entries"][i]["inliers"], eR, eC))
        assert eR < 4 * 6.4e-3 and eC < 4 * 5.6e-2               # test_localize_cpu.py: PLANTED_ROTATION, PLANTED_CENTRE
    # the merge, fed the device's finds
    mc = L.window_merge_case(w, lcase, got_l)
    em = MC.expected_merge(mc)
    got_m = {k: g.download(mouts[k], (n,), np.uint32) for k, n in msizes.items()}
    MC.compare(got_m, em, "chain, merge", keys=list(msizes))
    assert int(em["export_summary_out"].view(np.int32)[3]) == nb * npts + el["N"]
    # triangulate and refine on the merged scene
    ms = MC.merged_scene(mc, got_m)
    tcase = dict(ms, intrinsics=K, min_views=2, num_loops=5, memo={})
    with np.errstate(all="ignore"):
        et = TC.expected_triangulate(tcase)
    got_t = dict(points=g.download(tri[0], (4 * mto,), np.uint32), point_views=g.download(tri[1], (mto,), np.uint32),
                 point_status=g.download(tri[2], (mto,), np.uint32), obs_error=g.download(tri[3], (moo,), np.uint32),
                 summary=g.download(tri[4], (8,), np.uint32))
    for k in got_t:
        written = et[k] != POISON_WORD
        assert (got_t[k][written] == et[k][written]).all(), k
    T = int(ms["export_summary"][2])
    assert got_t["point_views"].view(np.int32)[:T].max() == nimg
    rcase = dict(ms, intrinsics=K, points=got_t["points"].view(f32).reshape(-1, 4),
                 point_status=got_t["point_status"].view(np.int32), hold=(), min_obs=6, num_loops=5, max_error=4.0,
                 orthonormalise=1)
    er = RC.expected_refine(rcase)
    for k in RC.OUTPUTS:
        assert g.download(routs[k], (len(er[k]),), np.uint32).tobytes() == er[k].tobytes(), k
    assert er["cam_status"].view(np.int32).tolist()[nb:] == [RC.OK] * 2


def test_guards_intact_at_the_end(g):
    from cudasift_amd import capi
    assert capi.check_guards() >= 1
    assert capi.lib().misift_test_check_guards(None) == 0

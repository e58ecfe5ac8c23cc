"""misift_link_poses_batch without a GPU: posegraph_cases.expected_link_poses, the numpy float32 restatement of the
definition in include/misift.h, which tests/test_gpu_posegraph.py holds the device to byte for byte.  Here the restatement
is pinned from both sides: the library's host-only hooks misift_test_posegraph_ratio and misift_test_posegraph_compose,
compiled from the functions the kernels run, must equal it byte for byte on every case of the GPU file, and on planted
scenes its answer is held to the same call in float64 on the same rows, and through that to the planted cameras.  The
premises of the cases are asserted here too: a link built to have c samples has c under the restatement alone."""
import numpy as np
import pytest

import posegraph_cases as G
from test_fundamental_cpu import f32
from test_pose_cpu import EPS, ORTHO_BOUND, rotation_error

STAGE = 4096                                                     # asserted against the library's hook below


def same_as_hooks(case, what):
    """Both hooks equal the restatement byte for byte on every link and on the graph; returns the expected outputs."""
    with np.errstate(all="ignore"):
        e = G.expected_link_poses(case)
    done = set()
    for l, (p, q, kind) in enumerate(np.asarray(case["links"]).reshape(-1, 3).tolist()):
        if (p, q, kind) in done:
            continue
        done.add((p, q, kind))
        ratio, common = G.hook_ratio(*G.pair_block(case, p), *G.pair_block(case, q), case["max_pts"], kind,
                                     case["max_error"], case["min_common"])
        assert common == e["link_common"][l], (what, "link", l, common, e["link_common"][l])
        assert f32(ratio).tobytes() == e["link_ratio"][l].tobytes(), (what, "link", l, ratio, e["link_ratio"][l])
    scale, cam, cam_pair, counts = G.hook_compose(case["pairs"], case["nimages"], case["pose"], case["num_front"],
                                                  case["links"], e["link_ratio"], case["seed_pair"],
                                                  case["root_image"], case["walk"])
    assert scale.tobytes() == e["pair_scale"].tobytes(), (what, scale, e["pair_scale"])
    assert cam_pair.tolist() == e["cam_pair"].tolist() and counts == e["summary"][1:3].tolist(), (what, cam_pair, counts)
    assert cam.tobytes() == e["cam"].tobytes(), (what, cam, e["cam"])
    return e


def premises(case, e, what):
    """Every link built to have a given sample count has it."""
    for l, want in enumerate(case.get("want", [])):
        assert want is None or e["link_common"][l] == want, (what, "link", l, e["link_common"][l], want)


def test_library_exports_the_call():
    """Fails without the feature: the symbols, their rows in capi.SIGNATURES, the binding, the argument checks that need
    no device."""
    from cudasift_amd import capi
    L = capi.lib()
    for name in ("misift_link_poses_batch", "misift_test_posegraph_ratio", "misift_test_posegraph_compose",
                 "misift_test_posegraph_capacity"):
        assert name in capi.SIGNATURES and hasattr(L, name), name
    assert hasattr(capi.Context, "link_poses_batch")
    none = [None] * 6
    assert L.misift_link_poses_batch(None, 0, None, 1, None, None, 8, 0.85, 0.95, 1.0, None, None, None, 0, None, 0, 0,
                                     8, 0, None, *none) == -1    # MISIFT_EINVAL
    assert L.misift_test_posegraph_ratio(None, None, 0, None, None, 0, 8, 0, 0.85, 0.95, 1.0, 8, None, None) == -1
    assert L.misift_test_posegraph_compose(0, None, 1, None, None, 0, None, None, 0, 0, 0, None, None, None, None,
                                           None) == -1
    assert G.capacity(0) == STAGE and G.capacity(1) >= 1024


@pytest.mark.parametrize("name", ["count", "row_count", "tie"])
def test_planted_links_equal_the_hooks(name):
    case = getattr(G, name + "_case")()
    e = same_as_hooks(case, name)
    premises(case, e, name)
    if name == "count":                                          # both parities of the lower median, by hand
        for l, c in enumerate(e["link_common"]):
            p, q, kind = case["links"][l]
            _, rho = G.samples(*G.pair_block(case, p), *G.pair_block(case, q), case["max_pts"], kind, case["max_error"])
            want = np.sort(rho)[(c - 1) // 2] if c >= G.MIN_COMMON else 0
            assert e["link_ratio"][l] == want and (c < G.MIN_COMMON or (rho <= want).sum() >= (c + 1) // 2)
        assert case["max_pts"] % 16 != 0
    if name == "tie":
        for l in (0, 4):
            assert e["link_ratio"][l] == 2.0
        for l in (1, 2, 5, 6):                                   # 20 + 20: the lower value; 21 of 4.0 and 20 of 0.5: 4.0
            assert e["link_ratio"][l] == (0.5 if l in (1, 5) else 4.0), (l, e["link_ratio"][l])


def test_the_staging_capacity_equals_the_hooks():
    case = G.capacity_case(G.capacity(0))
    e = same_as_hooks(case, "capacity")
    premises(case, e, "capacity")
    assert sorted(set(e["link_common"].tolist())) == [STAGE - 1, STAGE, STAGE + 1]


@pytest.mark.parametrize("max_error", [2.0, G.INF], ids=["finite max_error", "max_error inf"])
def test_hostile_rows_equal_the_hooks(max_error):
    case = G.hostile_case(max_error)
    e = same_as_hooks(case, "hostile")
    for l, (p, q, kind) in enumerate(case["links"]):
        rows, rho = G.samples(*G.pair_block(case, p), *G.pair_block(case, q), case["max_pts"], kind, case["max_error"])
        assert 42 in rows and rho[list(rows).index(42)] < 1.2e-38          # a subnormal ratio is a sample
        assert not {40, 41} & set(rows.tolist())                 # overflow and underflow to 0 are not
        hit = set(range(50, 58)) & set(rows.tolist())            # the hostile match fields: CHAIN has no partner for any;
        assert hit == (set() if kind == G.CHAIN else {52, 53, 54, 55, 56})     # FAN rejects the negative ones only
        assert not set(range(60, 68)) & set(rows.tolist())       # each term of the edge rule, alone
        assert np.isfinite(rho).all() and (rho > 0).all() and e["link_common"][l] == len(rows) >= 60
        nan = np.isnan(G.pair_block(case, p)[0]["match_error"][rows])
        assert nan.any() == (not np.isfinite(max_error))         # a NaN match_error is a sample only when not read


@pytest.mark.parametrize("name", [c[0] for c in G.graph_cases(1)])
def test_graphs_equal_the_hooks(name):
    case, facts = next((c[1], c[2]) for c in G.graph_cases(G.capacity(1)) if c[0] == name)
    e = same_as_hooks(case, name)
    premises(case, e, name)
    assert e["summary"][1] == facts["scaled"] and e["summary"][2] == facts["cams"], (name, e["summary"])
    assert (e["cam_pair"] == G.UNSET).sum() == case["nimages"] - facts["cams"]
    for i in facts.get("unset", []):
        assert e["cam_pair"][i] == G.UNSET and not e["cam"][i].any()
    for i, p in facts.get("placed_by", {}).items():
        assert e["cam_pair"][i] == p
    assert e["cam_pair"][case["root_image"]] == G.ROOT
    assert e["cam"][case["root_image"]].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    if name == "more links than step 2 stages":
        assert 3 * len(case["links"]) > G.capacity(1)
    if name == "backward":                                       # every scale through scale[p] = scale[q] * rho
        assert (e["pair_scale"] > 0).all() and e["pair_scale"][4] == 1 and (e["cam_pair"][:5] == np.arange(5)).all()


# ---- float64 and the planted cameras
#
# The noisy scene: what limits the answer is the 0.5 px noise in the rows, not fp32.  The same call in float64 on the same
# rows, samples and poses (link_poses64) has the same noise in it, so the bound on the fp32 answer's error against the
# planted scene is twice the float64 answer's: a margin for fp32 against float64, not a tuned number.  Measured (seed 31,
# 8 cameras, baselines 0.12 .. 0.6, 400 points, a quarter of the matches wrong): ratios within 6.81e-2 of |T_p| / |T_q|
# (the worst link joins the shortest baseline, 22 px of parallax), rotations within 2.67e-3, camera positions within
# 6.81e-2 seed baselines (3.05e-2 of their distance from the root); fp32 and float64 differ by 5.1e-8 in a ratio and 3.5e-7
# in a camera entry.
SCENE_RATIO_MEASURED = 6.81e-2
SCENE_R_MEASURED = 2.67e-3
SCENE_T_MEASURED = 6.81e-2


def camera_errors(cam, truth):
    cam = np.asarray(cam, np.float64)
    rot = max(rotation_error(c[:9], t[:9].reshape(3, 3)) for c, t in zip(cam, truth))
    return rot, float(np.linalg.norm(cam[:, 9:] - truth[:, 9:], axis=1).max())


def scene_errors(sc, e):
    """(ratio, rotation, translation) errors of the fp32 answer e and of float64 on the same rows, against the scene."""
    case = sc["case"]
    r64, _, c64 = G.link_poses64(case)
    truth = np.array([G.planted_ratio(sc["cams"], sc["pairs"], l) for l in sc["links"]])
    gt = G.planted_cameras(sc["cams"], case["root_image"], sc["pairs"][case["seed_pair"]])
    got = (float(np.abs(e["link_ratio"].astype(np.float64) / truth - 1).max()),) + camera_errors(e["cam"], gt)
    ref = (float(np.abs(r64 / truth - 1).max()),) + camera_errors(c64, gt)
    return got, ref


def test_planted_scene_against_float64():
    sc = G.planted_scene()
    case = sc["case"]
    e = same_as_hooks(case, "planted scene")
    assert (e["link_common"] >= case["min_common"]).all() and e["summary"].tolist()[:3] == [12, 13, 8]
    steps = [np.linalg.norm(sc["cams"][i][0].T @ sc["cams"][i][1] - sc["cams"][i + 1][0].T @ sc["cams"][i + 1][1])
             for i in range(7)]
    assert max(steps) / min(steps) >= 4.99                       # baselines a factor of 5 apart
    got, ref = scene_errors(sc, e)
    print("planted scene: fp32 %s float64 %s" % (got, ref))
    for g, r in zip(got, ref):
        assert g <= 2 * r, (got, ref)
    for g, m in zip(got, (SCENE_RATIO_MEASURED, SCENE_R_MEASURED, SCENE_T_MEASURED)):
        assert g <= 2 * m, (got, m)                              # what DESIGN.md records


# The exact chain: 64 images, 63 pairs with their exact F and exact rows.  RtR - I of a product M = fl(R Ra) moves by at
# most 2 |E|_F + the defect of R, with |E_ij| <= 3 EPS (three rounded products and two rounded sums of terms whose
# absolute sum is at most 1 by Cauchy-Schwarz), so |E|_F <= 9 EPS; the pose's own defect is within ORTHO_BOUND
# (test_pose_cpu.py).  Per step that is 18 EPS + ORTHO_BOUND, and 63 steps at the most.  Measured: 1.02e-5 at image 59;
# the rotations lie within 5.2e-6 and the positions within 1.8e-4 seed baselines of the planted ones (the path spans 15.6).
DRIFT_BOUND = 63 * (18 * EPS + ORTHO_BOUND)
DRIFT_MEASURED = 1.02e-5


def test_exact_chain_drift():
    x = G.exact_chain()
    case = x["case"]
    e = same_as_hooks(case, "exact chain")
    assert e["summary"].tolist()[:4] == [62, 63, 64, 64]
    R = e["cam"][:, :9].reshape(-1, 3, 3).astype(np.float64)
    drift = max(float(np.linalg.norm(r.T @ r - np.eye(3))) for r in R)
    gt = G.planted_cameras(x["cams"], 0, x["pairs"][0])
    rot, pos = camera_errors(e["cam"], gt)
    truth = np.array([G.planted_ratio(x["cams"], x["pairs"], l) for l in x["links"]])
    ratio = float(np.abs(e["link_ratio"] / truth - 1).max())
    print("exact chain: drift %.3g rotation %.3g position %.3g ratio %.3g" % (drift, rot, pos, ratio))
    assert drift <= DRIFT_BOUND and drift <= 2 * DRIFT_MEASURED
    r64, _, c64 = G.link_poses64(case)
    rot64, pos64 = camera_errors(c64, gt)
    assert rot <= 2 * max(rot64, 63 * 9 * EPS) and pos <= 2 * max(pos64, 63 * 9 * EPS * np.abs(gt[:, 9:]).max())


def test_hook_arguments():
    case = G.graph_cases()[0][1]
    from cudasift_amd import capi
    L = capi.lib()
    rows, xyz, n = G.pair_block(case, 0)
    out, c = np.zeros(1, f32), np.zeros(1, np.int32)
    a = [rows.ctypes.data, xyz.ctypes.data, n, rows.ctypes.data, xyz.ctypes.data, n, case["max_pts"], 0, 0.85, 0.95, 2.0,
         8, out.ctypes.data, c.ctypes.data]
    assert L.misift_test_posegraph_ratio(*a) == 0
    for i, v in ((0, None), (1, None), (3, None), (4, None), (6, 0), (7, 2), (7, -1), (11, 0), (12, None), (13, None)):
        b = list(a)
        b[i] = v
        assert L.misift_test_posegraph_ratio(*b) == -1, (i, v)

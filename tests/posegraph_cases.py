"""misift_link_poses_batch: expected_link_poses, the numpy float32 restatement of the definition in include/misift.h, the
wrappers of the library's host hooks, and the cases of its tests (test_posegraph_cpu.py pins the restatement to the hooks
and to float64, test_gpu_posegraph.py holds the device to it byte for byte).  A case is a dict of the call's arguments,
CASE_KEYS.  No GPU in here, and cudasift_amd.capi is imported inside functions only."""
import numpy as np

import pose_cases as PC
from test_fundamental_cpu import GATES, f32

CHAIN, FAN = 0, 1
UNSET, ROOT = -2, -1
INT_MAX = 2 ** 31 - 1
INF = float("inf")
MIN_COMMON = 8
CASE_KEYS = ("pairs", "nimages", "rows", "row_counts", "max_pts", "max_error", "pose", "num_front", "xyz", "links",
             "seed_pair", "root_image", "min_common", "walk")


# ---- step 1 restated: one array over the rows of pair p

def taking_part(count, max_pts):
    return min(max(int(count), 0), int(max_pts))


def accept(rows, min_score, max_ambiguity, max_error):
    with np.errstate(invalid="ignore"):
        ok = (rows["match"] >= 0) & (rows["score"] > f32(min_score)) & (rows["ambiguity"] < f32(max_ambiguity))
        if f32(max_error) < f32(np.inf):
            ok = ok & (rows["match_error"] < f32(max_error))
    return ok


def samples(rows_p, xyz_p, count_p, rows_q, xyz_q, count_q, max_pts, kind, max_error, gates=GATES):
    """(the rows of pair p that are samples, their rho as float32), in row order."""
    n_p, n_q = taking_part(count_p, max_pts), taking_part(count_q, max_pts)
    if n_p == 0 or n_q == 0:
        return np.zeros(0, np.int64), np.zeros(0, f32)
    a, za = rows_p[:n_p], np.asarray(xyz_p, f32).reshape(-1, 4)[:n_p]
    r = np.arange(n_p, dtype=np.int64)
    r2 = a["match"].astype(np.int64) if kind == CHAIN else r
    ok = (r2 >= 0) & (r2 < n_q)
    rc = np.where(ok, r2, 0)
    b, zb = rows_q[rc], np.asarray(xyz_q, f32).reshape(-1, 4)[rc]
    with np.errstate(all="ignore"):
        ok &= accept(a, *gates, max_error) & accept(b, *gates, max_error)
        ok &= (za[:, 2] > 0) & (za[:, 3] > 0) & (zb[:, 2] > 0) & (zb[:, 3] > 0)
        rho = (zb[:, 2] / (za[:, 3] if kind == CHAIN else za[:, 2])).astype(f32)
        ok &= np.isfinite(rho) & (rho > 0)
    return r[ok], rho[ok]


def link_ratio(rows_p, xyz_p, count_p, rows_q, xyz_q, count_q, max_pts, kind, max_error, min_common, gates=GATES):
    """(d_link_ratio, d_link_common) of one link: the lower median by bit pattern."""
    _, rho = samples(rows_p, xyz_p, count_p, rows_q, xyz_q, count_q, max_pts, kind, max_error, gates)
    c = len(rho)
    if c < min_common:
        return f32(0), c
    return np.sort(rho.view(np.uint32))[(c - 1) >> 1].view(f32), c


# ---- steps 2 and 3 restated: float32 scalars

def _one_nan(v):
    return PC.ONE_NAN if np.isnan(v) else f32(v)


def _sum3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def forward(P, s, ca):
    """Camera b from camera a through X_b = R X_a + s t."""
    R, t, Ra, ta = P[:9].reshape(3, 3), P[9:], ca[:9].reshape(3, 3), ca[9:]
    out = np.zeros(12, f32)
    for r in range(3):
        for c in range(3):
            out[3 * r + c] = _one_nan(_sum3(R[r, 0], Ra[0, c], R[r, 1], Ra[1, c], R[r, 2], Ra[2, c]))
        out[9 + r] = _one_nan(_sum3(R[r, 0], ta[0], R[r, 1], ta[1], R[r, 2], ta[2]) + s * t[r])
    return out


def backward(P, s, cb):
    """Camera a from camera b."""
    R, t, Rb, tb = P[:9].reshape(3, 3), P[9:], cb[:9].reshape(3, 3), cb[9:]
    d = [tb[j] - s * t[j] for j in range(3)]
    out = np.zeros(12, f32)
    for r in range(3):
        for c in range(3):
            out[3 * r + c] = _one_nan(_sum3(R[0, r], Rb[0, c], R[1, r], Rb[1, c], R[2, r], Rb[2, c]))
        out[9 + r] = _one_nan(_sum3(R[0, r], d[0], R[1, r], d[1], R[2, r], d[2]))
    return out


def usable_pairs(pose, num_front):
    pose = np.asarray(pose, f32).reshape(-1, 12)
    return (np.asarray(num_front).reshape(-1) > 0) & np.isfinite(pose).all(1)


def compose(pairs, nimages, pose, num_front, links, ratio, seed_pair, root_image, walk):
    """(d_pair_scale, d_cam (nimages, 12), d_cam_pair, [pairs with a scale, images with a camera])."""
    pairs, links = np.asarray(pairs, np.int64).reshape(-1, 2), np.asarray(links, np.int64).reshape(-1, 3)
    pose = np.asarray(pose, f32).reshape(-1, 12)
    usable = usable_pairs(pose, num_front)
    scale = np.zeros(len(pairs), f32)
    cam, cam_pair = np.zeros((nimages, 12), f32), np.full(nimages, UNSET, np.int32)
    if len(pairs) and usable[seed_pair]:
        scale[seed_pair] = 1
    with np.errstate(all="ignore"):
        for (p, q, _), rho in zip(links, np.asarray(ratio, f32).reshape(-1)):
            if not rho > 0 or not usable[p] or not usable[q]:
                continue
            if scale[p] > 0 and scale[q] == 0:
                v = scale[p] / rho
                if v > 0 and np.isfinite(v):
                    scale[q] = v
            elif scale[q] > 0 and scale[p] == 0:
                v = scale[q] * rho
                if v > 0 and np.isfinite(v):
                    scale[p] = v
        cam[root_image, [0, 4, 8]] = 1
        cam_pair[root_image] = ROOT
        for p in np.asarray(walk, np.int64).reshape(-1):
            a, b = pairs[p]
            s = scale[p]
            if not s > 0 or a == b:
                continue
            sa, sb = cam_pair[a] != UNSET, cam_pair[b] != UNSET
            if sa == sb:
                continue
            if sa:
                cam[b], cam_pair[b] = forward(pose[p], s, cam[a]), p
            else:
                cam[a], cam_pair[a] = backward(pose[p], s, cam[b]), p
    return scale, cam, cam_pair, [int((scale > 0).sum()), int((cam_pair != UNSET).sum())]


def pair_block(case, p):
    """(rows, xyz, row count) of pair p of a case."""
    m = case["max_pts"]
    return (case["rows"][p * m:(p + 1) * m], case["xyz"].reshape(-1, 4)[p * m:(p + 1) * m], int(case["row_counts"][p]))


def expected_link_poses(case, gates=GATES):
    """The six outputs of the call on a case, as a dict of arrays."""
    links = np.asarray(case["links"], np.int64).reshape(-1, 3)
    ratio, common = np.zeros(len(links), f32), np.zeros(len(links), np.int32)
    seen = {}                                                    # a link listed again has the same answer
    for l, key in enumerate(map(tuple, links)):
        if key not in seen:
            p, q, kind = key
            seen[key] = link_ratio(*pair_block(case, p), *pair_block(case, q), case["max_pts"], kind,
                                   case["max_error"], case["min_common"], gates)
        ratio[l], common[l] = seen[key]
    scale, cam, cam_pair, counts = compose(case["pairs"], case["nimages"], case["pose"], case["num_front"], links, ratio,
                                           case["seed_pair"], case["root_image"], case["walk"])
    enough = common >= case["min_common"]
    summary = np.array([enough.sum(), counts[0], counts[1], common[enough].min() if enough.any() else 0, 0, 0, 0, 0],
                       np.int32)
    return dict(link_ratio=ratio, link_common=common, pair_scale=scale, cam=cam, cam_pair=cam_pair, summary=summary)


# ---- the hooks

def hook_ratio(rows_p, xyz_p, count_p, rows_q, xyz_q, count_q, max_pts, kind, max_error, min_common, gates=GATES):
    from cudasift_amd import capi
    rows_p, rows_q = np.ascontiguousarray(rows_p), np.ascontiguousarray(rows_q)
    xyz_p, xyz_q = np.ascontiguousarray(xyz_p, f32), np.ascontiguousarray(xyz_q, f32)
    ratio, common = np.full(1, 3.5, f32), np.full(1, -77, np.int32)
    assert capi.lib().misift_test_posegraph_ratio(rows_p.ctypes.data, xyz_p.ctypes.data, count_p, rows_q.ctypes.data,
                                                  xyz_q.ctypes.data, count_q, max_pts, kind, gates[0], gates[1],
                                                  max_error, min_common, ratio.ctypes.data, common.ctypes.data) == 0
    return ratio[0], int(common[0])


def hook_compose(pairs, nimages, pose, num_front, links, ratio, seed_pair, root_image, walk):
    from cudasift_amd import capi
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    links = np.ascontiguousarray(links, np.int32).reshape(-1, 3)
    walk = np.ascontiguousarray(walk, np.int32).reshape(-1)
    pose, front = np.ascontiguousarray(pose, f32).reshape(-1, 12), np.ascontiguousarray(num_front, np.int32)
    ratio = np.ascontiguousarray(ratio, f32)
    scale, cam = np.full(max(len(pairs), 1), 3.5, f32), np.full((nimages, 12), 3.5, f32)
    cam_pair, counts = np.full(nimages, -77, np.int32), np.full(2, -77, np.int32)
    assert capi.lib().misift_test_posegraph_compose(len(pairs), pairs.ctypes.data, nimages, pose.ctypes.data,
                                                    front.ctypes.data, len(links), links.ctypes.data, ratio.ctypes.data,
                                                    seed_pair, root_image, len(walk), walk.ctypes.data,
                                                    scale.ctypes.data, cam.ctypes.data, cam_pair.ctypes.data,
                                                    counts.ctypes.data) == 0
    return scale[:len(pairs)], cam, cam_pair, counts.tolist()


def capacity(which):
    """0: the rows of a link the ratio kernel stages on chip; 1: the words of lists and state step 2 stages on chip."""
    from cudasift_amd import capi
    return int(capi.lib().misift_test_posegraph_capacity(which))


# ---- planted rows: no images, no geometry; what the call reads is written directly

def rotation(rng, angle=0.2):
    return PC.rodrigues(rng.normal(0, 1, 3), angle)


def random_pose(rng):
    t = rng.normal(0, 1, 3)
    return np.concatenate([rotation(rng).reshape(9), t / np.linalg.norm(t)]).astype(f32)


def good_rows(n, rng, nq=None, permute=True):
    """n accepted rows with random other bytes; match = a permutation of the partner's nq rows (or r itself)."""
    from cudasift_amd import capi
    rows = np.frombuffer(rng.bytes(576 * n), capi.POINT_DTYPE).copy()
    rows["score"], rows["ambiguity"], rows["match_error"] = 0.97, 0.3, 0.5
    nq = n if nq is None else nq
    m = rng.permutation(max(nq, n))[:n] if permute else np.arange(n)
    rows["match"] = np.where(m < nq, m, 0) if nq else 0
    return rows


def good_xyz(n, rng, unit=1.0, spread=0.2):
    """Depths z1, z2 in [3, 9] / unit with a relative jitter, and the point they belong to."""
    z1 = rng.uniform(3, 9, n) / unit
    z2 = z1 * (1 + rng.normal(0, spread, n) * 0.1) + 0.05
    return np.stack([z1 * rng.normal(0, 0.3, n), z1 * rng.normal(0, 0.3, n), z1, z2], 1).astype(f32)


BREAKS = ("score p", "ambiguity p", "match p", "error p", "score q", "ambiguity q", "match q", "error q", "z1 p", "z2 p",
          "z1 q", "z2 q")


def break_row(rows_p, xyz_p, rows_q, xyz_q, kind, r, how, max_error):
    """Make row r of pair p no sample, in one way; match q: the partner row's own match field is negative."""
    r2 = int(rows_p["match"][r]) if kind == CHAIN else r
    side, z = (rows_p, xyz_p) if how.endswith("p") else (rows_q, xyz_q)
    i = r if how.endswith("p") else r2
    what = how.split()[0]
    if what == "score":
        side["score"][i] = GATES[0]
    elif what == "ambiguity":
        side["ambiguity"][i] = GATES[1]
    elif what == "match":
        side["match"][i] = -1 - (r % 3)
    elif what == "error":
        side["match_error"][i] = max_error if np.isfinite(max_error) else 0.5
        if not np.isfinite(max_error):
            side["score"][i] = np.nan
    elif what == "z1":
        z[i, 2] = (0.0, -1.0, np.nan)[r % 3]
    else:
        z[i, 3] = (-0.0, -np.inf, np.nan)[r % 3]


class Builder:
    """Collects pairs, their rows and the links of one call."""

    def __init__(self, max_pts, seed, max_error=2.0, min_common=MIN_COMMON):
        self.rng = np.random.default_rng(seed)
        self.max_pts, self.max_error, self.min_common = max_pts, max_error, min_common
        self.pairs, self.rows, self.xyz, self.counts, self.links, self.want = [], [], [], [], [], []
        self.pose, self.front, self.nimages = [], [], 0

    def pair(self, a, b, rows, xyz, count=None, front=10, pose=None):
        """Adds pair (a, b); the rows are padded to max_pts with accepted rows that must not be read."""
        from cudasift_amd import capi
        assert len(rows) <= self.max_pts
        pad = self.max_pts - len(rows)
        extra = good_rows(pad, self.rng, permute=False)
        self.rows.append(np.concatenate([rows, extra]).astype(capi.POINT_DTYPE))
        self.xyz.append(np.concatenate([xyz, good_xyz(pad, self.rng)]).astype(f32))
        self.pairs.append((a, b))
        self.counts.append(len(rows) if count is None else count)
        self.pose.append(random_pose(self.rng) if pose is None else np.asarray(pose, f32))
        self.front.append(front)
        self.nimages = max(self.nimages, a + 1, b + 1)
        return len(self.pairs) - 1

    def image(self):
        self.nimages += 1
        return self.nimages - 1

    def link(self, p, q, kind, want=None):
        """want: the sample count the link is built to have (a premise the CPU file asserts), or None."""
        self.links.append((p, q, kind))
        self.want.append(want)

    def two_pairs(self, kind, n, nq=None, unit_q=2.0):
        """Two fresh pairs that form one link of the kind over three fresh images, all n rows samples."""
        nq = n if nq is None else nq
        i, j, k = self.image(), self.image(), self.image()
        rp, rq = good_rows(n, self.rng, nq, permute=kind == CHAIN), good_rows(nq, self.rng)
        zp, zq = good_xyz(n, self.rng), good_xyz(nq, self.rng, unit_q)
        return (i, j, k), rp, zp, rq, zq

    def planted_link(self, kind, c, nbad, want=True):
        """One link with exactly c samples among c + nbad rows; the bad rows are broken in rotating ways."""
        n = c + nbad
        (i, j, k), rp, zp, rq, zq = self.two_pairs(kind, n)
        bad = self.rng.permutation(n)[:nbad]
        for t, r in enumerate(bad):
            break_row(rp, zp, rq, zq, kind, int(r), BREAKS[(t + c) % len(BREAKS)], self.max_error)
        p = self.pair(i, j, rp, zp)
        q = self.pair(j, k, rq, zq) if kind == CHAIN else self.pair(i, k, rq, zq)
        self.link(p, q, kind, c if want else None)
        return p, q

    def case(self, seed_pair=0, root_image=0, walk=None):
        return dict(pairs=np.array(self.pairs, np.int32).reshape(-1, 2), nimages=max(self.nimages, 1),
                    rows=np.concatenate(self.rows), row_counts=np.array(self.counts, np.int32), max_pts=self.max_pts,
                    max_error=self.max_error, pose=np.array(self.pose, f32).reshape(-1, 12),
                    num_front=np.array(self.front, np.int32), xyz=np.concatenate(self.xyz).astype(f32),
                    links=np.array(self.links, np.int32).reshape(-1, 3), seed_pair=seed_pair, root_image=root_image,
                    min_common=self.min_common, walk=np.arange(len(self.pairs)) if walk is None else np.array(walk),
                    want=list(self.want))


SMALL_COUNTS = (0, 1, 2, 3, MIN_COMMON - 1, MIN_COMMON, 255, 256, 257)


def count_case():
    """Every small sample count, in CHAIN and in FAN, max_pts off the multiple of 16; counts below 255 sit among three
    broken rows, the others fill their pair, so the rows are 255, 256 and 257 as well."""
    b = Builder(261, 1)
    for kind in (CHAIN, FAN):
        for c in SMALL_COUNTS:
            b.planted_link(kind, c, 3 if c < 255 else 0)
    return b.case()


def capacity_case(cap):
    """cap - 1, cap and cap + 1 samples in as many rows: below, at and beyond what the ratio kernel stages."""
    b = Builder(cap + 3, 2)
    for kind in (CHAIN, FAN):
        for c in (cap - 1, cap, cap + 1):
            b.planted_link(kind, c, 0)
    return b.case()


def row_count_case():
    """d_row_counts of -1, 0 and above max_pts, on either side of a link; a partner shorter than the matches reach."""
    b = Builder(37, 3)
    for kind in (CHAIN, FAN):
        for cp, cq, want in ((-1, None, 0), (0, None, 0), (None, -1, 0), (None, 0, 0), (1000, None, 37), (None, 1000, 37),
                             (INT_MAX, INT_MAX, 37), (20, None, 20), (None, 20, None)):
            (i, j, k), rp, zp, rq, zq = b.two_pairs(kind, 37)
            p = b.pair(i, j, rp, zp, count=cp)
            q = b.pair(j, k, rq, zq, count=cq) if kind == CHAIN else b.pair(i, k, rq, zq, count=cq)
            b.link(p, q, kind, want)
    return b.case()


def tie_case():
    """All ratios equal; two values each on half of the samples, with an even and an odd count; two neighbouring floats.
    The factors are powers of two, so the products and the ratios are exact."""
    b = Builder(45, 4)
    for kind in (CHAIN, FAN):
        for n, values in ((40, (2.0,)), (40, (0.5, 4.0)), (41, (4.0, 0.5)), (9, (2.0, 2.0000002))):
            (i, j, k), rp, zp, rq, zq = b.two_pairs(kind, n)
            r2 = rp["match"] if kind == CHAIN else np.arange(n)
            zq[r2, 2] = (zp[:, 3] if kind == CHAIN else zp[:, 2]) * np.array(values, f32)[np.arange(n) % len(values)]
            p = b.pair(i, j, rp, zp)
            q = b.pair(j, k, rq, zq) if kind == CHAIN else b.pair(i, k, rq, zq)
            b.link(p, q, kind, n)
    return b.case()


HOSTILE_DEPTHS = (np.nan, np.inf, -np.inf, 0.0, -0.0, -2.5, 1e-45, 1e-39, 3e38, 1e-38)


def hostile_case(max_error=2.0):
    """Hostile depths in each of the four slots a link reads, ratios that overflow and underflow, match fields below 0,
    at and beyond the partner's rows and INT_MAX, and every term of the edge rule failing alone.  With max_error = +inf
    match_error holds NaNs and must not be read."""
    b = Builder(157, 5, max_error=max_error)
    for kind in (CHAIN, FAN):
        n = 150
        (i, j, k), rp, zp, rq, zq = b.two_pairs(kind, n, nq=140)
        r2 = np.where(rp["match"] < 140, rp["match"], 0) if kind == CHAIN else np.minimum(np.arange(n), 139)
        for t in range(40):                                      # rows 0..39: one hostile depth each
            v, slot = HOSTILE_DEPTHS[t % 10], t // 10
            (zp if slot < 2 else zq)[t if slot < 2 else r2[t], 2 + slot % 2] = v
        zp[40, 2:], zq[r2[40], 2] = 1e-38, 3e38                  # rho overflows
        zp[41, 2:], zq[r2[41], 2] = 3e38, 1e-45                  # rho underflows to 0
        zp[42, 2:], zq[r2[42], 2] = 1e3, 1e-39                   # rho is subnormal: a sample
        for t, m in enumerate((-1, -7, 140, 141, 157, 1000, INT_MAX, -INT_MAX - 1)):
            rp["match"][50 + t] = m                              # CHAIN: no partner; FAN: < 0 fails the edge rule
        for t, how in enumerate(BREAKS[:8]):
            break_row(rp, zp, rq, zq, kind, 60 + t, how, max_error)
        if not np.isfinite(max_error):
            rp["match_error"][70:90], rq["match_error"][::3] = np.nan, np.nan
        else:
            rp["match_error"][70], rq["match_error"][r2[71]] = np.nan, np.nan
        p = b.pair(i, j, rp, zp)
        q = b.pair(j, k, rq, zq) if kind == CHAIN else b.pair(i, k, rq, zq)
        b.link(p, q, kind)
    return b.case()


def _graph(pairs, links, seed, root, walk, front=None, few=(), nan_pose=(), rows=12, rng_seed=6, repeat_links=1):
    """A call over the image pairs given, every pair with `rows` rows that are all samples in every link, but for the
    pairs in `few`, which hold MIN_COMMON - 1 accepted rows.  Self links and any pair order are fine."""
    b = Builder(rows + 1, rng_seed)
    for p, (i, j) in enumerate(pairs):
        r = good_rows(rows, b.rng)
        if p in few:
            r["score"][MIN_COMMON - 1:] = GATES[0]
        pose = random_pose(b.rng)
        if p in nan_pose:
            pose[(5 * p) % 12] = (np.nan, np.inf)[p % 2]
        b.pair(i, j, r, good_xyz(rows, b.rng, unit=1 + 0.37 * p), front=10 if front is None else front[p], pose=pose)
    for _ in range(repeat_links):
        for p, q, kind in links:
            b.link(p, q, kind, MIN_COMMON - 1 if (p in few or q in few) else rows)
    return b.case(seed, root, walk)


SEQ = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
SEQ_LINKS = [(0, 1, CHAIN), (1, 2, CHAIN), (2, 3, CHAIN), (3, 4, CHAIN)]


def graph_cases(serial_words=None):
    """(name, case, what it must show: a dict of expected facts the CPU file asserts on the restatement)."""
    out = [
        ("outward", _graph(SEQ, SEQ_LINKS, 0, 0, range(5)), dict(scaled=5, cams=6)),
        ("a link met too early", _graph(SEQ, [SEQ_LINKS[1], SEQ_LINKS[0], SEQ_LINKS[2], SEQ_LINKS[3]], 0, 0, range(5)),
         dict(scaled=2, cams=3, unset=[3, 4, 5])),
        ("backward", _graph(SEQ, SEQ_LINKS[::-1], 4, 5, range(5)[::-1]), dict(scaled=5, cams=6)),
        ("a cycle", _graph([(0, 1), (1, 2), (2, 0)], [(0, 1, CHAIN), (1, 2, CHAIN), (2, 0, CHAIN)], 0, 0, range(3)),
         dict(scaled=3, cams=3)),
        ("an unusable seed", _graph(SEQ, SEQ_LINKS, 0, 0, range(5), front=[0, 9, 9, 9, 9]), dict(scaled=0, cams=1)),
        ("a negative vote at the seed", _graph(SEQ, SEQ_LINKS, 0, 0, range(5), front=[-3, 9, 9, 9, 9]),
         dict(scaled=0, cams=1)),
        ("no vote in the middle", _graph(SEQ, SEQ_LINKS, 0, 0, range(5), front=[9, 9, 0, 9, 9]),
         dict(scaled=2, cams=3, unset=[3, 4, 5])),
        ("a non-finite pose in the middle", _graph(SEQ, SEQ_LINKS, 0, 0, range(5), nan_pose=(2, 3)),
         dict(scaled=2, cams=3, unset=[3, 4, 5])),
        ("too few in the middle", _graph(SEQ, SEQ_LINKS, 0, 0, range(5), few=(2,)), dict(scaled=2, cams=3)),
        ("reachable two ways", _graph([(0, 1), (0, 2), (1, 2)], [(0, 1, FAN), (0, 2, CHAIN)], 0, 0, [0, 2, 1]),
         dict(scaled=3, cams=3, placed_by={2: 2})),
        ("forward then backward from the middle", _graph(SEQ, [(1, 2, CHAIN), (0, 1, CHAIN), (2, 3, CHAIN)], 1, 2,
                                                         [2, 1, 0, 3, 4]), dict(scaled=4, cams=5, unset=[5])),
        ("a self pair and a pair listed twice", _graph([(0, 1), (1, 1), (1, 2)], [(0, 1, CHAIN), (1, 2, CHAIN), (1, 1, CHAIN),
                                                                                 (1, 1, FAN)], 0, 0, [1, 0, 0, 1, 2, 2, 1]),
         dict(scaled=3, cams=3)),
        ("fans", _graph([(0, 1), (0, 2), (0, 3), (3, 4)], [(0, 1, FAN), (1, 2, FAN), (2, 3, CHAIN)], 0, 0, range(4)),
         dict(scaled=4, cams=5)),
        ("no links", _graph(SEQ, [], 1, 1, range(5)), dict(scaled=1, cams=2)),
        ("no walk", _graph(SEQ, SEQ_LINKS, 0, 3, []), dict(scaled=5, cams=1)),
    ]
    if serial_words:
        reps = serial_words // (3 * len(SEQ_LINKS)) + 1          # the links' list alone exceeds what step 2 stages
        out.append(("more links than step 2 stages", _graph(SEQ, SEQ_LINKS, 0, 0, range(5), repeat_links=reps),
                    dict(scaled=5, cams=6)))
    return out


# ---- planted scenes: cameras on a curved path, pair rows through find -> improve -> recover_pose

SCENE = dict(ncams=8, n=400, noise=0.5, outliers=0.25, find_loops=256, improve_loops=5, thresh=1.0, max_error=2.0)
_SCENE = {}


def camera_path(ncams, rng, steps=None, turn=lambda i: 0.03 * (i + 1)):
    """World-to-camera (R_i, t_i), X_i = R_i X + t_i, camera 0 at the identity: centres on a curve, baselines of unequal
    length, each camera turned a little further."""
    if steps is None:
        steps = np.geomspace(0.12, 0.6, ncams - 1)[rng.permutation(ncams - 1)]        # a factor of 5
    R, C = [np.eye(3)], [np.zeros(3)]
    for i, s in enumerate(steps):
        heading = 0.25 * i
        d = np.array([np.cos(heading), 0.15 * np.sin(1.7 * i), np.sin(heading) * 0.6])
        C.append(C[-1] + s * d / np.linalg.norm(d))
        R.append(PC.rodrigues([0.2, 1.0, 0.1], turn(i)) @ PC.rodrigues(rng.normal(0, 1, 3), 0.01))
    return [(r, -r @ c) for r, c in zip(R, C)]


def window_pairs(ncams):
    """The pairs (i, i + 1) then (i, i + 2), the CHAIN links along the sequence and the FAN links onto the skips, in
    outward order from pair 0; the walk is the consecutive pairs."""
    pairs = [(i, i + 1) for i in range(ncams - 1)] + [(i, i + 2) for i in range(ncams - 2)]
    links = [(i, i + 1, CHAIN) for i in range(ncams - 2)] + [(i, ncams - 1 + i, FAN) for i in range(ncams - 2)]
    return pairs, links, list(range(ncams - 1))


def scene_rows(cams, X, rng, noise, outliers, pairs, K4=PC.K_A):
    """Per-image observations and record orders, and for each of the pairs the rows a pair matcher would leave: xpos /
    ypos of the set-1 record, match and match_xpos / match_ypos of the set-2 record, a share wrong.  (rows, inliers)."""
    K = PC.kmat(K4)
    n = len(X)
    obs, order = [], []
    for R, t in cams:
        x = (K @ ((R @ X.T).T + t).T).T
        order.append(rng.permutation(n))                         # record order[j] holds point j
        o = np.zeros((n, 2))
        o[order[-1]] = x[:, :2] / x[:, 2:] + rng.normal(0, noise, (n, 2))
        obs.append(o)
    rows, inl = [], []
    for p, (a, b) in enumerate(pairs):
        point = np.argsort(order[a])                             # the point of record r of image a
        m = order[b][point]
        good = np.ones(n, bool)
        if outliers:
            good[rng.choice(n, int(n * outliers), replace=False)] = False
            m = np.where(good, m, (m + rng.integers(1, n, n)) % n)
        r = PC.records(np.concatenate([obs[a], obs[b][m]], 1), 900 + p)
        r["match"], r["match_error"] = m, 0
        rows.append(r)
        inl.append(good)
    return rows, inl


def pair_chain(rows, K8, find_seed, S):
    """find -> improve -> recover_pose restated on one pair's rows: (rows as improve leaves them, F, expected_pose)."""
    from test_fundamental_cpu import expected_find
    from test_fundamental_refine_cpu import expected_improve
    n = len(rows)
    with np.errstate(all="ignore"):
        F0, _ = expected_find(rows, n, find_seed, S["find_loops"], *GATES, S["thresh"], max_pts=n)
        out, F, _, _ = expected_improve(rows, n, F0, S["improve_loops"], *GATES, S["thresh"])
        return out, F, PC.expected_pose(out, n, F, K8, *GATES, S["thresh"])


def planted_scene(seed=31, **kw):
    """The 8-camera scene: dict(case, cams, pairs, links, raw rows, find seeds, F per pair, K8, inl)."""
    S = dict(SCENE, **kw)
    key = (seed,) + tuple(sorted(S.items()))
    if key not in _SCENE:
        rng = np.random.default_rng(seed)
        cams = camera_path(S["ncams"], rng)
        X = rng.uniform([-4, -2.5, 5], [5, 2.5, 12], (S["n"], 3))
        pairs, links, walk = window_pairs(S["ncams"])
        raw, inl = scene_rows(cams, X, rng, S["noise"], S["outliers"], pairs)
        K8 = np.array(PC.K_A + PC.K_A, f32)
        seeds = [40 + p for p in range(len(pairs))]
        done = [pair_chain(r, K8, s, S) for r, s in zip(raw, seeds)]
        case = dict(pairs=np.array(pairs, np.int32), nimages=S["ncams"], rows=np.concatenate([d[0] for d in done]),
                    row_counts=np.full(len(pairs), S["n"], np.int32), max_pts=S["n"], max_error=S["max_error"],
                    pose=np.stack([d[2]["pose"] for d in done]),
                    num_front=np.array([d[2]["num_front"] for d in done], np.int32),
                    xyz=np.concatenate([d[2]["xyz"] for d in done]), links=np.array(links, np.int32), seed_pair=0,
                    root_image=0, min_common=MIN_COMMON, walk=np.array(walk, np.int32))
        _SCENE[key] = dict(case=case, cams=cams, pairs=pairs, links=links, raw=raw, seeds=seeds,
                           F=np.stack([d[1] for d in done]), K8=K8, inl=inl, S=S)
    return _SCENE[key]


def exact_chain(ncams=64, n=64, seed=32):
    """A chain of ncams images from exact rows: no noise, no wrong match, the exact F of each planted pose; the rows are
    the pairs (i, i + 1) only."""
    key = ("exact", ncams, n, seed)
    if key not in _SCENE:
        rng = np.random.default_rng(seed)
        cams = camera_path(ncams, rng, steps=rng.uniform(0.12, 0.6, ncams - 1), turn=lambda i: 0.25 * np.sin(0.3 * i))
        centre = np.mean([-r.T @ t for r, t in cams], 0)
        X = centre + rng.uniform([-6, -3, 9], [6, 3, 18], (n, 3))
        K, K8 = PC.kmat(PC.K_A), np.array(PC.K_A + PC.K_A, f32)
        pairs = [(i, i + 1) for i in range(ncams - 1)]
        rows, pose, front, xyz = [], [], [], []
        for p, (a, b) in enumerate(pairs):
            (Ra, ta), (Rb, tb) = cams[a], cams[b]
            R, t = Rb @ Ra.T, tb - Rb @ Ra.T @ ta
            xa, xb = (K @ ((Ra @ X.T).T + ta).T).T, (K @ ((Rb @ X.T).T + tb).T).T
            r = PC.records(np.concatenate([xa[:, :2] / xa[:, 2:], xb[:, :2] / xb[:, 2:]], 1), 1200 + p)
            r["match"], r["match_error"] = np.arange(n), 0
            F = np.linalg.inv(K).T @ PC.skew(t) @ R @ np.linalg.inv(K)
            F = (F / np.abs(F).max()).astype(f32).reshape(9)
            with np.errstate(all="ignore"):
                e = PC.expected_pose(r, n, F, K8, *GATES, 1.0)
            rows.append(r), pose.append(e["pose"]), front.append(e["num_front"]), xyz.append(e["xyz"])
        links = [(i, i + 1, CHAIN) for i in range(ncams - 2)]
        case = dict(pairs=np.array(pairs, np.int32), nimages=ncams, rows=np.concatenate(rows),
                    row_counts=np.full(len(pairs), n, np.int32), max_pts=n, max_error=INF, pose=np.stack(pose),
                    num_front=np.array(front, np.int32), xyz=np.concatenate(xyz), links=np.array(links, np.int32),
                    seed_pair=0, root_image=0, min_common=MIN_COMMON, walk=np.arange(len(pairs), dtype=np.int32))
        _SCENE[key] = dict(case=case, cams=cams, pairs=pairs, links=links)
    return _SCENE[key]


def planted_ratio(cams, pairs, link):
    """|T_p| / |T_q| of a link: the baselines are the distances of the camera centres."""
    def base(p):
        (Ra, ta), (Rb, tb) = cams[pairs[p][0]], cams[pairs[p][1]]
        return np.linalg.norm(Ra.T @ ta - Rb.T @ tb)
    return base(link[0]) / base(link[1])


def planted_cameras(cams, root, seed_pair_images):
    """The planted cameras with the root at the identity and the seed pair's baseline as the unit: (n, 12) float64."""
    Rr, tr = cams[root]
    (Ra, ta), (Rb, tb) = cams[seed_pair_images[0]], cams[seed_pair_images[1]]
    unit = np.linalg.norm(Ra.T @ ta - Rb.T @ tb)
    return np.array([np.concatenate([(R @ Rr.T).reshape(9), (t - R @ Rr.T @ tr) / unit]) for R, t in cams])


def link_poses64(case, gates=GATES):
    """The call in float64 on the same rows, the same samples and the same poses: (ratios, scales, cameras)."""
    links = np.asarray(case["links"], np.int64).reshape(-1, 3)
    ratio = np.zeros(len(links))
    for l, (p, q, kind) in enumerate(links):
        (rp, zp, cp), (rq, zq, cq) = pair_block(case, p), pair_block(case, q)
        r, _ = samples(rp, zp, cp, rq, zq, cq, case["max_pts"], kind, case["max_error"], gates)
        if len(r) >= case["min_common"]:
            r2 = rp["match"][r] if kind == CHAIN else r
            rho = zq[r2, 2].astype(np.float64) / zp[r, 3 if kind == CHAIN else 2].astype(np.float64)
            ratio[l] = np.sort(rho)[(len(rho) - 1) >> 1]
    pairs, pose = np.asarray(case["pairs"]).reshape(-1, 2), np.asarray(case["pose"], np.float64).reshape(-1, 12)
    usable = usable_pairs(case["pose"], case["num_front"])
    scale = np.zeros(len(pairs))
    scale[case["seed_pair"]] = 1.0 if usable[case["seed_pair"]] else 0.0
    for (p, q, _), rho in zip(links, ratio):
        if rho > 0 and usable[p] and usable[q]:
            if scale[p] > 0 and scale[q] == 0:
                scale[q] = scale[p] / rho
            elif scale[q] > 0 and scale[p] == 0:
                scale[p] = scale[q] * rho
    cam, have = np.zeros((case["nimages"], 12)), np.zeros(case["nimages"], bool)
    cam[case["root_image"], [0, 4, 8]] = 1
    have[case["root_image"]] = True
    for p in case["walk"]:
        a, b = pairs[p]
        R, t, s = pose[p, :9].reshape(3, 3), pose[p, 9:], scale[p]
        if s > 0 and a != b and have[a] != have[b]:
            if have[a]:
                cam[b] = np.concatenate([(R @ cam[a, :9].reshape(3, 3)).reshape(9), R @ cam[a, 9:] + s * t])
            else:
                cam[a] = np.concatenate([(R.T @ cam[b, :9].reshape(3, 3)).reshape(9), R.T @ (cam[b, 9:] - s * t)])
            have[a] = have[b] = True
    return ratio, scale, cam

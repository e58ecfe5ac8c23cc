"""misift_correspond_tracks_batch, misift_align_points_batch and misift_transform_scene_batch: expected_correspond,
expected_align and expected_transform, the numpy restatement of the definitions in include/misift.h, the wrappers of the
library's host hooks, and the cases of their tests (test_align_cpu.py pins the restatement to the hooks and to float64 and
asserts the premises of the cases, test_gpu_align.py holds the device to it byte for byte).  The restatement takes its
number format as an argument: with float32 every operation is rounded as the library rounds it, with float64 the same
algorithm is the yardstick.  No GPU in here, and cudasift_amd.capi is imported inside functions only."""
import numpy as np

from batch_util import POISON_WORD
from test_fundamental_cpu import f32, libc_stream

OK, FEW_CAND, NO_MODEL = 0, 1, 2
UNSET = -2
SWEEPS, SLOTS = 6, 256
ALIGN_OUTPUTS = ("sim", "align_cand", "align_inliers", "align_status", "summary")
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


# ---- misift_align_points_batch restated

def draw3(seed, n, num_loops):
    """Step 2: (num_loops, 3) positions: per hypothesis three draws first, then p[1] and p[2] in turn redrawn while they
    repeat an earlier one; all hypotheses from one stream."""
    need = 8 * num_loops + 64
    while True:
        r = iter(libc_stream(seed, need).tolist())
        out = np.zeros((num_loops, 3), np.int64)
        try:
            for i in range(num_loops):
                p = [next(r) % n for _ in range(3)]
                for k in range(1, 3):
                    while p[k] in p[:k]:
                        p[k] = next(r) % n
                out[i] = p
            return out
        except StopIteration:
            need *= 4


def finite(v):
    return np.abs(v) <= np.finfo(v.dtype).max


def from_moments(S, ca, cb, dt):
    """Steps 3c to 3e on L sets of sums: S (L, 11) = the nine moments row-major, sa, sb; ca, cb (L, 3).  Returns
    (h (L, 13) of dt: R row-major, t, s; ok (L,)); an INVALID row is thirteen NaNs."""
    one, two = dt(1), dt(2)
    L = len(S)
    M = S[:, :9]
    sa, sb = S[:, 9], S[:, 10]
    ok = finite(M).all(1)
    m = np.abs(M).max(1)
    m = np.where(np.isnan(m), dt(0), m)                          # v > m is false for a NaN
    ok &= m != 0
    A = [[M[:, 3 * r + c] / m for c in range(3)] for r in range(3)]
    V = [[np.full(L, 1 if r == c else 0, dt) for c in range(3)] for r in range(3)]

    def dot(X, i, j):
        return X[0][i] * X[0][j] + X[1][i] * X[1][j] + X[2][i] * X[2][j]

    for _ in range(SWEEPS):
        for a, b in ((0, 1), (0, 2), (1, 2)):
            alpha, beta, gamma = dot(A, a, a), dot(A, b, b), dot(A, a, b)
            skip = gamma == 0
            zeta = (beta - alpha) / (two * gamma)
            tau = one / (np.abs(zeta) + np.sqrt(one + zeta * zeta))
            tau = np.where(zeta < 0, -tau, tau)
            cs = one / np.sqrt(one + tau * tau)
            sn = cs * tau
            for X in (A, V):
                for r in range(3):
                    xa, xb = X[r][a], X[r][b]
                    X[r][a] = np.where(skip, xa, cs * xa - sn * xb)
                    X[r][b] = np.where(skip, xb, sn * xa + cs * xb)
    w = [dot(A, j, j) for j in range(3)]
    i1 = np.where(w[1] > w[0], 1, 0)
    i1 = np.where(w[2] > np.where(i1 == 0, w[0], w[1]), 2, i1)
    ja, jb = np.where(i1 == 0, 1, 0), np.where(i1 == 2, 1, 2)
    wa, wb = np.where(ja == 0, w[0], w[1]), np.where(jb == 1, w[1], w[2])
    i2 = np.where(wb > wa, jb, ja)
    w1 = np.where(i1 == 0, w[0], np.where(i1 == 1, w[1], w[2]))
    w2 = np.where(wb > wa, wb, wa)
    ok &= (w2 > 0) & (w2 > w1 * dt(f32(1e-10)))

    def column(X, i):
        return [np.where(i == 0, X[r][0], np.where(i == 1, X[r][1], X[r][2])) for r in range(3)]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    n1, n2 = np.sqrt(w1), np.sqrt(w2)
    u1, u2 = [x / n1 for x in column(A, i1)], [x / n2 for x in column(A, i2)]
    v1, v2 = column(V, i1), column(V, i2)
    u3, v3 = cross(u1, u2), cross(v1, v2)
    h = np.zeros((L, 13), dt)
    for r in range(3):
        for c in range(3):
            h[:, 3 * r + c] = (u1[r] * v1[c] + u2[r] * v2[c]) + u3[r] * v3[c]
    ok &= sa != 0
    s = np.sqrt(sb / sa)
    ok &= (s != 0) & finite(s)
    for r in range(3):
        h[:, 9 + r] = cb[:, r] - s * ((h[:, 3 * r] * ca[:, 0] + h[:, 3 * r + 1] * ca[:, 1]) + h[:, 3 * r + 2] * ca[:, 2])
    h[:, 12] = s
    ok &= finite(h).all(1)
    h[~ok] = np.nan
    return h, ok


def moment_terms(a, b, ca, cb):
    """Step 3b: the eleven terms of correspondences a, b (..., 3) under the centroids ca, cb -> (..., 11)."""
    da, db = a - ca, b - cb
    x = [db[..., r] * da[..., c] for r in range(3) for c in range(3)]
    x.append((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2])
    x.append((db[..., 0] * db[..., 0] + db[..., 1] * db[..., 1]) + db[..., 2] * db[..., 2])
    return np.stack(x, -1)


def solve3(a, b, dt=f32):
    """Step 3 for L samples: a, b (L, 3, 3) float32, sample k at [:, k].  Returns (h (L, 13) of dt, valid (L,))."""
    a, b = np.asarray(a, f32).astype(dt), np.asarray(b, f32).astype(dt)
    with np.errstate(all="ignore"):
        ca = (((dt(0) + a[:, 0]) + a[:, 1]) + a[:, 2]) / dt(3)
        cb = (((dt(0) + b[:, 0]) + b[:, 1]) + b[:, 2]) / dt(3)
        S = np.zeros((len(a), 11), dt)
        for k in range(3):
            S = S + moment_terms(a[:, k], b[:, k], ca, cb)
        return from_moments(S, ca, cb, dt)


def error2(h, a, b, dt=f32):
    """Step 4: E2 (L, n) of the candidates a, b (n, 3) under the transforms h (L, 13)."""
    h = np.asarray(h, dt).reshape(-1, 13)
    a, b = np.asarray(a, f32).astype(dt), np.asarray(b, f32).astype(dt)
    s = h[:, 12, None]
    d = []
    with np.errstate(all="ignore"):
        for r in range(3):
            p = s * ((h[:, 3 * r, None] * a[None, :, 0] + h[:, 3 * r + 1, None] * a[None, :, 1]) +
                     h[:, 3 * r + 2, None] * a[None, :, 2]) + h[:, 9 + r, None]
            d.append(b[None, :, r] - p)
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def thresh2_of(thresh, dt):
    with np.errstate(all="ignore"):
        return f32(thresh) * f32(thresh) if dt is f32 else dt(f32(thresh)) * dt(f32(thresh))


def count_members(h, a, b, thresh, dt=f32):
    """The members of every hypothesis (L,) over the n candidates."""
    t2 = thresh2_of(thresh, dt)
    out = np.zeros(len(h), np.int64)
    for at in range(0, len(h), 256):
        out[at:at + 256] = (error2(h[at:at + 256], a, b, dt) < t2).sum(1)
    return out


def slot_sum(v, member, dt):
    """The sum of step 6: v (n, K) over the candidates with member (n,) true -> (K,).  Slot t adds its members
    p = t, t + 256, ... in ascending order from +0 (a candidate that is no member is skipped), then the halving tree."""
    v = np.asarray(v, dt)
    n, K = v.shape
    rows = max(-(-n // SLOTS), 1)
    V, M = np.zeros((rows * SLOTS, K), dt), np.zeros(rows * SLOTS, bool)
    V[:n], M[:n] = v, member
    p = np.zeros((SLOTS, K), dt)
    with np.errstate(all="ignore"):
        for j in range(rows):
            sl = slice(j * SLOTS, (j + 1) * SLOTS)
            p = np.where(M[sl, None], p + V[sl], p)
        off = SLOTS // 2
        while off:
            p[:off] = p[:off] + p[off:2 * off]
            off //= 2
    return p[0].copy()


def refit(a, b, h, thresh, refit_loops, dt=f32):
    """Step 6 on the candidates a, b (n, 3) from the transform h (13,): dict(h, members, kept, rms, member (n,) bool,
    history: the member counts of the transforms tried)."""
    a32, b32 = np.asarray(a, f32), np.asarray(b, f32)
    a, b = a32.astype(dt), b32.astype(dt)
    t2 = thresh2_of(thresh, dt)
    h = np.asarray(h, dt).copy()
    with np.errstate(all="ignore"):
        mem = error2(h, a32, b32, dt)[0] < t2
        c, kept, history = int(mem.sum()), 0, []
        for _ in range(refit_loops):
            if c < 1:
                break
            C = slot_sum(np.concatenate([a, b], 1), mem, dt)
            ca, cb = C[:3] / dt(c), C[3:] / dt(c)
            S = slot_sum(moment_terms(a, b, ca, cb), mem, dt)
            hp, ok = from_moments(S[None], ca[None], cb[None], dt)
            if not ok[0]:
                history.append(-1)
                break
            memp = error2(hp[0], a32, b32, dt)[0] < t2
            cp = int(memp.sum())
            history.append(cp)
            if cp < c:
                break
            h, c, mem, kept = hp[0], cp, memp, kept + 1
        E = slot_sum(error2(h, a32, b32, dt)[0][:, None], mem, dt)
        rms = np.sqrt(E[0] / dt(c)) if c > 0 else dt(0)
    return dict(h=h, members=c, kept=kept, rms=dt(rms), member=mem, history=history)


def candidates(case, e):
    """Step 1: (the source indices i of the candidates of entry e in ascending order, a (n, 3), b (n, 3) float32)."""
    sf, sc, df, dc = (int(v) for v in case["ranges"][e])
    ne = sc
    if case.get("count") is not None:
        ne = min(max(int(case["count"][e * case["count_stride"]]), 0), sc)
    src, dst = np.asarray(case["src"], f32).reshape(-1, 4), np.asarray(case["dst"], f32).reshape(-1, 4)
    m = np.asarray(case["map"], np.int64)[sf:sf + ne]
    ok = (m >= 0) & (m < dc)
    mm = np.where(ok, m, 0)
    if case.get("src_status") is not None:
        ok &= np.asarray(case["src_status"])[sf:sf + ne] == 0
    if case.get("dst_status") is not None:
        ok &= np.asarray(case["dst_status"])[df + mm] == 0
    a, b = src[sf:sf + ne, :3], dst[df + mm, :3]
    with np.errstate(invalid="ignore"):
        ok &= finite(a).all(1) & finite(b).all(1)
    i = np.nonzero(ok)[0]
    return i, a[i], b[i]


def search(seed, a, b, num_loops, thresh, dt=f32):
    """Steps 2 to 5 over n >= 3 candidates: dict(hyps, valid, counts, index, inliers, samples)."""
    pos = draw3(seed, len(a), num_loops)
    hyps, valid = solve3(a[pos], b[pos], dt)
    counts = count_members(hyps, a, b, thresh, dt)
    idx = int(np.argmax(counts))                                 # the first maximum
    return dict(hyps=hyps, valid=valid, counts=counts, index=idx, inliers=int(counts[idx]), samples=pos)


def expected_entry(case, e, dt=f32):
    """One entry: dict(sim (16,), cand, inliers, status, kept, index (the candidates' source indices), member (bool per
    candidate), search, refit)."""
    i, a, b = candidates(case, e)
    out = dict(sim=np.zeros(16, dt), cand=len(i), inliers=0, status=OK, kept=0, index=i,
               member=np.zeros(len(i), bool), search=None, refit=None)
    if len(i) < max(3, case["min_inliers"]):
        out["status"] = FEW_CAND
        return out
    memo = case.setdefault("memo", {})
    key = (e, int(case["seeds"][e]), case["num_loops"], float(case["thresh"]), dt)
    if key not in memo:
        memo[key] = search(int(case["seeds"][e]), a, b, case["num_loops"], case["thresh"], dt)
    s = out["search"] = memo[key]
    out["inliers"] = s["inliers"]
    if s["inliers"] < case["min_inliers"]:
        out["status"] = NO_MODEL
        return out
    r = out["refit"] = refit(a, b, s["hyps"][s["index"]], case["thresh"], case["refit_loops"], dt)
    out["sim"][:13], out["sim"][13] = r["h"], r["rms"]
    out["inliers"], out["kept"], out["member"] = r["members"], r["kept"], r["member"]
    return out


def expected_align(case, dt=f32):
    """The outputs of the call as uint32 arrays of exactly the stated sizes (inlier: one word per source point of the
    pool, POISON_WORD where the call must not write), and the per-entry dicts under 'entries'."""
    nsel = len(case["ranges"])
    ents = [expected_entry(case, e, dt) for e in range(nsel)]
    summary = np.zeros(8, np.int32)
    inlier = np.full(len(np.asarray(case["map"])), POISON_WORD, np.uint32).view(np.int32)
    for e, x in enumerate(ents):
        summary[(0, 2, 3)[x["status"]]] += 1
        summary[4] += x["cand"]
        if x["status"] == OK:
            summary[1] += x["inliers"]
            summary[5] += x["kept"]
        sf, sc = int(case["ranges"][e][0]), int(case["ranges"][e][1])
        inlier[sf:sf + sc] = -1
        inlier[sf + x["index"]] = x["member"].astype(np.int32)
    sim = np.array([x["sim"] for x in ents], f32).reshape(-1)
    ints = {k: np.array([x[k] for x in ents], np.int32).view(np.uint32) for k in ("cand", "inliers", "status")}
    return dict(sim=sim.view(np.uint32), align_cand=ints["cand"], align_inliers=ints["inliers"],
                align_status=ints["status"], summary=summary.view(np.uint32), inlier=inlier.view(np.uint32),
                entries=ents)


# ---- misift_correspond_tracks_batch restated

def clamp(v, hi):
    return min(max(int(v), 0), hi)


def track_of(off, T, o):
    if T < 1:
        return -1
    lo, hi = 0, T
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if off[mid] <= o:
            lo = mid
        else:
            hi = mid
    return lo if off[lo] <= o < off[lo + 1] else -1


def expected_correspond(case):
    """dict(map: max_tracks_a uint32 words, POISON_WORD beyond T_A; summary: 8 words; ties: the list of (g, t_A, t_B))."""
    A, B, shift = case["a"], case["b"], case["shift"]
    TA, OA = clamp(A["export_summary"][2], A["max_tracks"]), clamp(A["export_summary"][3], A["max_obs"])
    TB, OB = clamp(B["export_summary"][2], B["max_tracks"]), clamp(B["export_summary"][3], B["max_obs"])
    offa, offb = [int(v) for v in A["track_offsets"]], [int(v) for v in B["track_offsets"]]
    ties = []
    for g in range(A["max_records"]):
        gb = g - shift
        if not 0 <= gb < B["max_records"]:
            continue
        oa, ob = int(A["record_obs"][g]), int(B["record_obs"][gb])
        if not (0 <= oa < OA and 0 <= ob < OB):
            continue
        ta, tb = track_of(offa, TA, oa), track_of(offb, TB, ob)
        if ta >= 0 and tb >= 0:
            ties.append((g, ta, tb))
    out = np.full(A["max_tracks"], POISON_WORD, np.uint32).view(np.int32)
    out[:TA] = -1
    for _, ta, tb in ties:
        out[ta] = tb if out[ta] in (-1, tb) else -2
    summary = np.zeros(8, np.int32)
    summary[:5] = TA, TB, len(ties), (out[:TA] >= 0).sum(), (out[:TA] == -2).sum()
    return dict(map=out.view(np.uint32), summary=summary.view(np.uint32), ties=ties)


# ---- misift_transform_scene_batch restated

def one_nan(v):
    """A computed NaN is stored as 0x7fc00000."""
    v = np.asarray(v, f32).copy()
    v[np.isnan(v)] = np.uint32(0x7fc00000).view(f32)
    return v


def transform_points(sim, X, dt=f32):
    sim, X = np.asarray(sim, f32).astype(dt), np.asarray(X, f32).astype(dt).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([sim[12] * ((sim[3 * r] * X[:, 0] + sim[3 * r + 1] * X[:, 1]) + sim[3 * r + 2] * X[:, 2]) +
                         sim[9 + r] for r in range(3)], 1)


def transform_cameras(sim, cam, dt=f32):
    sim, cam = np.asarray(sim, f32).astype(dt), np.asarray(cam, f32).astype(dt).reshape(-1, 12)
    out = np.zeros_like(cam)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                out[:, 3 * r + c] = (cam[:, 3 * r] * sim[3 * c] + cam[:, 3 * r + 1] * sim[3 * c + 1]) + \
                    cam[:, 3 * r + 2] * sim[3 * c + 2]
            out[:, 9 + r] = sim[12] * cam[:, 9 + r] - ((out[:, 3 * r] * sim[9] + out[:, 3 * r + 1] * sim[10]) +
                                                       out[:, 3 * r + 2] * sim[11])
    return out


def expected_transform(case):
    """dict(points_out: 4 max_tracks words, cam_out: 12 nimages words), uint32."""
    pts = np.ascontiguousarray(case["points"], f32).reshape(-1, 4).copy()
    cam = np.ascontiguousarray(case["cam"], f32).reshape(-1, 12).copy()
    apply = case.get("sim_status") is None or int(case["sim_status"]) == 0
    if apply:
        T = clamp(case["export_summary"][2], case["max_tracks"])
        on = np.zeros(len(pts), bool)
        on[:T] = np.asarray(case["point_status"])[:T] == 0
        pts[on, :3] = one_nan(transform_points(case["sim"], pts[on, :3]))
        on = np.asarray(case["cam_pair"]) != UNSET
        cam[on] = one_nan(transform_cameras(case["sim"], cam[on]))
    return dict(points_out=pts.reshape(-1).view(np.uint32), cam_out=cam.reshape(-1).view(np.uint32))


# ---- the hooks

def hook_samples(seed, n, num_loops):
    from cudasift_amd import capi
    out = np.full((max(num_loops, 1), 3), -77, np.int32)
    assert capi.lib().misift_test_align_samples(seed, n, num_loops, out.ctypes.data) == 0
    return out[:num_loops]


def hook_solve(a, b):
    """The library's solve of one sample a, b (3, 3): (h (13,) float32, valid)."""
    from cudasift_amd import capi
    a, b = np.ascontiguousarray(a, f32).reshape(9), np.ascontiguousarray(b, f32).reshape(9)
    h, valid = np.full(13, 3.5, f32), np.full(1, -77, np.int32)
    assert capi.lib().misift_test_align_solve(a.ctypes.data, b.ctypes.data, h.ctypes.data, valid.ctypes.data) == 0
    return h, int(valid[0])


def hook_refit(a, b, h, thresh, refit_loops):
    """The library's step 6: (h (13,), members, kept, rms)."""
    from cudasift_amd import capi
    a, b = np.ascontiguousarray(a, f32).reshape(-1, 3), np.ascontiguousarray(b, f32).reshape(-1, 3)
    h = np.ascontiguousarray(h, f32).copy()
    counts, rms = np.full(2, -77, np.int32), np.full(1, 3.5, f32)
    assert capi.lib().misift_test_align_refit(a.ctypes.data, b.ctypes.data, len(a), float(thresh), refit_loops,
                                              h.ctypes.data, counts.ctypes.data, rms.ctypes.data) == 0
    return h, int(counts[0]), int(counts[1]), rms[0]


def hook_transform_camera(sim, cam):
    from cudasift_amd import capi
    sim, cam = np.ascontiguousarray(sim, f32), np.ascontiguousarray(cam, f32).reshape(12)
    out = np.full(12, 3.5, f32)
    assert capi.lib().misift_test_transform_camera(sim.ctypes.data, cam.ctypes.data, out.ctypes.data) == 0
    return out


def hook_transform_point(sim, x):
    from cudasift_amd import capi
    sim, x = np.ascontiguousarray(sim, f32), np.ascontiguousarray(x, f32).reshape(3)
    out = np.full(3, 3.5, f32)
    assert capi.lib().misift_test_transform_point(sim.ctypes.data, x.ctypes.data, out.ctypes.data) == 0
    return out


# ---- cases of the alignment

_MEMO = {}


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def planted_pairs(n, seed, wrong=0.25, noise=0.01, disp=2.0):
    """n correspondences b = s R a + t + noise; a share `wrong` of them displaced by `disp` units in a random direction.
    dict(a (n, 3) float32, b (n, 3) float32, good (n,) bool, R, t, s: the planted transform in float64)."""
    key = ("pairs", n, seed, wrong, noise, disp)
    if key in _MEMO:
        return _MEMO[key]
    rng = np.random.default_rng(seed)
    R, t, s = rotation(rng), rng.uniform(-5, 5, 3), rng.uniform(0.5, 3.0)
    a = rng.uniform(-4, 4, (n, 3)).astype(f32)
    b = s * a.astype(np.float64) @ R.T + t + rng.normal(0, noise, (n, 3))
    bad = np.zeros(n, bool)
    bad[rng.choice(n, int(round(wrong * n)), replace=False)] = True
    d = rng.normal(size=(n, 3))
    b[bad] += disp * d[bad] / np.linalg.norm(d[bad], axis=1, keepdims=True)
    out = dict(a=a, b=b.astype(f32), good=~bad, R=R, t=t, s=s)
    _MEMO[key] = out
    return out


def align_case(entries, seeds=None, num_loops=64, thresh=0.05, min_inliers=3, refit_loops=2, status=True, count=None,
               count_stride=1, pad=(3, 5), slack=0, perm_seed=5):
    """A case from a list of (a (n, 3), b (n, 3)) entries pooled one after another: the correspondents of entry e are
    shuffled among its own range of dst; `pad` points lie before the first entry in src and dst, `slack` more source
    slots per entry lie behind its points (map -1).  The fourth words hold a pattern that must not matter."""
    rng = np.random.default_rng(perm_seed)
    src, dst, mp, ranges = [np.full((pad[0], 4), 7.5, f32)], [np.full((pad[1], 4), -7.5, f32)], [np.full(pad[0], -1)], []
    sf, df = pad
    for a, b in entries:
        n = len(a)
        perm = rng.permutation(n)
        s4, d4 = np.full((n + slack, 4), 1e30, f32), np.full((max(n, 1), 4), -1e30, f32)
        s4[:n, :3] = a
        d4[perm, :3] = b
        m = np.full(n + slack, -1, np.int64)
        m[:n] = perm
        src.append(s4), dst.append(d4), mp.append(m)
        ranges.append((sf, max(n + slack, 1), df, max(n, 1)))
        if n + slack == 0:
            src.append(np.full((1, 4), 2.5, f32)), mp.append(np.full(1, -1))
        sf, df = sf + max(n + slack, 1), df + max(n, 1)
    src, dst, mp = np.concatenate(src), np.concatenate(dst), np.concatenate(mp).astype(np.int32)
    nsel = len(entries)
    seeds = np.asarray([100 + 7 * e for e in range(nsel)] if seeds is None else seeds, np.uint32)
    return dict(src=src, dst=dst, map=mp, ranges=np.array(ranges, np.int32).reshape(-1, 4), seeds=seeds,
                src_status=np.zeros(len(src), np.int32) if status else None,
                dst_status=np.zeros(len(dst), np.int32) if status else None, count=count, count_stride=count_stride,
                num_loops=num_loops, thresh=thresh, min_inliers=min_inliers, refit_loops=refit_loops, want_inlier=True)


def variant(case, **kw):
    out = {k: v for k, v in case.items() if k != "memo"}
    out.update(kw)
    return out


def pairs_of(n, seed, **kw):
    p = planted_pairs(n, seed, **kw)
    return p["a"], p["b"]


def hostile_case(**kw):
    """120 planted correspondences with hostile entries among them: map values -1, -2, INT_MIN, dst_cap and INT_MAX,
    NaN / inf / 1e20 coordinates on either side, non-zero statuses on either side."""
    case = align_case([pairs_of(120, 31)], **kw)
    sf, sc, df, dc = (int(v) for v in case["ranges"][0])
    case["map"][sf + np.arange(5)] = [-1, -2, INT_MIN, dc, INT_MAX]
    case["src"][sf + 10, 0], case["src"][sf + 11, 1], case["src"][sf + 12, 2] = np.nan, np.inf, -np.inf
    case["src"][sf + 13, 0] = 1e20                               # finite: a candidate that fits nothing
    for k, i in enumerate((20, 21, 22)):
        case["dst"][df + case["map"][sf + i], k] = (np.nan, np.inf, -np.inf)[k]
    case["dst"][df + case["map"][sf + 23], 1] = -1e20
    case["src_status"][sf + 30], case["src_status"][sf + 31] = 1, -1
    case["dst_status"][df + case["map"][sf + 40]], case["dst_status"][df + case["map"][sf + 41]] = 3, INT_MIN
    return case


def line_pairs(n, seed):
    """n correspondences on the x axis, b = 2 a + 1 along it: every centred sample has y = z = 0 exactly, so its moment
    matrix has one non-zero entry and the second-largest w is exactly 0.  (Points on a line in a general direction are
    collinear only up to rounding: such a sample is valid and ill-conditioned, see test_align_cpu.py.)"""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 3), f32)
    a[:, 0] = rng.uniform(-3, 3, n)
    b = np.zeros((n, 3), f32)
    b[:, 0] = a[:, 0] * f32(2) + f32(1)
    return a, b


def skew_line_pairs(n, seed):
    """n correspondences on a line along (1, 2, -0.5), b = 2 a: collinear up to rounding only, so the second-largest w
    of a sample is the roundings of M / m, positive but below 1e-10 of the largest."""
    rng = np.random.default_rng(seed)
    a = np.outer(rng.uniform(-3, 3, n), [1.0, 2.0, -0.5]).astype(f32)
    return a, (a * f32(2)).astype(f32)


def same_pairs(n):
    return np.tile(np.array([1.0, 2.0, 3.0], f32), (n, 1)), np.tile(np.array([-1.0, 0.5, 2.0], f32), (n, 1))


def turned_away_pairs():
    """40 exact correspondences of which nine are moved by +0.19 and one by -0.19 along x in dst.  Under thresh 0.2 the
    exact transform holds all forty; its refit moves towards the nine and loses the one, so it is turned away."""
    p = planted_pairs(40, 41, wrong=0.0, noise=0.0)
    a, b = p["a"].copy(), p["b"].copy()
    b[30:39, 0] += f32(0.19)
    b[39, 0] -= f32(0.19)
    return a, b


GPU_CASES = (
    "candidates 0 2 3 4", "candidates 511 512", "candidates 513 1025", "collinear, identical", "count below at beyond",
    "count negative, stride 8", "four entries", "hostile", "min_inliers count +0", "min_inliers count +1",
    "min_inliers count -1", "no inlier, no status", "nsel 0", "num_loops 1", "num_loops 100", "num_loops 63",
    "num_loops 64", "num_loops 65", "refit_loops 0", "refit_loops 1", "refit_loops 5", "seed a", "seed b",
    "slots wrap", "src_cap 37", "thresh inf", "turned away",
)


def gpu_cases():
    """name -> case: everything test_gpu_align.py compares byte for byte; test_align_cpu.py asserts what each is built to
    hit."""
    if "gpu" in _MEMO:
        return _MEMO["gpu"]
    out = {}
    out["candidates 0 2 3 4"] = align_case([pairs_of(n, 50 + n, wrong=0.0) for n in (0, 2, 3, 4)], num_loops=16)
    out["candidates 511 512"] = align_case([pairs_of(n, 50 + n) for n in (511, 512)], num_loops=65)
    out["candidates 513 1025"] = align_case([pairs_of(n, 50 + n) for n in (1025, 513)], num_loops=100, min_inliers=12)
    out["src_cap 37"] = align_case([pairs_of(30, 61)], slack=7, num_loops=32)
    small = align_case([pairs_of(90, 62), pairs_of(60, 63)], slack=4, num_loops=64)
    for L in (1, 63, 64, 65, 100):
        out["num_loops %d" % L] = variant(small, num_loops=L)
    out["nsel 0"] = variant(small, ranges=np.zeros((0, 4), np.int32), seeds=np.zeros(0, np.uint32))
    cnt = np.full(16, 12345, np.int32)
    cnt[[0, 8]] = 50, -3
    out["count negative, stride 8"] = variant(small, count=cnt, count_stride=8)
    three = align_case([pairs_of(80, 64)] * 3 + [pairs_of(80, 65)], slack=4, num_loops=48)
    out["count below at beyond"] = variant(three, count=np.array([40, 84, 90, INT_MAX], np.int32), count_stride=1)
    # status 0, 1, 2 and 0 in one call, each with its own dst_first: a planted entry, two candidates, a cloud that fits
    # nothing, another planted entry
    rng = np.random.default_rng(66)
    cloud = (rng.uniform(-4, 4, (50, 3)).astype(f32), rng.uniform(-4, 4, (50, 3)).astype(f32))
    out["four entries"] = align_case([pairs_of(70, 67), pairs_of(2, 68, wrong=0.0), cloud, pairs_of(45, 69)],
                                     num_loops=48, min_inliers=8)
    base = align_case([pairs_of(90, 62)], num_loops=64, refit_loops=0)
    c = expected_entry(base, 0)["inliers"]
    for d in (-1, 0, 1):
        out["min_inliers count %+d" % d] = variant(base, min_inliers=c + d)
    out["thresh inf"] = variant(small, thresh=np.inf, num_loops=16)
    out["seed a"] = variant(small, seeds=np.array([1, 2], np.uint32))
    out["seed b"] = variant(small, seeds=np.array([3, 0], np.uint32))
    out["hostile"] = hostile_case(num_loops=48)
    out["collinear, identical"] = align_case([line_pairs(40, 70), same_pairs(20), skew_line_pairs(40, 76)], num_loops=40)
    noisy = align_case([pairs_of(400, 71, noise=0.01)], num_loops=64)
    for r in (0, 1, 5):
        out["refit_loops %d" % r] = variant(noisy, refit_loops=r)
    out["turned away"] = align_case([turned_away_pairs()], num_loops=32, thresh=0.2, refit_loops=3)
    out["slots wrap"] = align_case([pairs_of(700, 72, wrong=0.1)], num_loops=32, refit_loops=2)
    out["no inlier, no status"] = variant(small, src_status=None, dst_status=None, want_inlier=False)
    assert sorted(out) == sorted(GPU_CASES), sorted(set(out) ^ set(GPU_CASES))
    _MEMO["gpu"] = out
    return out


# ---- cases of the correspondence

def export_scene(max_records, tracks, seed, slack_tracks=3, slack_obs=5):
    """An exported scene fabricated directly: `tracks` is a list of lists of global record indices; the slots of a track
    hold its records in ascending order.  dict(max_records, record_obs, max_tracks, max_obs, track_offsets,
    export_summary); what lies behind T and O is stale."""
    T, O = len(tracks), sum(len(t) for t in tracks)
    mt, mo = T + slack_tracks, O + slack_obs
    off = np.full(mt + 1, 7777, np.int32)
    off[0] = 0
    off[1:T + 1] = np.cumsum([len(t) for t in tracks])
    rec = np.full(max_records, -1, np.int32)
    o = 0
    for t in tracks:
        for g in sorted(t):
            rec[g] = o
            o += 1
    summary = np.array([0, 0, T, O, 0, 0, 0, 0], np.int32)
    return dict(max_records=max_records, record_obs=rec, max_tracks=max(mt, 1), max_obs=max(mo, 1), track_offsets=off,
                export_summary=summary)


def correspond_case(TA, seed, shift=0, per=3):
    """Scene A of TA tracks of `per` records each over one record batch; scene B takes every second record of A's tracks
    into tracks of its own order (so a track of A maps to exactly one of B) and adds tracks of records A does not hold."""
    rng = np.random.default_rng(seed)
    nrec = per * TA + 40
    perm = rng.permutation(nrec)
    ta = [perm[per * t:per * t + per].tolist() for t in range(TA)]
    extra = perm[per * TA:].tolist()
    order = rng.permutation(TA)
    tb = [ta[t][::2] + [extra[k]] if k < len(extra) else ta[t][::2] for k, t in enumerate(order.tolist()) if t % 5]
    A = export_scene(nrec, ta, seed)
    nb = nrec + abs(shift) + 3
    B = export_scene(nb, [[g - shift for g in t if 0 <= g - shift < nb] for t in tb], seed + 1)
    return dict(a=A, b=B, shift=shift)


CORRESPOND_CASES = ("T_A 0", "T_A 1", "T_A 255", "T_A 256", "T_A 257", "shift +5", "shift -9", "shift out of range",
                    "conflict", "stale and hostile")


def correspond_cases():
    if "correspond" in _MEMO:
        return _MEMO["correspond"]
    out = {}
    for T in (0, 1, 255, 256, 257):
        out["T_A %d" % T] = correspond_case(T, 80 + T)
    out["shift +5"] = correspond_case(40, 90, shift=5)
    out["shift -9"] = correspond_case(40, 91, shift=-9)
    far = correspond_case(40, 92)
    far["shift"] = 100                                           # B's records were numbered without it: most fall outside
    out["shift out of range"] = far
    # a track of A whose records B spreads over two tracks
    A = export_scene(30, [[0, 1, 2, 3], [4, 5, 6], [7, 8]], 93)
    B = export_scene(30, [[0, 1, 20], [2, 3, 21], [4, 5, 6, 22]], 94)
    out["conflict"] = dict(a=A, b=B, shift=0)
    h = correspond_case(60, 95)
    A, B = dict(h["a"]), dict(h["b"])
    ra, rb, oa, ob = A["record_obs"].copy(), B["record_obs"].copy(), A["track_offsets"].copy(), B["track_offsets"].copy()
    ra[[0, 1, 2, 3]] = [INT_MIN, INT_MAX, int(A["export_summary"][3]), -2]
    rb[[5, 6, 7]] = [INT_MAX, -7, int(B["export_summary"][3]) + 2]
    oa[[7, 8, 20]] = [-3, INT_MAX, 1]                            # negative, beyond O, decreasing
    ob[[4, 30]] = [INT_MIN, 10 ** 9]
    A.update(record_obs=ra, track_offsets=oa)
    B.update(record_obs=rb, track_offsets=ob)
    B["export_summary"] = B["export_summary"].copy()
    B["export_summary"][2] = INT_MAX                             # T_B clamps to its capacity: stale offsets are searched
    out["stale and hostile"] = dict(a=A, b=B, shift=0)
    assert sorted(out) == sorted(CORRESPOND_CASES)
    _MEMO["correspond"] = out
    return out


# ---- cases of the transform

def transform_case(seed=7, ntracks=70, nimages=9, sim_status=0, slack=5):
    rng = np.random.default_rng(seed)
    sim = np.zeros(16, f32)
    sim[:9], sim[9:12], sim[12], sim[13] = rotation(rng).reshape(9), rng.uniform(-3, 3, 3), 1.7, 0.01
    mt = ntracks + slack
    pts = rng.uniform(-5, 5, (mt, 4)).astype(f32)
    pts[:, 3] = (np.arange(mt, dtype=np.uint32) + np.uint32(0x7fc00100)).view(f32)     # NaN payloads: copied bit for bit
    st = np.zeros(mt, np.int32)
    st[[3, 11, 12]] = [1, 4, -1]                                 # failed points are copied
    pts[20, 0], pts[21, 2] = np.nan, np.inf
    cam = np.concatenate([np.concatenate([rotation(rng).reshape(9), rng.uniform(-2, 2, 3)]) for _ in range(nimages)])
    cam = cam.astype(f32).reshape(nimages, 12)
    pair = np.arange(nimages, dtype=np.int32)
    pair[0], pair[2], pair[5], pair[6] = -1, UNSET, -3, UNSET    # the root, unset, resected
    cam[2] = 0
    cam[6, 4] = np.uint32(0xffc12345).view(f32)                  # an unset camera's NaN is copied bit for bit
    cam[7, 1], cam[8, 10] = np.nan, np.inf                       # a set camera's NaN becomes the one quiet NaN
    return dict(sim=sim, sim_status=sim_status, max_tracks=mt, export_summary=np.array([0, 0, ntracks, 0, 0, 0, 0, 0],
                                                                                       np.int32),
                points=pts, point_status=st, nimages=nimages, cam=cam, cam_pair=pair)

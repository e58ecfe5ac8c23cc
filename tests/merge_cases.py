"""misift_merge_scenes_batch: expected_merge, the numpy restatement of the definition in include/misift.h rule by rule,
the wrapper of the library's host hook, and the cases of its tests (test_merge_cpu.py pins the restatement to the hook and
asserts what each case is built to hit, test_gpu_merge.py holds the device to it byte for byte).  A scene is a dict of
the MERGE_SCENE_KEYS of cudasift_amd.capi as numpy arrays; a case is two scenes a and b, the map, accept (or None), the
shifts and output capacities, and which optional outputs are wanted.  No GPU in here, and cudasift_amd.capi is imported
inside functions only."""
import numpy as np

from batch_util import POISON_WORD

f32 = np.float32
OBS_DTYPE = np.dtype([("frame", "<i4"), ("record", "<i4"), ("xpos", "<f4"), ("ypos", "<f4")])
NOT_VALID, CONFLICT, REJECTED, BAD_MAP, NOT_LIVE, CUT = -1, -2, -3, -4, -5, -6
UNSET, ROOT, CAM_MERGED = -2, -1, -4
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
OUTPUTS = ("track_offsets_out", "obs_out", "export_summary_out", "points_out", "point_views_out", "point_status_out",
           "cam_out", "cam_pair_out", "track_map_a", "obs_map_a", "obs_map_b", "record_obs_out", "summary")
OPTIONAL = ("obs_map_a", "obs_map_b", "record_obs_out")
SCENE_ARRAYS = (("track_offsets", np.int32), ("obs", OBS_DTYPE), ("export_summary", np.int32), ("points", f32),
                ("point_views", np.int32), ("point_status", np.int32), ("cam", f32), ("cam_pair", np.int32),
                ("record_obs", np.int32))


# ---- the definition restated

def clamp(v, hi):
    return min(max(int(v), 0), hi)


def counts(S):
    return clamp(S["export_summary"][2], S["max_tracks"]), clamp(S["export_summary"][3], S["max_obs"])


def owners(S):
    """(valid (T,), owner (O,)): the owner of a slot is the largest valid track that holds it, -1 for none."""
    T, O = counts(S)
    off = [int(v) for v in S["track_offsets"][:T + 1]] if T else []
    valid, owner = np.zeros(T, bool), np.full(O, -1, np.int64)
    for t in range(T):
        if 0 <= off[t] <= off[t + 1] <= O:
            valid[t] = True
            owner[off[t]:off[t + 1]] = t
    return valid, owner


def live_elements(S, fshift, source, owner, t):
    """Rule 1: the live observations track t owns, as (key, source, slot)."""
    off, end = int(S["track_offsets"][t]), int(S["track_offsets"][t + 1])
    out = []
    for o in range(off, end):
        f = int(S["obs"]["frame"][o])
        if owner[o] == t and 0 <= f < S["nimages"]:
            out.append((((f + fshift) << 32) | (int(S["obs"]["record"][o]) & 0xffffffff), source, o))
    return out


def classes(case, valid_a, TB):
    """Rule 2 per A-track: the negative class, or ('partner', tB), or 'alone'."""
    out = []
    for t, ok in enumerate(valid_a):
        m = int(case["map"][t])
        if not ok:
            out.append(NOT_VALID)
        elif m == -2:
            out.append(CONFLICT)
        elif m < -2 or m >= TB:
            out.append(BAD_MAP)
        elif m >= 0 and case["accept"] is not None and int(case["accept"][t]) == 0:
            out.append(REJECTED)
        else:
            out.append(("partner", m) if m >= 0 else "alone")
    return out


def decide(case):
    """Rules 1 to 4: dict(cls, merged: per merged track t' < N a dict(src ('b' or 'a'), t, union (the elements), kept
    (sorted by key), len, off, written), TA, OA, TB, OB, owner_a, owner_b, T', O')."""
    A, B = case["a"], case["b"]
    (TA, OA), (TB, OB) = counts(A), counts(B)
    valid_a, owner_a = owners(A)
    valid_b, owner_b = owners(B)
    cls = classes(case, valid_a, TB)
    merged = [dict(src="b", t=t, union=live_elements(B, case["fshift_b"], 0, owner_b, t) if valid_b[t] else [])
              for t in range(TB)]
    for t, c in enumerate(cls):
        if isinstance(c, tuple):
            merged[c[1]]["union"] += live_elements(A, case["fshift_a"], 1, owner_a, t)
        elif c == "alone":
            merged.append(dict(src="a", t=t, union=live_elements(A, case["fshift_a"], 1, owner_a, t)))
    off = 0
    for tn, m in enumerate(merged):
        first = {}
        for e in m["union"]:                                     # kept: the smallest (source, slot) of its key
            if e[0] not in first or e[1:] < first[e[0]][1:]:
                first[e[0]] = e
        m["kept"] = sorted(first.values())
        m["len"], m["off"] = len(m["kept"]), off
        m["written"] = tn < case["max_tracks_out"] and off + m["len"] <= case["max_obs_out"]
        off += m["len"]
    Tn = sum(m["written"] for m in merged)
    assert all(m["written"] for m in merged[:Tn])                # a prefix
    On = merged[Tn - 1]["off"] + merged[Tn - 1]["len"] if Tn else 0
    return dict(cls=cls, merged=merged, TA=TA, OA=OA, TB=TB, OB=OB, owner_a=owner_a, owner_b=owner_b, Tn=Tn, On=On)


def sizes(case):
    A, B = case["a"], case["b"]
    mt, mo, n = case["max_tracks_out"], case["max_obs_out"], case["nimages_out"]
    return dict(track_offsets_out=mt + 1, obs_out=4 * mo, export_summary_out=8, points_out=4 * mt, point_views_out=mt,
                point_status_out=mt, cam_out=12 * n, cam_pair_out=n, track_map_a=A["max_tracks"], obs_map_a=A["max_obs"],
                obs_map_b=B["max_obs"], record_obs_out=max(case["max_records_out"], 1), summary=8)


def u32(a, dt=np.int32):
    return np.ascontiguousarray(a, dt).reshape(-1).view(np.uint32)


def expected_merge(case):
    """The thirteen outputs as uint32 arrays of exactly the stated sizes (poison where the call writes nothing; an
    optional output that is not wanted stays all poison), and the decisions under 'res'."""
    res = decide(case)
    A, B = case["a"], case["b"]
    TA, OA, TB, OB, Tn, On = (res[k] for k in ("TA", "OA", "TB", "OB", "Tn", "On"))
    out = {k: np.full(m, POISON_WORD, np.uint32) for k, m in sizes(case).items()}
    obs_out = out["obs_out"].reshape(-1, 4)
    words = {0: np.ascontiguousarray(B["obs"]).view(np.uint32).reshape(-1, 4),
             1: np.ascontiguousarray(A["obs"]).view(np.uint32).reshape(-1, 4)}
    fshift = {0: case["fshift_b"], 1: case["fshift_a"]}
    track_map = np.zeros(TA, np.int64)
    maps = {0: np.full(OB, NOT_VALID, np.int64), 1: np.full(OA, NOT_VALID, np.int64)}
    out["track_offsets_out"][0] = 0
    summary = np.zeros(8, np.int64)
    longest = 0
    number_of_b = {}
    for tn, m in enumerate(res["merged"]):
        S, key = (B, "b") if m["src"] == "b" else (A, "a")
        if m["src"] == "a":
            track_map[m["t"]] = tn if m["written"] else CUT
            summary[3] += m["written"]
        else:
            number_of_b[m["t"]] = tn if m["written"] else CUT
        place = {e[0]: m["off"] + k for k, e in enumerate(m["kept"])}
        for e in m["union"]:
            maps[e[1]][e[2]] = place[e[0]] if m["written"] else CUT
        if not m["written"]:
            continue
        out["track_offsets_out"][tn + 1] = m["off"] + m["len"]
        for k, (_, source, o) in enumerate(m["kept"]):
            w = words[source][o].copy()
            w[0] = np.int32(int(w.view(np.int32)[0]) + fshift[source]).view(np.uint32)
            obs_out[m["off"] + k] = w
        out["points_out"][4 * tn:4 * tn + 4] = u32(S["points"], f32).reshape(-1, 4)[m["t"]]
        out["point_views_out"][tn] = u32(S["point_views"])[m["t"]]
        out["point_status_out"][tn] = u32(S["point_status"])[m["t"]]
        longest = max(longest, m["len"])
        summary[5] += len(m["union"]) - m["len"]
    for t, c in enumerate(res["cls"]):
        if isinstance(c, tuple):
            track_map[t] = number_of_b[c[1]]
            summary[2] += track_map[t] >= 0
        elif c != "alone":
            track_map[t] = c
            summary[4] += 1
    # the slots that are in no union: not live, or their owner was dropped
    for source, S, owner, O in ((1, A, res["owner_a"], OA), (0, B, res["owner_b"], OB)):
        for o in range(O):
            t = owner[o]
            if t < 0:
                continue
            c = res["cls"][t] if source else "b"
            if isinstance(c, int):
                maps[source][o] = c
                continue
            tn = number_of_b[c[1]] if isinstance(c, tuple) else track_map[t] if source else number_of_b[t]
            if tn == CUT:
                maps[source][o] = CUT
            elif not 0 <= int(S["obs"]["frame"][o]) < S["nimages"]:
                maps[source][o] = NOT_LIVE
    out["track_map_a"][:TA] = u32(track_map)
    if case["want"]["obs_map_a"]:
        out["obs_map_a"][:OA] = u32(maps[1])
    if case["want"]["obs_map_b"]:
        out["obs_map_b"][:OB] = u32(maps[0])
    if case["want"]["record_obs_out"]:
        rec = np.full(case["max_records_out"], -1, np.int64)
        for g in range(case["max_records_out"]):
            for source, S, O, rshift in ((0, B, OB, case["rshift_b"]), (1, A, OA, case["rshift_a"])):
                gs = g - rshift
                if 0 <= gs < S["max_records"]:
                    o = int(S["record_obs"][gs])
                    if 0 <= o < O and maps[source][o] >= 0:
                        rec[g] = maps[source][o]
                        break
        out["record_obs_out"][:] = u32(rec)
    cam_out, pair_out = out["cam_out"].reshape(-1, 12), out["cam_pair_out"]
    for i in range(case["nimages_out"]):
        ib, ia = i - case["fshift_b"], i - case["fshift_a"]
        if 0 <= ib < B["nimages"] and B["cam_pair"][ib] != UNSET:
            cam_out[i], pair_out[i] = u32(B["cam"], f32).reshape(-1, 12)[ib], u32(B["cam_pair"])[ib]
        elif 0 <= ia < A["nimages"] and A["cam_pair"][ia] != UNSET:
            cam_out[i], pair_out[i] = u32(A["cam"], f32).reshape(-1, 12)[ia], u32([CAM_MERGED])[0]
            summary[7] += 1
        else:
            cam_out[i], pair_out[i] = 0, u32([UNSET])[0]
    N = len(res["merged"])
    total = sum(m["len"] for m in res["merged"])
    out["export_summary_out"][:] = u32([N, total, Tn, On, longest, 0, 0, 0])
    summary[[0, 1, 6]] = Tn, On, N - Tn
    out["summary"][:] = u32(summary)
    return dict(out, res=res)


def compare(got, e, what, keys=OUTPUTS):
    for k in keys:
        bad = np.nonzero(got[k] != e[k])[0]
        assert len(bad) == 0, (what, k, "%d words differ, first %s" % (len(bad), bad[:8]), got[k][bad[:4]].view(np.int32),
                               e[k][bad[:4]].view(np.int32))


def merged_sets(out):
    """The written tracks of a merged export (uint32 outputs) as a set of frozensets of (frame, record)."""
    T = int(out["export_summary_out"].view(np.int32)[2])
    off = out["track_offsets_out"].view(np.int32)
    obs = out["obs_out"].view(np.int32).reshape(-1, 4)
    return {frozenset((int(f), int(r)) for f, r in obs[off[t]:off[t + 1], :2]) for t in range(T)}


def merged_scene(case, out, cam_pair_as_is=True):
    """The scene a later call sees: the merge's outputs (uint32 arrays) as a scene dict."""
    mt, mo, n = case["max_tracks_out"], case["max_obs_out"], case["nimages_out"]
    return dict(max_tracks=mt, max_obs=mo, track_offsets=out["track_offsets_out"].view(np.int32).copy(),
                obs=out["obs_out"].view(OBS_DTYPE).copy(), export_summary=out["export_summary_out"].view(np.int32).copy(),
                points=out["points_out"].view(f32).reshape(mt, 4).copy(),
                point_views=out["point_views_out"].view(np.int32).copy(),
                point_status=out["point_status_out"].view(np.int32).copy(), nimages=n,
                cam=out["cam_out"].view(f32).reshape(n, 12).copy(), cam_pair=out["cam_pair_out"].view(np.int32).copy(),
                max_records=case["max_records_out"],
                record_obs=out["record_obs_out"].view(np.int32).copy() if case["want"]["record_obs_out"] else None)


# ---- the hook

def capacity():
    from cudasift_amd import capi
    return capi.merge_capacity()


def scene_inputs(S):
    """The arrays of a scene at exactly the sizes the call states (record_obs: None when the scene has none)."""
    mt, mo, n = S["max_tracks"], S["max_obs"], S["nimages"]
    ins = dict(track_offsets=np.ascontiguousarray(S["track_offsets"][:mt + 1], np.int32),
               obs=np.ascontiguousarray(S["obs"][:mo]), export_summary=np.ascontiguousarray(S["export_summary"], np.int32),
               points=np.ascontiguousarray(S["points"], f32).reshape(-1, 4),
               point_views=np.ascontiguousarray(S["point_views"], np.int32),
               point_status=np.ascontiguousarray(S["point_status"], np.int32),
               cam=np.ascontiguousarray(S["cam"], f32).reshape(-1, 12), cam_pair=np.ascontiguousarray(S["cam_pair"], np.int32),
               record_obs=None if S.get("record_obs") is None else np.ascontiguousarray(S["record_obs"], np.int32))
    assert len(ins["track_offsets"]) == mt + 1 and len(ins["obs"]) == mo and len(ins["cam"]) == n == len(ins["cam_pair"])
    assert len(ins["points"]) == mt == len(ins["point_status"]) == len(ins["point_views"])
    assert ins["record_obs"] is None or len(ins["record_obs"]) == S["max_records"]
    return ins


def inputs(case):
    return dict(a=scene_inputs(case["a"]), b=scene_inputs(case["b"]), map=np.ascontiguousarray(case["map"], np.int32),
                accept=None if case["accept"] is None else np.ascontiguousarray(case["accept"], np.int32))


def scene_args(S, ins, ptr):
    """One scene's thirteen arguments of the C call; ptr turns an array (or None) into a pointer."""
    return [S["max_tracks"], S["max_obs"], ptr(ins["track_offsets"]), ptr(ins["obs"]), ptr(ins["export_summary"]),
            ptr(ins["points"]), ptr(ins["point_views"]), ptr(ins["point_status"]), S["nimages"], ptr(ins["cam"]),
            ptr(ins["cam_pair"]), int(S.get("max_records") or 0), ptr(ins["record_obs"])]


def scalar_args(case):
    return [case[k] for k in ("fshift_a", "fshift_b", "nimages_out", "rshift_a", "rshift_b", "max_records_out",
                              "max_tracks_out", "max_obs_out")]


def hook_merge(case):
    """misift_test_merge_scenes on poisoned outputs of exactly the stated sizes, as uint32 arrays; the inputs must come
    back as they went in."""
    from cudasift_amd import capi
    ins = inputs(case)
    before = {(s, k): ins[s][k].tobytes() for s in "ab" for k in ins[s] if ins[s][k] is not None}
    out = {k: np.full(m, POISON_WORD, np.uint32) for k, m in sizes(case).items()}

    def ptr(a):
        return None if a is None else a.ctypes.data

    outs = [None if k in OPTIONAL and not case["want"][k] else out[k].ctypes.data for k in OUTPUTS]
    rc = capi.lib().misift_test_merge_scenes(*scene_args(case["a"], ins["a"], ptr), *scene_args(case["b"], ins["b"], ptr),
                                             ptr(ins["map"]), ptr(ins["accept"]), *scalar_args(case), *outs)
    assert rc == 0, (rc, capi.lib().misift_last_error())
    for (s, k), v in before.items():
        assert ins[s][k].tobytes() == v, (s, k, "was written")
    return out


# ---- cases

R = 1000                                                        # records per frame of the fabricated record batches


def scene_from_tracks(tracks, nimages, seed, slack=(3, 5), shuffle=False, records=True, cam_pair=None, per_frame=R):
    """A scene fabricated directly: `tracks` is a list of lists of (frame, record); the slots of a track hold them in
    ascending order, or shuffled.  Positions, points, view counts, statuses and cameras are patterns that must come
    through bit for bit (NaN payloads among them); what lies behind T and O is stale."""
    rng = np.random.default_rng(seed)
    T, O = len(tracks), sum(len(t) for t in tracks)
    mt, mo = max(T + slack[0], 1), max(O + slack[1], 1)
    off = np.full(mt + 1, 7777, np.int32)
    off[0] = 0
    off[1:T + 1] = np.cumsum([len(t) for t in tracks], dtype=np.int64)
    obs = np.zeros(mo, OBS_DTYPE)
    obs["frame"], obs["record"] = rng.integers(0, max(nimages, 1), mo), rng.integers(0, per_frame, mo)  # stale beyond O
    o = 0
    for t in tracks:
        lst = sorted(t)
        if shuffle:
            lst = [lst[i] for i in rng.permutation(len(lst))]
        for f, r in lst:
            obs["frame"][o], obs["record"][o] = f, r
            o += 1
    obs["xpos"], obs["ypos"] = rng.uniform(0, 1920, mo).astype(f32), rng.uniform(0, 1080, mo).astype(f32)
    obs["xpos"][::17] = (np.arange(len(obs["xpos"][::17]), dtype=np.uint32) + np.uint32(0x7fc00200)).view(f32)
    pts = rng.uniform(-5, 5, (mt, 4)).astype(f32)
    pts[:, 3] = (np.arange(mt, dtype=np.uint32) + np.uint32(0x7fc00100 + seed % 64 * 4096)).view(f32)
    views = rng.integers(0, 9, mt).astype(np.int32)
    status = (rng.random(mt) < 0.2).astype(np.int32) * rng.integers(1, 5, mt).astype(np.int32)
    cam = rng.uniform(-2, 2, (nimages, 12)).astype(f32)
    cam[:, 5] = (np.arange(nimages, dtype=np.uint32) + np.uint32(0xffc00300)).view(f32)
    pair = np.arange(nimages, dtype=np.int32) if cam_pair is None else np.asarray(cam_pair, np.int32)
    S = dict(max_tracks=mt, max_obs=mo, track_offsets=off, obs=obs, export_summary=np.array([T, O, T, O, 0, 0, 0, 0], np.int32),
             points=pts, point_views=views, point_status=status, nimages=nimages, cam=cam, cam_pair=pair, max_records=0,
             record_obs=None)
    if records:
        S["max_records"] = nimages * per_frame
        rec = np.full(S["max_records"], -1, np.int32)
        for o in range(O - 1, -1, -1):                           # of hostile duplicates the first slot stays
            f, r = int(obs["frame"][o]), int(obs["record"][o])
            if 0 <= f < nimages and 0 <= r < per_frame:
                rec[f * per_frame + r] = o
        S["record_obs"] = rec
    return S


def merge_case(a, b, point_map, accept=None, fshift_a=0, fshift_b=0, nimages_out=None, max_tracks_out=None,
               max_obs_out=None, want=(True, True, True), slack_images=1, per_frame=R):
    nout = max(a["nimages"] + fshift_a, b["nimages"] + fshift_b) + slack_images if nimages_out is None else nimages_out
    mp = np.full(a["max_tracks"], 123456, np.int32)              # stale beyond T_A
    mp[:len(point_map)] = point_map
    acc = None
    if accept is not None:
        acc = np.full(a["max_tracks"], 0, np.int32)
        acc[:len(accept)] = accept
    recs = a["record_obs"] is not None and b["record_obs"] is not None
    return dict(a=a, b=b, map=mp, accept=acc, fshift_a=fshift_a, fshift_b=fshift_b, nimages_out=nout,
                rshift_a=fshift_a * per_frame, rshift_b=fshift_b * per_frame,
                max_records_out=nout * per_frame if recs else 0,
                max_tracks_out=a["max_tracks"] + b["max_tracks"] if max_tracks_out is None else max_tracks_out,
                max_obs_out=a["max_obs"] + b["max_obs"] if max_obs_out is None else max_obs_out,
                want=dict(obs_map_a=want[0], obs_map_b=want[1], record_obs_out=want[2] and recs))


def variant(case, **kw):
    return dict(case, **kw)


def windows_case(TA, TB, seed, nimages=6, fshift_a=0, fshift_b=3, shuffle=False, **kw):
    """Two windows of `nimages` images over one world: min(TA, TB) // 2 world tracks are seen by both (their observations
    in the frames both windows hold are duplicates), the other tracks by one only.  The tracks of each scene are in an
    order of their own, so the map is no identity."""
    rng = np.random.default_rng(seed)
    shared = min(TA, TB) // 2
    lo, hi = max(fshift_a, fshift_b), min(fshift_a, fshift_b) + nimages     # the frames both hold: [lo, hi)
    next_record = np.zeros(max(fshift_a, fshift_b) + nimages, np.int64)

    def run(first, last):                                        # a track over the global frames first .. last
        out = []
        for f in range(first, last + 1):
            out.append((f, int(next_record[f])))
            next_record[f] += 1
        return out

    world = []
    for _ in range(shared):
        first = int(rng.integers(min(fshift_a, fshift_b), lo + 1)) if hi > lo else lo
        world.append(("ab", run(first, int(rng.integers(max(hi - 1, first), max(fshift_a, fshift_b) + nimages)))))
    for which, n, fs in (("a", TA - shared, fshift_a), ("b", TB - shared, fshift_b)):
        for _ in range(n):
            first = int(rng.integers(fs, fs + nimages - 1))
            world.append((which, run(first, int(rng.integers(first + 1, fs + nimages)))))
    scenes, index = {}, {}
    for which, fs in (("a", fshift_a), ("b", fshift_b)):
        mine = [k for k, (w, _) in enumerate(world) if which in w]
        mine = [mine[i] for i in rng.permutation(len(mine))]
        index[which] = {k: t for t, k in enumerate(mine)}
        tracks = [[(f - fs, r) for f, r in world[k][1] if fs <= f < fs + nimages] for k in mine]
        scenes[which] = scene_from_tracks(tracks, nimages, seed + (which == "b"), shuffle=shuffle)
    point_map = np.full(len(index["a"]), -1, np.int32)
    for k, t in index["a"].items():
        if k in index["b"]:
            point_map[t] = index["b"][k]
    return merge_case(scenes["a"], scenes["b"], point_map, fshift_a=fshift_a, fshift_b=fshift_b, **kw)


def union_sizes_case(sizes_, seed=3, dup=None, shuffle=False, **kw):
    """One B-track and one partner per entry U of `sizes_`: B holds U // 2 observations and A the other U - U // 2, in
    frames of their own (no duplicate), over 700 images and no shift.  dup = 'all': A's observations are B's first ones
    instead (every A observation a duplicate); dup = 'inside': every list holds its first observation twice more."""
    ta, tb = [], []
    for k, U in enumerate(sizes_):
        nb = U // 2
        b = [(350 + i, k) for i in range(nb)]
        a = [(i, k) for i in range(U - nb)] if dup != "all" else b[:max(nb // 2, 1)]
        if dup == "inside":
            a, b = a + a[:1] * 2, b + b[:1] * 2
        ta.append(a), tb.append(b)
    A = scene_from_tracks(ta, 700, seed, shuffle=shuffle)
    B = scene_from_tracks(tb, 700, seed + 1, shuffle=shuffle)
    return merge_case(A, B, np.arange(len(sizes_)), **kw)


def union_sizes():
    cap = capacity()
    return [0, 1, 2, 63, 64, 65, 255, 256, 257, 602] + [u for u in (cap + 1, cap + 70) if u not in (257, 602)]


def partners_case(seed=5):
    """B-track 1 has 70 partners (A's tracks 3 .. 72, each holding some of its frames and some of their own); B-tracks 3
    and 4 are not valid (a hostile offset between them) and B-track 3 has two partners."""
    tb = [[(f, 10 + t) for f in range(2 + t % 3)] for t in range(6)]
    tb[1] = [(f, 11) for f in range(40)]
    ta = [[(f, 500 + t) for f in range(3)] for t in range(3)]
    ta += [[(k % 40, 11), ((k + 1) % 40, 11), (40 + k % 20, 600 + k)] for k in range(70)]
    ta += [[(0, 13), (5, 700)], [(1, 13), (6, 701)]]
    A, B = scene_from_tracks(ta, 60, seed), scene_from_tracks(tb, 60, seed + 1)
    off = B["track_offsets"].copy()
    off[4] = B["max_obs"] + 9                                    # tracks 3 and 4: their ranges are no ranges
    B = dict(B, track_offsets=off)
    return merge_case(A, B, [-1, -1, -1] + [1] * 70 + [3, 3])


def hostile_map_case(seed=7, accept=True):
    """Map values -1, -2, -3, INT_MIN, T_B and INT_MAX among good ones; accept 1, 0 and -1 mixed (or None); frames -1 and
    nimages in both scenes; a track of A that is not valid; hostile duplicates inside lists of both scenes."""
    case = windows_case(40, 30, seed, shuffle=True)
    A, B = dict(case["a"]), dict(case["b"])
    TB = counts(B)[0]
    mp = case["map"].copy()
    partners = np.nonzero(mp[:40] >= 0)[0]
    mp[partners[:2]] = [-2, -3]
    alone = np.nonzero(mp[:40] == -1)[0]
    mp[alone[:4]] = [INT_MIN, TB, INT_MAX, -2]
    for S in (A, B):
        obs = S["obs"].copy()
        off = S["track_offsets"]
        obs["frame"][off[5]] = -1
        obs["frame"][off[6]] = S["nimages"]
        obs["frame"][off[7]] = INT_MIN
        obs["frame"][off[8] + 1] = INT_MAX
        obs[off[9] + 1] = obs[off[9]]                            # a duplicate inside one list
        S["obs"] = obs
    off = A["track_offsets"].copy()
    off[12] = -4                                                 # tracks 11 and 12 of A are not valid
    A["track_offsets"] = off
    acc = None
    if accept:
        acc = np.ones(A["max_tracks"], np.int32)
        acc[partners[2:8]] = [0, -1, 0, 1, -1, 0]
        acc[alone[4:6]] = [0, -1]                                # no partner: not looked at
    return variant(case, a=A, b=B, map=mp, accept=acc)


def with_counts(case, which, T, O):
    S = dict(case[which])
    es = S["export_summary"].copy()
    es[2], es[3] = T, O
    S["export_summary"] = es
    return variant(case, **{which: S})


def cameras_case(seed=11):
    """Six images from B only, from A only, from both and from neither: A holds merged images 0 .. 5 and B 3 .. 8 of ten;
    A's root is image 1 (B has none there), B's root image 4 (A's camera there is set too); A is unset at 0 and 3, B at
    3 and 8, so image 3 has a camera in neither."""
    pa, pb = [UNSET, ROOT, 0, UNSET, -3, 2], [UNSET, ROOT, 1, 0, -3, UNSET]
    case = windows_case(9, 7, seed, nimages=6, fshift_a=0, fshift_b=3)
    return variant(case, a=dict(case["a"], cam_pair=np.array(pa, np.int32)), b=dict(case["b"], cam_pair=np.array(pb, np.int32)))


def cut_cases(seed=13):
    """Capacity cuts: at max_tracks_out inside B's part and inside A's part, at max_obs_out in each."""
    base = windows_case(20, 16, seed)
    res = decide(base)
    TB, N = res["TB"], len(res["merged"])
    off = [m["off"] for m in res["merged"]] + [sum(m["len"] for m in res["merged"])]
    return {"cut tracks in B": variant(base, max_tracks_out=TB - 5), "cut tracks in A": variant(base, max_tracks_out=TB + 3),
            "cut tracks at T_B": variant(base, max_tracks_out=TB), "cut tracks at N": variant(base, max_tracks_out=N),
            "cut obs in B": variant(base, max_obs_out=off[TB - 4] + 1),
            "cut obs in A": variant(base, max_obs_out=off[TB + 2] + 1),
            "cut obs exact": variant(base, max_obs_out=off[TB + 2]),
            "cut obs one short": variant(base, max_obs_out=off[TB + 2] - 1), "cut obs 1": variant(base, max_obs_out=1)}


TRACK_COUNTS = ((0, 5), (5, 0), (0, 0), (1, 1), (63, 65), (64, 64), (65, 63), (257, 257), (2047, 2049), (2048, 2048),
                (2049, 2047))
DEVICE_COUNTS = ((10, 40), (20, 10 ** 9), (INT_MAX, INT_MAX), (-1, 50), (20, -5), (INT_MIN, INT_MIN), (0, 0))
_MEMO = {}


def gpu_cases():
    """name -> case: everything test_gpu_merge.py compares byte for byte; test_merge_cpu.py holds the hook to each and
    asserts what it is built to hit."""
    if "gpu" in _MEMO:
        return _MEMO["gpu"]
    out = {}
    for TA, TB in TRACK_COUNTS:
        out["T %d %d" % (TA, TB)] = windows_case(TA, TB, 100 + TA + TB)
    out["unions"] = union_sizes_case(union_sizes())
    out["unions, unsorted"] = union_sizes_case(union_sizes(), shuffle=True, seed=4)
    out["unions, every A a duplicate"] = union_sizes_case(union_sizes(), dup="all")
    out["unions, duplicates inside"] = union_sizes_case(union_sizes(), dup="inside", shuffle=True)
    out["partners"] = partners_case()
    out["hostile"] = hostile_map_case()
    out["hostile, no accept"] = hostile_map_case(accept=False)
    out["unsorted"] = windows_case(50, 50, 21, shuffle=True)
    out["no shift"] = windows_case(30, 30, 22, fshift_a=0, fshift_b=0)
    out["shift a"] = windows_case(30, 30, 23, fshift_a=4, fshift_b=0)
    base = windows_case(20, 30, 24)
    assert (base["a"]["max_tracks"], base["a"]["max_obs"]) == (23, counts(base["a"])[1] + 5)
    for T, O in DEVICE_COUNTS:
        out["counts a %d %d" % (T, O)] = with_counts(base, "a", T, O)
        out["counts b %d %d" % (T, O)] = with_counts(base, "b", T, O)
    out.update(cut_cases())
    out["cameras"] = cameras_case()
    for k, name in enumerate(OPTIONAL):
        want = [True, True, True]
        want[k] = False
        out["no " + name] = windows_case(12, 12, 30 + k, want=tuple(want))
    norec = windows_case(12, 12, 33)
    out["no record_obs inputs"] = merge_case(dict(norec["a"], record_obs=None, max_records=0),
                                             dict(norec["b"], record_obs=None, max_records=0), norec["map"][:12],
                                             fshift_b=3)
    _MEMO["gpu"] = out
    return out


def empty_a_case(seed=40):
    """T_A = 0 merged into B with room for all of B and no shift: B comes back."""
    case = windows_case(0, 25, seed, fshift_a=0, fshift_b=0, slack_images=0)
    return case

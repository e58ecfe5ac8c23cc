"""misift_merge_scenes_batch without a GPU: the numpy restatement merge_cases.expected_merge (what test_gpu_merge.py holds
the device to, byte for byte) pinned to the library's host hook, which runs the rules its kernels compile, on every case
of the device tests; what each case is built to hit; the argument errors; that merging an empty scene returns the other;
and, on a planted 8-camera scene linked and exported over two overlapping pair sets, that the merged tracks are the
tracks of the export over both sets."""
import numpy as np
import pytest

import align_cases as AC
import merge_cases as MC
import posegraph_cases as G
from batch_util import POISON_WORD
from test_tracks_cpu import GATES, expected_tracks
from test_tracks_export_cpu import expected_export

MISIFT_OK, MISIFT_EINVAL = 0, -1
CASE_NAMES = tuple(MC.gpu_cases())


def test_library_exports_the_call():
    """Fails without the feature: the symbols, their rows in capi.SIGNATURES, the binding and the constant."""
    from cudasift_amd import capi
    L = capi.lib()
    for name in ("misift_merge_scenes_batch", "misift_test_merge_scenes", "misift_test_merge_capacity"):
        assert name in capi.SIGNATURES and hasattr(L, name), name
    assert len(capi.SIGNATURES["misift_merge_scenes_batch"][1]) == 50
    assert len(capi.SIGNATURES["misift_test_merge_scenes"][1]) == 49
    assert hasattr(capi.Context, "merge_scenes_batch") and capi.Context.merge_scenes is capi.Context.merge_scenes_batch
    assert capi.CAM_MERGED == MC.CAM_MERGED == -4
    assert capi.MERGE_OUTPUTS == MC.OUTPUTS
    assert MC.capacity() >= 64


@pytest.mark.parametrize("name", CASE_NAMES)
def test_hook_matches_the_restatement(name):
    case = MC.gpu_cases()[name]
    MC.compare(MC.hook_merge(case), MC.expected_merge(case), name)


def test_case_premises():
    """Each case hits what it is built for."""
    cases = MC.gpu_cases()
    cap = MC.capacity()
    res = {k: MC.expected_merge(c) for k, c in cases.items()}

    def summary(name):
        return res[name]["summary"].view(np.int32)

    for TA, TB in MC.TRACK_COUNTS:
        r = res["T %d %d" % (TA, TB)]["res"]
        assert (r["TA"], r["TB"]) == (TA, TB)
        s = summary("T %d %d" % (TA, TB))
        assert s[0] == TB + TA - min(TA, TB) // 2 and s[2] == min(TA, TB) // 2 and s[6] == 0
        assert (s[5] > 0) == (min(TA, TB) >= 2)                   # the shared frames hold duplicates
    lens = [len(m["union"]) for m in res["unions"]["res"]["merged"]]
    assert lens == MC.union_sizes() and max(lens) > cap and 602 in lens and cap + 1 in lens
    assert summary("unions")[5] == 0                             # none a duplicate
    r = res["unions, every A a duplicate"]["res"]
    assert all(m["len"] == len([e for e in m["union"] if e[1] == 0]) for m in r["merged"])
    assert summary("unions, every A a duplicate")[5] == sum(len([e for e in m["union"] if e[1] == 1]) for m in r["merged"])
    r = res["unions, duplicates inside"]["res"]
    assert any(len(m["union"]) > cap and len(m["union"]) - m["len"] == 4 for m in r["merged"])
    for name in ("unions, unsorted", "unsorted", "hostile"):
        S = cases[name]["a"]
        T = MC.counts(S)[0]
        off = S["track_offsets"]
        assert any((np.diff(S["obs"]["frame"][off[t]:off[t + 1]].astype(np.int64)) < 0).any() for t in range(T)), name
    r = res["partners"]["res"]
    assert sum(1 for c in r["cls"] if c == ("partner", 1)) == 70 and sum(1 for c in r["cls"] if c == ("partner", 3)) == 2
    valid_b, _ = MC.owners(cases["partners"]["b"])
    assert not valid_b[3] and not valid_b[4] and r["merged"][3]["len"] == 4 and r["merged"][4]["len"] == 0
    for name in ("hostile", "hostile, no accept"):
        c = res[name]["res"]["cls"]
        assert {x for x in c if isinstance(x, int)} == ({-1, -2, -3, -4} if name == "hostile" else {-1, -2, -4}), name
        mp = cases[name]["map"][:res[name]["res"]["TA"]]
        assert {-1, -2, -3, MC.INT_MIN, MC.INT_MAX, res[name]["res"]["TB"]} <= set(int(v) for v in mp)
        m = res[name]["obs_map_a"].view(np.int32)
        assert MC.NOT_LIVE in m and MC.NOT_LIVE in res[name]["obs_map_b"].view(np.int32) and MC.NOT_VALID in m
        assert summary(name)[5] > 0
    acc = cases["hostile"]["accept"]
    assert {0, 1, -1} <= set(int(v) for v in acc) and cases["hostile, no accept"]["accept"] is None
    for name, (fa, fb) in (("no shift", (0, 0)), ("shift a", (4, 0)), ("unsorted", (0, 3))):
        assert (cases[name]["fshift_a"], cases[name]["fshift_b"]) == (fa, fb) and summary(name)[2] > 0
    # the cuts: where they fall, and that the partners of a cut B-track go with it
    base = res["cut tracks at N"]
    TB, N = base["res"]["TB"], len(base["res"]["merged"])
    assert summary("cut tracks at N")[6] == 0 and summary("cut tracks at N")[0] == N
    for name, inside_b in (("cut tracks in B", True), ("cut tracks in A", False), ("cut obs in B", True),
                           ("cut obs in A", False), ("cut tracks at T_B", False), ("cut obs exact", False),
                           ("cut obs one short", False)):
        s, tm = summary(name), res[name]["track_map_a"].view(np.int32)[:base["res"]["TA"]]
        assert s[6] > 0 and (s[0] < TB) == inside_b and (MC.CUT in tm), name
        partners_cut = [t for t, c in enumerate(res[name]["res"]["cls"]) if isinstance(c, tuple) and c[1] >= s[0]]
        assert bool(partners_cut) == inside_b or name == "cut tracks at T_B", name
        assert all(tm[t] == MC.CUT for t in partners_cut), name
    assert summary("cut obs exact")[0] == summary("cut obs in A")[0] == summary("cut obs one short")[0] + 1
    assert summary("cut obs 1")[0] <= 1
    # the device-read counts
    for which in "ab":
        S = cases["counts %s 10 40" % which][which]
        assert MC.counts(cases["counts %s 20 1000000000" % which][which])[1] == S["max_obs"]
        assert MC.counts(cases["counts %s %d %d" % (which, MC.INT_MAX, MC.INT_MAX)][which]) == (S["max_tracks"], S["max_obs"])
        assert MC.counts(cases["counts %s -1 50" % which][which])[0] == 0
        assert MC.counts(cases["counts %s 20 -5" % which][which])[1] == 0
    pair = res["cameras"]["cam_pair_out"].view(np.int32)
    assert pair.tolist() == [-2, -4, -4, -2, -1, 1, 0, -3, -2, -2] and summary("cameras")[7] == 2
    assert (pair == -1).sum() == 1                               # A's root did not come through as a second root
    for name in MC.OPTIONAL:
        assert (res["no " + name][name] == POISON_WORD).all()
    assert not cases["no record_obs inputs"]["want"]["record_obs_out"]
    rec = res["T 64 64"]["record_obs_out"].view(np.int32)
    assert (rec >= 0).sum() == res["T 64 64"]["summary"].view(np.int32)[1]      # every kept observation has its record


def test_merging_an_empty_scene_returns_the_other():
    """Idempotence: T_A = 0 merged into B gives B's bytes."""
    case = MC.empty_a_case()
    B = case["b"]
    T, O = MC.counts(B)
    got = MC.hook_merge(case)
    MC.compare(got, MC.expected_merge(case), "empty A")
    assert got["summary"].view(np.int32).tolist() == [T, O, 0, 0, 0, 0, 0, 0]
    assert got["export_summary_out"].view(np.int32)[:4].tolist() == [T, O, T, O]
    ins = MC.scene_inputs(B)
    for k, name, n in (("track_offsets_out", "track_offsets", T + 1), ("obs_out", "obs", O), ("points_out", "points", T),
                       ("point_views_out", "point_views", T), ("point_status_out", "point_status", T),
                       ("cam_out", "cam", B["nimages"]), ("cam_pair_out", "cam_pair", B["nimages"])):
        want = ins[name][:n].tobytes()
        assert got[k].tobytes()[:len(want)] == want, k
    assert got["obs_map_b"].view(np.int32)[:O].tolist() == list(range(O))
    assert got["record_obs_out"].view(np.int32).tobytes() == ins["record_obs"].tobytes()


def test_argument_errors():
    """Every argument error of the header, through the hook (its checks are the call's own), and that nothing is written;
    the NULL context through the call itself."""
    from cudasift_amd import capi
    L = capi.lib()
    case = MC.gpu_cases()["T 5 0"]
    names, good, keep = bad_argument_table(case)

    def call(**kw):
        a = dict(good, **kw)
        return L.misift_test_merge_scenes(*[a[k] for k in names])

    assert call() == MISIFT_OK
    out0 = {k: v.copy() for k, v in keep["out"].items()}
    for kw in keep["bad"]:
        assert call(**kw) == MISIFT_EINVAL, kw
    for k, v in keep["out"].items():
        assert v.tobytes() == out0[k].tobytes(), k
    assert L.misift_merge_scenes_batch(None, *[good[k] for k in names]) == MISIFT_EINVAL


def bad_argument_table(case, ptr_of=None, alloc_out=None):
    """(the argument names in call order, a good call's arguments, dict(bad: the broken variants, out: the outputs)) for
    host arrays, or for device buffers when ptr_of (array -> device pointer) and alloc_out (words -> (buffer, pointer))
    are given."""
    ins = MC.inputs(case)
    hold = []

    def host_ptr(a):
        return None if a is None else a.ctypes.data

    ptr = ptr_of or host_ptr
    sizes = MC.sizes(case)
    out, optr = {}, {}
    for k, m in sizes.items():
        if alloc_out:
            out[k], optr[k] = alloc_out(m)
        else:
            out[k] = np.full(m, POISON_WORD, np.uint32)
            optr[k] = out[k].ctypes.data
    scene_keys = ("max_tracks", "max_obs", "track_offsets", "obs", "export_summary", "points", "point_views",
                  "point_status", "nimages", "cam", "cam_pair", "max_records", "record_obs")
    names = [k + "_" + s for s in "ab" for k in scene_keys] + ["map", "accept"] + \
        ["fshift_a", "fshift_b", "nimages_out", "rshift_a", "rshift_b", "max_records_out", "max_tracks_out",
         "max_obs_out"] + list(MC.OUTPUTS)
    good = {}
    for s in "ab":
        for k, v in zip(scene_keys, MC.scene_args(case[s], ins[s], ptr)):
            good[k + "_" + s] = v
    good["map"], good["accept"] = ptr(ins["map"]), ptr(np.ones(case["a"]["max_tracks"], np.int32))
    hold.append(ins)
    for k, v in zip(names[28:36], MC.scalar_args(case)):
        good[k] = v
    good.update(optr)
    A, B = case["a"], case["b"]
    bad = [{k: 0} for k in ("max_tracks_a", "max_obs_a", "nimages_a", "max_records_a", "max_tracks_b", "max_obs_b",
                            "nimages_b", "max_records_b", "nimages_out", "max_records_out", "max_tracks_out", "max_obs_out")]
    bad += [{k: -3} for k in ("max_tracks_a", "max_obs_b", "nimages_out", "max_tracks_out", "max_obs_out", "fshift_a",
                              "fshift_b", "rshift_a", "rshift_b")]
    bad += [dict(nimages_out=A["nimages"] + case["fshift_a"] - 1), dict(nimages_out=B["nimages"] + case["fshift_b"] - 1),
            dict(fshift_a=case["nimages_out"] - A["nimages"] + 1), dict(fshift_b=MC.INT_MAX),
            dict(max_records_out=A["max_records"] + case["rshift_a"] - 1),
            dict(max_records_out=B["max_records"] + case["rshift_b"] - 1), dict(rshift_a=MC.INT_MAX),
            dict(record_obs_a=None), dict(record_obs_b=None)]
    optional = ("accept", "obs_map_a", "obs_map_b", "record_obs_out", "record_obs_a", "record_obs_b")
    pointers = [k + "_" + s for s in "ab" for k in spans_keys()] + ["map", "accept"] + list(MC.OUTPUTS)
    bad += [{k: None} for k in pointers if k not in optional]
    for k in ("obs_a", "obs_b", "obs_out"):
        bad += [{k: good[k] + 4}, {k: good[k] + 8}]
    # every output on every input and on every other output: at its start, and ending on its first word
    spans = dict(track_offsets=lambda S: 4 * (S["max_tracks"] + 1), obs=lambda S: 16 * S["max_obs"],
                 export_summary=lambda S: 32, points=lambda S: 16 * S["max_tracks"], point_views=lambda S: 4 * S["max_tracks"],
                 point_status=lambda S: 4 * S["max_tracks"], cam=lambda S: 48 * S["nimages"],
                 cam_pair=lambda S: 4 * S["nimages"], record_obs=lambda S: 4 * S["max_records"])
    in_spans = {k + "_" + s: f(case[s]) for s in "ab" for k, f in spans.items()}
    in_spans["map"] = in_spans["accept"] = 4 * A["max_tracks"]
    for o in MC.OUTPUTS:
        align = 16 if o == "obs_out" else 4
        for k, nbytes in in_spans.items():
            bad += [{o: good[k]}, {o: good[k] + (nbytes - align) // align * align},
                    {o: good[k] - (4 * sizes[o] - align) // align * align}]
        for o2 in MC.OUTPUTS:
            if o2 != o:
                bad += [{o: good[o2]}, {o: good[o2] + (4 * sizes[o2] - align) // align * align}]
    return names, good, dict(bad=bad, out=out, hold=hold)


def spans_keys():
    return ("track_offsets", "obs", "export_summary", "points", "point_views", "point_status", "cam", "cam_pair",
            "record_obs")


# ---- the property on a planted scene

def planted_windows(outliers):
    """The 8-camera path of posegraph_cases with rows over its 13 pairs; P_A: the pairs inside images 0 .. 4, P_B: those
    inside images 3 .. 7; both hold pair (3, 4), and together they are all pairs.  Returns what link and export take."""
    S = G.SCENE
    rng = np.random.default_rng(77)
    cams = G.camera_path(S["ncams"], rng)
    n = 96
    X = rng.uniform([-4, -2.5, 5], [5, 2.5, 12], (n, 3))
    pairs, _, _ = G.window_pairs(S["ncams"])
    rows, _ = G.scene_rows(cams, X, rng, S["noise"], outliers, pairs)
    in_a = np.array([b <= 4 for a, b in pairs])
    in_b = np.array([a >= 3 for a, b in pairs])
    assert (in_a | in_b).all() and (in_a & in_b).sum() == 1
    return dict(pairs=np.array(pairs, np.int32), rows=np.concatenate(rows), n=n, nimg=S["ncams"], in_a=in_a, in_b=in_b)


def exported(W, member, seed):
    """Link and export (min_len 2, consistent only) over the pairs with `member`, as a scene dict."""
    n, nimg = W["n"], W["nimg"]
    total = nimg * n
    counts = np.full(nimg, n, np.int32)
    row_counts = np.where(member, n, 0).astype(np.int32)
    track, tlen, tframes, _ = expected_tracks(W["pairs"], W["rows"], row_counts, n, counts, None, n, total, GATES)
    xy = np.random.default_rng(5).integers(0, 2 ** 32, (total, 2), dtype=np.uint64).astype(np.uint32)   # one batch
    mt, mo = total // 2 + 1, total
    off, _, obs, rec, summ = expected_export(xy, counts, None, n, total, track, tlen, tframes, 2, 1, mt, mo, POISON_WORD)
    base = MC.scene_from_tracks([], nimg, seed, slack=(mt, mo), records=False)
    assert base["max_tracks"] == mt and base["max_obs"] == mo
    return dict(base, track_offsets=off, obs=obs.view(MC.OBS_DTYPE), export_summary=summ, max_records=total, record_obs=rec,
                labels=(track, tlen, tframes))


@pytest.mark.parametrize("outliers", [0.0, 0.03])
def test_merged_tracks_are_the_tracks_of_the_union(outliers):
    W = planted_windows(outliers)
    A, B, U = exported(W, W["in_a"], 1), exported(W, W["in_b"], 2), exported(W, W["in_a"] | W["in_b"], 3)
    ec = AC.expected_correspond(dict(a=A, b=B, shift=0))
    point_map = ec["map"].view(np.int32)
    TA, TB = MC.counts(A)[0], MC.counts(B)[0]
    assert TA > 20 and TB > 20 and (point_map[:TA] >= 0).sum() > 10
    assert (point_map[:TA] != -2).all()                          # a condition on the input: no track of A spans two of B
    case = MC.merge_case(A, B, point_map[:TA], slack_images=0)
    case["rshift_a"] = case["rshift_b"] = 0
    case["max_records_out"] = A["max_records"]
    e = MC.expected_merge(case)
    MC.compare(MC.hook_merge(case), e, "planted")
    s = e["summary"].view(np.int32)
    assert s[4] == 0 and s[6] == 0 and s[5] > 0
    merged = {t for t in MC.merged_sets(e) if len(t)}
    TU = MC.counts(U)[0]
    off, obs = U["track_offsets"], U["obs"]
    union = {frozenset((int(f), int(r)) for f, r in zip(obs["frame"][off[t]:off[t + 1]], obs["record"][off[t]:off[t + 1]]))
             for t in range(TU)}
    print("planted: T_A %d T_B %d merged %d union %d" % (TA, TB, len(merged), len(union)))
    # With no -2 in the map every consistent track of the union is a B-track with its partners or an A-track alone, so it
    # is a merged track.  The converse holds where the matches are clean; a wrong match can make a track of the union
    # inconsistent (two records of one frame) while its parts in A and B are consistent: those parts stay merged tracks.
    assert union <= merged
    track, tlen, tframes = U["labels"]
    for extra in merged - union:
        roots = {int(track[f * W["n"] + r]) for f, r in extra}
        assert len(roots) == 1 and tlen[min(roots)] != tframes[min(roots)], extra
    assert (len(merged - union) > 0) == (outliers > 0)
    # the merged record index names the slot of every record of the merged export
    rec = e["record_obs_out"].view(np.int32)
    o = e["obs_out"].view(np.int32).reshape(-1, 4)
    for g in np.nonzero(rec >= 0)[0][::7]:
        assert (o[rec[g], 0], o[rec[g], 1]) == (g // W["n"], g % W["n"])

"""The geometry-chain batch calls as a step table, for tests that run them on a context other calls have used
(test_gpu_used_context.py; the premises are asserted without a GPU in test_used_context_cpu.py).  No tests in here, and
cudasift_amd.capi is imported inside functions only.

A step is one call.  Its cases come from the builders its own GPU test file uses and its expected bytes from the same
restatement; what is new is only the form: every step gives, per size,
  case(size)            the host inputs, built once and left unchanged
  lists(case)           the caller-owned host lists handed to the call (contiguous, of the dtype the wrapper passes on)
  other_lists(case)     a second, valid set of the same shapes whose expected output differs
  uploads(case)         name -> array of every device input
  outputs(case)         name -> the poisoned content of every output at exactly its stated capacity
  enqueue(ctx, case, dev, lists)    library calls only: nothing read, nothing uploaded, no synchronisation
  expected(case, lists) name -> the bytes of every device buffer the call writes (outputs, and inputs refined in place)
  tmp_bytes(case, ncu)  the bytes of the context's shared temp the call asks for
and check() holds every device buffer to expected(), or to what was uploaded where the call must not write.
zeroed(case) is the case with every device input zero-filled: what a call that ran too early would have been given
(stream_util.py).  table() holds the 14 calls test_gpu_used_context.py sizes its plans from; stream_table() is table()
and, at `small` only and without tmp_bytes(), the further batch calls the caller-stream tests run.

Sizes.  `small` is the smallest case of the call's own tests that still runs every launch, off the multiples of 16;
`large` is a few times that in every dimension that sizes temp.  `huge` asks for more temp than any other step at
`small` or `large`, which means more than the pair matchers' partials: 12 MiB (fp32) and 16 MiB (int8) on 256 CUs,
whatever the pairs.  Ten calls size their temp by a capacity that costs no work (max_pts of the searches, the guided
matchers and the int8 pair matcher, max_records of the two track calls, max_obs of refine and resect, images without a
camera for triangulate): their `huge` is the `small` or `large` case under a larger capacity, milliseconds of GPU time
and the restatement unchanged.  The four others have no `huge`, and Step.no_huge says why, call by call.

Temp sizes.  include/misift.h states them in bytes for link_tracks, export_tracks, link_poses, triangulate, refine and
resect; for the matchers and the searches it names only what they are sized from, so tmp_bytes() restates the layouts
of the sources for those (the partials' item bound comes from the planners' host hooks).  The GPU tests hold
misift_test_ctx_state to these figures after every call, so a figure that drifts from the library fails there."""
import ctypes as C
import functools

import numpy as np

from batch_util import (OUT_FIELDS, POISON, POISON_WORD, expected_pair, fabricated_records, frames, gated_frame, layout,
                        matched_frames, orc, planted_members, quantize_np, span, xy_bits)

SIZES = ("small", "large", "huge")
GATES = (0.85, 0.95)
INF = float("inf")
CUS = 256                                                        # the CUs of an MI355X, where no device can be asked
f32 = np.float32


def align16(v):
    return (v + 15) // 16 * 16


def poisoned(words):
    return np.full(max(int(words), 1), POISON_WORD, np.uint32)


def i32(a):
    return np.ascontiguousarray(a, np.int32)


def u32(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


class Step:
    """One call of the table; the subclasses fill in the methods of the module's docstring."""
    name = None
    sizes = ("small", "large")
    no_huge = None                                               # for a step without `huge`: the reason
    temp = True                                                  # uses the shared temp
    carries_lists = True                                         # hands the library a host list
    takes_slot = True                                            # takes a slot of the pinned ring (with or without a list)

    def __init__(self):
        self._cases, self._expected = {}, {}

    def case(self, size):
        if size not in self._cases:
            assert size in self.sizes, (self.name, size)
            self._cases[size] = self.build(size)
        return self._cases[size]

    def lists(self, case):
        return {}

    def other_lists(self, case):
        return {}

    def zeroed(self, case):
        """The case with every device input zero-filled and the host lists as they are: what a call that ran before its
        inputs were staged would have been given.  expected(zeroed(case), lists) is what it would have written."""
        out = {k: v for k, v in case.items() if not k.startswith("memo")}
        for k, v in self.uploads(case).items():
            assert k in case, (self.name, k)
            out[k] = np.zeros_like(np.ascontiguousarray(v))
        return out

    def expected_for(self, size, lists=None):
        """expected() of the case of `size` under `lists` (default: its own), computed once per content of the lists."""
        case = self.case(size)
        lists = self.lists(case) if lists is None else lists
        key = (size,) + tuple((k, lists[k].tobytes()) for k in sorted(lists))
        if key not in self._expected:
            with np.errstate(all="ignore"):
                self._expected[key] = {k: np.ascontiguousarray(v) for k, v in self.expected(case, lists).items()}
        return self._expected[key]


class Bufs:
    """One instance of a step on a context: its case, the host content of every device buffer as uploaded, the buffers."""

    def __init__(self, ctx, step, size):
        self.ctx, self.step, self.size, self.case = ctx, step, size, step.case(size)
        self.host = {k: np.ascontiguousarray(v) for k, v in step.uploads(self.case).items()}
        for k, v in step.outputs(self.case).items():
            assert k not in self.host
            self.host[k] = v
        self.dev = {k: ctx.upload(v) for k, v in self.host.items()}
        self.lists = step.lists(self.case)
        self.at_call = None                                      # the content of the lists when the call was made

    def enqueue(self):
        self.at_call = {k: v.copy() for k, v in self.lists.items()}
        self.step.enqueue(self.ctx, self.case, self.dev, self.lists)

    def overwrite_lists(self):
        """The caller reuses its lists at once: other_lists(), written into the very arrays the call was given."""
        for k, v in self.step.other_lists(self.case).items():
            assert v.shape == self.lists[k].shape and v.dtype == self.lists[k].dtype, (self.step.name, k)
            self.lists[k][...] = v

    def check(self, what):
        """Byte equality of every device buffer: the restatement's bytes under the lists as they were at the call, and
        the uploaded bytes for everything the call must not write."""
        exp = self.step.expected_for(self.size, self.at_call)
        assert set(exp) <= set(self.host), (self.step.name, set(exp) - set(self.host))
        for k, up in self.host.items():
            want = exp.get(k, up)
            want = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
            assert want.nbytes == up.nbytes, (self.step.name, k, want.nbytes, up.nbytes)
            got = self.ctx.download(self.dev[k], (want.nbytes,), np.uint8)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, "%s: %s %s, %s: %d bytes differ, first at %s" % (
                what, self.step.name, self.size, k, len(bad), bad[:8])


# ---- the pair matchers

def _partial_items(hook, ncu, n1, n2, *lead):
    """The planner's bound on the items of partials (its host hook; no device needed)."""
    from cudasift_amd import capi
    n1, n2 = i32(n1), i32(n2)
    plan5 = np.zeros(5 * max(len(n1), 1), np.int32)
    ni, ch, pb = C.c_int(), C.c_int(), C.c_int()
    capi.check(getattr(capi.lib(), hook)(ncu, *lead, len(n1), n1.ctypes.data, n2.ctypes.data, plan5.ctypes.data,
                                         C.byref(ni), C.byref(ch), C.byref(pb)), hook)
    return pb.value


class MatchPairs(Step):
    """misift_match_pairs_batch with mutual = 1 on one packed batch matched against itself: a window of pairs, a pair
    backwards, a self pair, an empty frame, a frame of count -1 and one over max_pts (its pairs get -1 and no row)."""
    name = "match_pairs_batch"
    i8 = False
    SHAPES = dict(small=([130, 33, 200, 64, 0, 77, 20], 131, 21),                # frame sizes, max_pts, seed
                  large=([700, 513, 300, 900, 128, 450, 0, 31, 640], 701, 22),
                  huge=([700, 513, 300, 900, 128, 450, 0, 31, 640], 1401, 22))
    no_huge = ("max_pts is a capacity of the keys (8 bytes per pair and row) but also of the output (576 bytes per pair "
               "and row): the 4.3 MB of keys that lift this call above the int8 matcher's partials mean about 310 MB "
               "of rows")
    PART_BYTES = 128 * 8 * 3 * 4                                 # an item: 128 rows x 8 classes x (max, second, index)

    def build(self, size):
        sizes, max_pts, seed = self.SHAPES[size]
        counts = list(sizes)
        counts[-2] = -1
        fr = frames(sizes, seed, self.i8)
        recs, offs, _ = layout(fr, counts, False, min_stride=0, pad_error=0.0)
        n = len(sizes)
        pairs = [(f, g) for f in range(n) for g in range(f + 1, min(f + 3, n))] + [(n - 1, 0), (1, 1)]
        case = dict(recs=recs, counts=i32(counts), offs=offs, max_pts=max_pts, pairs=i32(pairs))
        if self.i8:
            case["q"] = quantize_np(recs["data"]).reshape(len(recs), 128)
        return case

    def lists(self, case):
        return dict(pairs=case["pairs"].copy())

    def other_lists(self, case):
        return dict(pairs=case["pairs"][::-1].copy())

    def uploads(self, case):
        return {k: case[k] for k in ("recs", "counts", "offs") + (("q",) if self.i8 else ())}

    def outputs(self, case):
        npairs = len(case["pairs"])
        return dict(out=np.full(npairs * case["max_pts"] * 576, POISON, np.uint8), out_counts=poisoned(npairs),
                    num_matched=poisoned(npairs))

    def enqueue(self, ctx, case, dev, lists):
        ctx.match_pairs_batch(lists["pairs"], dev["recs"], len(case["counts"]), dev["counts"], dev["offs"], 0,
                              max_pts=case["max_pts"], mutual=1, out=dev["out"], out_counts=dev["out_counts"],
                              num_matched=dev["num_matched"])

    def pair_rows(self, case, p1, p2, f1, f2):
        return expected_pair(p1, p2, False, False, True)

    def expected(self, case, lists):
        from cudasift_amd import capi
        pairs, mp = lists["pairs"], case["max_pts"]
        out = np.frombuffer(bytes([POISON]) * (576 * len(pairs) * mp), capi.POINT_DTYPE).copy()
        oc, nm = np.zeros(len(pairs), np.int32), np.zeros(len(pairs), np.int32)
        memo = case.setdefault("memo", {})
        for i, (f1, f2) in enumerate(pairs.tolist()):
            n1, n2 = max(int(case["counts"][f1]), 0), max(int(case["counts"][f2]), 0)
            if n1 > mp or n2 > mp:
                oc[i] = nm[i] = -1
                continue
            if (f1, f2) not in memo:
                memo[f1, f2] = self.pair_rows(case, case["recs"][span(case["offs"], 0, f1, n1)],
                                              case["recs"][span(case["offs"], 0, f2, n2)], f1, f2)
            e, k = memo[f1, f2]
            for fld in OUT_FIELDS:
                out[fld][i * mp:i * mp + n1] = e[fld]
            oc[i], nm[i] = n1, k
        return dict(out=out, out_counts=oc, num_matched=nm)

    def part_bytes(self, case, ncu):
        c = np.maximum(case["counts"], 0)
        p = case["pairs"]
        return self.PART_BYTES * _partial_items("misift_test_match_batch_plan", ncu, c[p[:, 0]], c[p[:, 1]], 0)

    def tmp_bytes(self, case, ncu):
        """The partials, then the mutual check's key per (pair, column)."""
        return self.part_bytes(case, ncu) + 8 * len(case["pairs"]) * case["max_pts"]


class MatchPairsI8(MatchPairs):
    """misift_match_pairs_batch_i8 with mutual = 1 on the same shapes; the 8-bit descriptors are quantised on the host by
    the rule test_match_i8_cpu.py pins to the library's."""
    name = "match_pairs_batch_i8"
    i8 = True
    sizes, no_huge = SIZES, None                                 # its own partials are the largest: a few keys more do
    PART_BYTES = 128 * 16                                        # an item's partials: 128 rows x int4

    def enqueue(self, ctx, case, dev, lists):
        ctx.match_pairs_batch_i8(lists["pairs"], dev["recs"], dev["q"], len(case["counts"]), dev["counts"], dev["offs"],
                                 0, max_pts=case["max_pts"], mutual=1, out=dev["out"], out_counts=dev["out_counts"],
                                 num_matched=dev["num_matched"])

    def pair_rows(self, case, p1, p2, f1, f2):
        from test_match_pairs_i8_cpu import expected_pair_i8
        n1, n2 = len(p1), len(p2)
        return expected_pair_i8(p1, case["q"][span(case["offs"], 0, f1, n1)], p2, case["q"][span(case["offs"], 0, f2, n2)],
                                True)

    def part_bytes(self, case, ncu):
        c = np.maximum(case["counts"], 0)
        p = case["pairs"]
        return self.PART_BYTES * _partial_items("misift_test_match_i8_plan", ncu, c[p[:, 0]], c[p[:, 1]])


# ---- the guided matchers

class Guided(Step):
    """misift_match_guided_batch / misift_match_epipolar_batch on the `offset` scene of guided_cases.py (boxes far from
    the origin, rows of 129, 65, 64, 63 and 1): without its first pair at `small`, whole at `large`.  The set-1 records
    are written in place."""
    sizes = SIZES
    SHAPES = dict(small=(slice(1, None), 301), large=(slice(None), 2101), huge=(slice(None), 250001))

    def __init__(self, kind):
        super().__init__()
        self.kind, self.name = kind, "match_%s_batch" % kind

    def build(self, size):
        import guided_cases as gc
        s = gc.scene(self.kind, "offset")
        which, max_pts = self.SHAPES[size]
        if size == "huge" and self.kind == "epipolar":
            max_pts += 10000                                     # no two huge steps of one size: each grows the temp
        r1, o1, _ = layout(s.fr1, s.counts1, False, min_stride=0, pad_error=0.0)
        r2, o2, _ = layout(s.fr2, s.counts2, False, min_stride=0, pad_error=0.0)
        return dict(recs1=r1, counts1=i32(s.counts1), offs1=o1, recs2=r2, counts2=i32(s.counts2), offs2=o2,
                    pairs=i32(s.pairs[which]), mats=np.ascontiguousarray(np.stack(s.mats[which]), f32).reshape(-1, 9),
                    radius=s.radius, max_pts=max_pts)

    def lists(self, case):
        return dict(pairs=case["pairs"].copy())

    def other_lists(self, case):
        return dict(pairs=np.roll(case["pairs"], 1, axis=0).copy())          # pair i keeps matrix i, and gets other frames

    def uploads(self, case):
        return {k: case[k] for k in ("recs1", "counts1", "offs1", "recs2", "counts2", "offs2", "mats")}

    def outputs(self, case):
        return dict(num_found=poisoned(len(case["pairs"])))

    def enqueue(self, ctx, case, dev, lists):
        call = ctx.match_guided_batch if self.kind == "guided" else ctx.match_epipolar_batch
        call(lists["pairs"], dev["recs1"], len(case["counts1"]), dev["counts1"], dev["mats"], case["radius"], dev["offs1"],
             0, dev["recs2"], len(case["counts2"]), dev["counts2"], dev["offs2"], 0, max_pts=case["max_pts"],
             num_found=dev["num_found"])

    def expected(self, case, lists):
        import guided_cases as gc
        restated = gc.expected_guided if self.kind == "guided" else gc.expected_epipolar
        exp, nf = restated([tuple(p) for p in lists["pairs"].tolist()], case["mats"].reshape(-1, 3, 3), case["radius"],
                           case["max_pts"], case["recs1"], case["counts1"], case["offs1"], 0, case["recs2"],
                           case["counts2"], case["offs2"], 0)
        return dict(recs1=exp, num_found=nf)

    def tmp_bytes(self, case, ncu):
        """Pair starts, a pair entry (16 bytes) per pair; per distinct set-2 frame a grid (64 bytes), 4096 + 4 cell
        starts and max_pts binned positions of 16 bytes."""
        npairs, nd = len(case["pairs"]), len(set(case["pairs"][:, 1].tolist()))
        return align16(4 * (npairs + 1)) + 16 * npairs + 64 * nd + 4 * (64 * 64 + 4) * nd + 16 * nd * case["max_pts"]


# ---- tracks

TRACK_GATES = (0.85, 0.95, INF)


def _tracks_case(size, max_records=None):
    """max_records: a capacity beyond the records the frames hold (the frames stay where they are)."""
    from test_tracks_cpu import blank_rows, plant, window_pairs
    sizes, window, mp, seed, ntracks = dict(small=([40, 17, 64, 0, 33, 25], 2, 65, 71, 30),
                                            large=([300, 64, 500, 0, 65, 1, 63, 300, 129], 3, 501, 72, 200))[size]
    counts = list(sizes)
    rng = np.random.default_rng(seed)
    pairs = window_pairs(list(range(len(sizes))), window)
    rows = blank_rows(len(pairs), mp, seed)
    usable = [f for f in range(len(sizes)) if counts[f] > 0]
    plant(rows, mp, pairs, planted_members(sizes, usable, [1 + t % len(usable) for t in range(ntracks)], rng), 0.2, rng)
    offs = np.concatenate([[0], np.cumsum(np.maximum(counts, 0))]).astype(np.int32)
    return dict(pairs=i32(pairs), rows=rows, row_counts=i32([max(counts[a], 0) for a, _ in pairs]), max_pts=mp,
                counts=i32(counts), offs=offs, max_records=int(offs[-1]) if max_records is None else max_records)


class LinkTracks(Step):
    """misift_link_tracks_batch on planted tracks with dropped edges over a window of pairs, an empty frame among them."""
    name = "link_tracks_batch"
    sizes = SIZES
    OUT = ("track", "track_len", "track_frames", "summary")

    def build(self, size):
        case = _tracks_case("small", 900001) if size == "huge" else _tracks_case(size)     # huge: max_records alone
        assert case["max_records"] % 16 and case["max_pts"] % 16
        return case

    def lists(self, case):
        return dict(pairs=case["pairs"].copy())

    def other_lists(self, case):
        return dict(pairs=case["pairs"][::-1].copy())           # pair i keeps its rows and gets other frames: other edges

    def uploads(self, case):
        return {k: case[k] for k in ("rows", "row_counts", "counts", "offs")}

    def outputs(self, case):
        return dict(track=poisoned(case["max_records"]), track_len=poisoned(case["max_records"]),
                    track_frames=poisoned(case["max_records"]), summary=poisoned(8))

    def enqueue(self, ctx, case, dev, lists):
        ctx.link_tracks_batch(lists["pairs"], dev["rows"], dev["row_counts"], case["max_pts"], len(case["counts"]),
                              dev["counts"], dev["offs"], 0, max_records=case["max_records"], min_score=TRACK_GATES[0],
                              max_ambiguity=TRACK_GATES[1], max_error=TRACK_GATES[2], track=dev["track"],
                              track_len=dev["track_len"], track_frames=dev["track_frames"], summary=dev["summary"])

    def expected(self, case, lists):
        from test_tracks_cpu import expected_tracks
        e = expected_tracks([tuple(p) for p in lists["pairs"].tolist()], case["rows"], case["row_counts"], case["max_pts"],
                            case["counts"], case["offs"], 0, case["max_records"], TRACK_GATES, poison=POISON_WORD)
        return dict(zip(self.OUT, e))

    def tmp_bytes(self, case, ncu):
        """include/misift.h: 20 bytes per record of max_records plus 16 per pair (each part rounded up to 16)."""
        return align16(4 * case["max_records"]) + align16(16 * len(case["pairs"])) + 16 * case["max_records"]


class ExportTracks(Step):
    """misift_export_tracks_batch on the labels of the link_tracks step of the same size (from the restatement), the
    positions random bit patterns; max_tracks and max_obs below what the labels hold, so a track is left out whole."""
    name = "export_tracks_batch"
    sizes = SIZES
    carries_lists = False
    OUT = ("track_offsets", "track_root", "obs", "record_obs", "summary")

    def build(self, size):
        from test_tracks_cpu import expected_tracks
        t = _tracks_case("small", 1100003) if size == "huge" else _tracks_case(size)       # huge: max_records alone
        labels = expected_tracks([tuple(p) for p in t["pairs"].tolist()], t["rows"], t["row_counts"], t["max_pts"],
                                 t["counts"], t["offs"], 0, t["max_records"], TRACK_GATES, poison=POISON_WORD)
        n = int(t["offs"][-1])                                  # the records the frames hold
        case = dict(recs=fabricated_records(n, 80 + len(t["counts"])), counts=t["counts"], offs=t["offs"],
                    max_records=t["max_records"], track=labels[0], track_len=labels[1], track_frames=labels[2], min_len=2,
                    consistent_only=1, max_tracks=n // 5 + 1, max_obs=n // 2 + 3)
        assert case["max_obs"] % 16
        return case

    def uploads(self, case):
        return {k: case[k] for k in ("recs", "counts", "offs", "track", "track_len", "track_frames")}

    def outputs(self, case):
        return dict(track_offsets=poisoned(case["max_tracks"] + 1), track_root=poisoned(case["max_tracks"]),
                    obs=poisoned(4 * case["max_obs"]), record_obs=poisoned(case["max_records"]), summary=poisoned(8))

    def enqueue(self, ctx, case, dev, lists):
        ctx.export_tracks_batch(dev["recs"], len(case["counts"]), dev["counts"], dev["offs"], 0,
                                max_records=case["max_records"], track=dev["track"], track_len=dev["track_len"],
                                track_frames=dev["track_frames"], min_len=case["min_len"],
                                consistent_only=case["consistent_only"], max_tracks=case["max_tracks"],
                                max_obs=case["max_obs"], track_offsets=dev["track_offsets"], track_root=dev["track_root"],
                                obs=dev["obs"], record_obs=dev["record_obs"], summary=dev["summary"])

    def expected(self, case, lists):
        from test_tracks_export_cpu import expected_export
        e = expected_export(xy_bits(case["recs"]), case["counts"], case["offs"], 0, case["max_records"], case["track"],
                            case["track_len"], case["track_frames"], case["min_len"], case["consistent_only"],
                            case["max_tracks"], case["max_obs"], POISON_WORD)
        return dict(zip(self.OUT, e))

    def tmp_bytes(self, case, ncu):
        """include/misift.h: 16 bytes per record of max_records (four arrays, each rounded up to 16) plus 8 per 2048."""
        n = case["max_records"]
        return 4 * align16(4 * n) + 8 * ((n + 2047) // 2048)


# ---- the pose graph and what follows it

class LinkPoses(Step):
    """misift_link_poses_batch: five pairs in a row at `small`, every small sample count in CHAIN and FAN at `large`."""
    name = "link_poses_batch"
    no_huge = ("no capacity argument: 12 bytes per link and pair, so 1.4 million links, each a 256-thread workgroup with "
               "its own restated median")
    OUT = ("link_ratio", "link_common", "pair_scale", "cam", "cam_pair", "summary")

    def build(self, size):
        import posegraph_cases as G
        case = G.graph_cases()[0][1] if size == "small" else G.count_case()
        assert case["max_pts"] % 16
        return case

    def lists(self, case):
        return dict(pairs=i32(case["pairs"]).reshape(-1, 2).copy(), links=i32(case["links"]).reshape(-1, 3).copy(),
                    walk=i32(case["walk"]).reshape(-1).copy())

    def other_lists(self, case):
        own = self.lists(case)                                   # the same graph, its links and its walk backwards
        return dict(pairs=own["pairs"], links=own["links"][::-1].copy(), walk=own["walk"][::-1].copy())

    def uploads(self, case):
        return dict(rows=case["rows"], row_counts=i32(case["row_counts"]), pose=np.ascontiguousarray(case["pose"], f32),
                    num_front=i32(case["num_front"]), xyz=np.ascontiguousarray(case["xyz"], f32))

    def sizes_of(self, case):
        nl, npairs, n = len(case["links"]), len(case["pairs"]), case["nimages"]
        return dict(link_ratio=nl, link_common=nl, pair_scale=npairs, cam=12 * n, cam_pair=n, summary=8)

    def outputs(self, case):
        return {k: poisoned(n) for k, n in self.sizes_of(case).items()}

    def enqueue(self, ctx, case, dev, lists):
        ctx.link_poses_batch(lists["pairs"], case["nimages"], dev["rows"], dev["row_counts"], case["max_pts"], dev["pose"],
                             dev["num_front"], dev["xyz"], lists["links"], case["seed_pair"], case["root_image"],
                             lists["walk"], min_common=case["min_common"], min_score=GATES[0], max_ambiguity=GATES[1],
                             max_error=case["max_error"], **{k: dev[k] for k in self.OUT})

    def expected(self, case, lists):
        import posegraph_cases as G
        e = G.expected_link_poses(dict(case, **lists))
        out = {}
        for k, n in self.sizes_of(case).items():
            out[k] = u32(e[k]) if n else poisoned(0)             # an output of no entry keeps its one poisoned word
            assert len(out[k]) == max(n, 1), (k, len(out[k]), n)
        return out

    def tmp_bytes(self, case, ncu):
        """include/misift.h: 12 bytes per link, 12 per pair and 4 per walk entry, plus 16."""
        return 12 * len(case["links"]) + 12 * len(case["pairs"]) + 4 * len(case["walk"]) + 16


def _track_inputs(case, more=()):
    """The device inputs the three calls behind the export share, at exactly the sizes they state."""
    import triangulate_cases as TC
    mt, mo = case["max_tracks"], case["max_obs"]
    ins = dict(track_offsets=i32(case["track_offsets"][:mt + 1]), obs=np.ascontiguousarray(case["obs"][:mo], TC.OBS_DTYPE),
               export_summary=i32(case["export_summary"]), cam=np.ascontiguousarray(case["cam"], f32),
               cam_pair=i32(case["cam_pair"]))
    if "points" in more:
        ins.update(points=np.ascontiguousarray(case["points"], f32).reshape(-1, 4), point_status=i32(case["point_status"]))
        assert len(ins["points"]) == mt == len(ins["point_status"])
    assert len(ins["track_offsets"]) == mt + 1 and len(ins["obs"]) == mo and len(ins["cam"]) == case["nimages"]
    return ins


def _other_intrinsics(K):
    """Other in-range intrinsics of the same shape: every image gets its neighbour's, and a focal length 3 % longer."""
    K = np.roll(np.ascontiguousarray(K, f32), 1, axis=0).copy()
    K[:, :2] *= f32(1.03)
    return K


class Triangulate(Step):
    """misift_triangulate_tracks_batch with one image more than the kernel stages on chip at `small` (so that the
    intrinsics go through temp at all), four times that at `large`."""
    name = "triangulate_tracks_batch"
    sizes = SIZES
    OUT = ("points", "point_views", "point_status", "obs_error", "summary")

    def build(self, size):
        import pose_cases as PC
        import triangulate_cases as TC
        n = TC.capacity() + 1
        if size != "huge":
            return TC.capacity_case(n if size == "small" else 4 * n - 1)
        base, n = self.case("small"), 1100001                    # huge: images without a camera behind the small case's
        cam, pair = np.zeros((n, 12), f32), np.full(n, TC.UNSET, np.int32)
        cam[:base["nimages"]], pair[:base["nimages"]] = base["cam"], base["cam_pair"]
        K = np.tile(np.array(PC.K_A, f32), (n, 1))
        K[:base["nimages"]] = base["intrinsics"]
        return dict(base, nimages=n, cam=cam, cam_pair=pair, intrinsics=K, memo={})

    def lists(self, case):
        return dict(intrinsics=np.ascontiguousarray(case["intrinsics"], f32).reshape(-1, 4).copy())

    def other_lists(self, case):
        return dict(intrinsics=_other_intrinsics(case["intrinsics"]))

    def uploads(self, case):
        return _track_inputs(case)

    def outputs(self, case):
        mt, mo = case["max_tracks"], case["max_obs"]
        return dict(points=poisoned(4 * mt), point_views=poisoned(mt), point_status=poisoned(mt), obs_error=poisoned(mo),
                    summary=poisoned(8))

    def enqueue(self, ctx, case, dev, lists):
        ctx.triangulate_tracks_batch(case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"],
                                     dev["export_summary"], case["nimages"], dev["cam"], dev["cam_pair"],
                                     lists["intrinsics"], min_views=case["min_views"], num_loops=case["num_loops"],
                                     **{k: dev[k] for k in self.OUT})

    def expected(self, case, lists):
        import triangulate_cases as TC
        e = TC.expected_triangulate(dict(case, intrinsics=lists["intrinsics"], memo={}))
        return {k: e[k] for k in self.OUT}

    def tmp_bytes(self, case, ncu):
        """include/misift.h: beyond 512 images, a copy of the intrinsics in 16 bytes per image."""
        import triangulate_cases as TC
        return 16 * case["nimages"] if case["nimages"] > TC.capacity() else 0


def _more_slots(case, max_obs):
    """The case under a larger max_obs, a capacity: the observations padded to it, O from the device as it was."""
    obs = np.zeros(max_obs, case["obs"].dtype)
    obs[:len(case["obs"])] = case["obs"]
    out = dict(case, max_obs=max_obs, obs=obs)
    out.pop("memo_resect", None)
    return out


class Refine(Step):
    """misift_refine_cameras_batch on the spread scene: 257 slots of 4 images at `small`, 1025 of 9 at `large`."""
    name = "refine_cameras_batch"
    sizes = SIZES

    def build(self, size):
        import refine_cases as RC
        if size == "huge":
            return _more_slots(self.case("small"), 2300001)
        case = RC.spread_case(257, hold=(2,), orthonormalise=1) if size == "small" else \
            RC.spread_case(1025, nimages=9, seed=64, hold=(2, 5), orthonormalise=1)
        assert case["max_obs"] % 16
        return case

    def lists(self, case):
        return dict(intrinsics=np.ascontiguousarray(case["intrinsics"], f32).reshape(-1, 4).copy(),
                    hold=i32(case["hold"]).reshape(-1).copy())

    def other_lists(self, case):
        return dict(intrinsics=_other_intrinsics(case["intrinsics"]), hold=i32(case["hold"]).reshape(-1) + 1)

    def uploads(self, case):
        return _track_inputs(case, ("points",))

    def outputs(self, case):
        n = case["nimages"]
        return dict(cam_out=poisoned(12 * n), cam_obs=poisoned(n), cam_rms=poisoned(2 * n), cam_steps=poisoned(n),
                    cam_status=poisoned(n), summary=poisoned(8))

    def enqueue(self, ctx, case, dev, lists):
        import refine_cases as RC
        ctx.refine_cameras_batch(case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"],
                                 dev["export_summary"], dev["points"], dev["point_status"], case["nimages"], dev["cam"],
                                 dev["cam_pair"], lists["intrinsics"], hold=lists["hold"], min_obs=case["min_obs"],
                                 num_loops=case["num_loops"], max_error=case["max_error"],
                                 orthonormalise=case["orthonormalise"], **{k: dev[k] for k in RC.OUTPUTS})

    def expected(self, case, lists):
        import refine_cases as RC
        e = RC.expected_refine(RC.variant(case, intrinsics=lists["intrinsics"], hold=tuple(lists["hold"].tolist())))
        return {k: e[k] for k in RC.OUTPUTS}

    def tmp_bytes(self, case, ncu):
        """include/misift.h: 8 bytes per slot of max_obs."""
        return 8 * case["max_obs"]


class Resect(Step):
    """misift_resect_cameras_batch: three images of the small scene (slack behind T and O, points behind the cameras) at
    49 loops; four of the edge scene (7, 511, 513 and 1025 candidates) at 100 loops."""
    name = "resect_cameras_batch"
    sizes = SIZES

    def build(self, size):
        import resect_cases as RC
        if size == "huge":
            return dict(_more_slots(self.case("small"), 2400001), memo_resect={})
        if size == "small":
            return RC.resect_case(RC.small_scene()["case"], [2, 3, 0], max_cand=91, num_loops=49, min_inliers=12)
        return RC.resect_case(RC.edge_scene()["case"], [7, 6, 4, 3], max_cand=1030, num_loops=100, min_inliers=12)

    def lists(self, case):
        return dict(intrinsics=np.ascontiguousarray(case["intrinsics"], f32).reshape(-1, 4).copy(),
                    images=i32(case["images"]).copy(), seeds=np.ascontiguousarray(case["seeds"], np.uint32).copy())

    def other_lists(self, case):
        own = self.lists(case)
        return dict(intrinsics=_other_intrinsics(case["intrinsics"]), images=own["images"][::-1].copy(),
                    seeds=own["seeds"] + np.uint32(1000))

    def uploads(self, case):
        return _track_inputs(case, ("points",))

    def outputs(self, case):
        n = len(case["images"])
        return dict(res_cam=poisoned(12 * n), res_cand=poisoned(n), res_inliers=poisoned(n), res_status=poisoned(n),
                    summary=poisoned(8))

    def enqueue(self, ctx, case, dev, lists):
        import resect_cases as RC
        ctx.resect_cameras_batch(case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"],
                                 dev["export_summary"], dev["points"], dev["point_status"], case["nimages"],
                                 lists["intrinsics"], lists["images"], lists["seeds"], case["max_cand"],
                                 num_loops=case["num_loops"], thresh=case["thresh"], min_inliers=case["min_inliers"],
                                 only_unset=case["only_unset"], install=case["install"], cam=dev["cam"],
                                 cam_pair=dev["cam_pair"], **{k: dev[k] for k in RC.OUTPUTS})

    def expected(self, case, lists):
        import resect_cases as RC
        e = RC.expected_resect(RC.variant(case, memo_resect={}, **lists))
        return {k: e[k] for k in RC.OUTPUTS + ("cam", "cam_pair")}

    def tmp_bytes(self, case, ncu):
        """include/misift.h: 8 bytes per slot, and per entry 20 bytes per candidate of min(max_cand, max_obs) and 76 per
        hypothesis (both rounded up to 16), plus the entry's 16 bytes of meta."""
        cap = align16(min(case["max_cand"], case["max_obs"]))
        return 8 * case["max_obs"] + len(case["images"]) * (20 * cap + 76 * align16(case["num_loops"]) + 16)


# ---- the calls on frames of stored matches

class RecoverPose(Step):
    """misift_recover_pose_batch (no temp, a copied frame list and a copied intrinsics list) on the frame counts of
    test_gpu_pose.py: a frame of count -1, an empty one, fewer than a wave, around the workgroup's 256 threads."""
    name = "recover_pose_batch"
    temp = False
    no_huge = "uses no temp"
    SHAPES = dict(small=([40, 0, 7, 8, 65, 30], [4, 2, 0, 1, 3]),
                  large=([40, 0, 1, 7, 8, 255, 256, 257, 513, 30], [8, 3, 0, 6, 1, 5, 2, 7, 4]))

    def build(self, size):
        import pose_cases as PC
        sizes, sel = self.SHAPES[size]
        made = [PC.planted_frame(n, 300 + f, PC.K_B if f % 2 else PC.K_A) for f, n in enumerate(sizes)]
        counts = [-1] + sizes[1:]
        recs, offs, _ = layout([m[0] for m in made], counts, False, min_stride=0, pad_error=-7.0)
        return dict(recs=recs, counts=i32(counts), offs=offs, sel=i32(sel), fr=[m[0] for m in made],
                    F=np.ascontiguousarray(np.stack([made[f][1] for f in sel]), f32).reshape(-1, 9),
                    K=np.ascontiguousarray(np.stack([made[f][2] for f in sel]), f32).reshape(-1, 8))

    def lists(self, case):
        return dict(frames=case["sel"].copy(), intrinsics=case["K"].copy())

    def other_lists(self, case):
        return dict(frames=np.roll(case["sel"], 1).copy(), intrinsics=np.roll(case["K"], 2, axis=0).copy())

    def uploads(self, case):
        return {k: case[k] for k in ("recs", "counts", "offs", "F")}

    def zeroed(self, case):
        return dict(Step.zeroed(self, case), fr=[np.zeros_like(p) for p in case["fr"]])

    def outputs(self, case):
        ns = len(case["sel"])
        return dict(pose=poisoned(12 * ns), num_front=poisoned(ns), votes=poisoned(4 * ns),
                    xyz=poisoned(4 * len(case["recs"])))

    def enqueue(self, ctx, case, dev, lists):
        import pose_cases as PC
        ctx.recover_pose_batch(lists["frames"], lists["intrinsics"], dev["recs"], len(case["counts"]), dev["counts"],
                               dev["F"], dev["offs"], 0, pose=dev["pose"], num_front=dev["num_front"], votes=dev["votes"],
                               xyz=dev["xyz"], min_score=GATES[0], max_ambiguity=GATES[1], thresh=PC.THRESH)

    def expected(self, case, lists):
        import pose_cases as PC
        ns = len(case["sel"])
        pose, front, votes = np.zeros((ns, 12), f32), np.zeros(ns, np.int32), np.zeros((ns, 4), np.int32)
        xyz = np.full((len(case["recs"]), 4), POISON_WORD, np.uint32)        # rows of frames not selected stay poisoned
        for i, f in enumerate(lists["frames"].tolist()):
            n = int(case["counts"][f])
            e = PC.expected_pose(case["fr"][f], n, case["F"][i], lists["intrinsics"][i], *GATES, PC.THRESH)
            pose[i], front[i], votes[i] = e["pose"], e["num_front"], e["votes"]
            xyz[span(case["offs"], 0, f, max(n, 0))] = e["xyz"].view(np.uint32)
        return dict(pose=pose, num_front=front, votes=votes, xyz=xyz)

    def tmp_bytes(self, case, ncu):
        return 0


class ImproveFundamental(Step):
    """misift_improve_fundamental_batch (no temp, a copied frame list) on the frame counts of
    test_gpu_fundamental_refine.py; F and the records' match_error are written in place."""
    name = "improve_fundamental_batch"
    temp = False
    no_huge = "uses no temp"
    SHAPES = dict(small=([40, 0, 7, 9, 70, 30], [4, 0, 3, 1, 2], 2),
                  large=([40, 0, 7, 8, 9, 255, 256, 257, 513, 30], [8, 3, 0, 7, 1, 5, 2, 4, 6], 5))

    def build(self, size):
        import fundamental_cases as FC
        sizes, sel, loops = self.SHAPES[size]
        fr = [FC.noisy_records(n, f) for f, n in enumerate(sizes)]
        counts = [-1] + sizes[1:]
        recs, offs, _ = layout(fr, counts, False, min_stride=0, pad_error=-7.0)
        F0 = np.ascontiguousarray(np.stack([FC.start_F(fr[f], f) for f in sel]), f32).reshape(-1, 9)
        return dict(recs=recs, counts=i32(counts), offs=offs, sel=i32(sel), F=F0, loops=loops)

    def lists(self, case):
        return dict(frames=case["sel"].copy())

    def other_lists(self, case):
        return dict(frames=np.roll(case["sel"], 1).copy())     # entry i keeps its start F and gets another frame

    def uploads(self, case):
        return {k: case[k] for k in ("recs", "counts", "offs", "F")}

    def outputs(self, case):
        return dict(num_fit=poisoned(len(case["sel"])), num_rounds=poisoned(len(case["sel"])))

    def enqueue(self, ctx, case, dev, lists):
        ctx.improve_fundamental_batch(lists["frames"], dev["recs"], len(case["counts"]), dev["counts"], dev["F"],
                                      dev["offs"], 0, num_fit=dev["num_fit"], num_rounds=dev["num_rounds"],
                                      num_loops=case["loops"], min_score=GATES[0], max_ambiguity=GATES[1], thresh=1.0)

    def expected(self, case, lists):
        from test_fundamental_refine_cpu import expected_improve
        ns = len(case["sel"])
        want, F = case["recs"].copy(), np.zeros((ns, 9), f32)
        fit, rounds = np.zeros(ns, np.int32), np.zeros(ns, np.int32)
        for i, f in enumerate(lists["frames"].tolist()):
            n = int(case["counts"][f])
            sl = span(case["offs"], 0, f, max(n, 0))
            want[sl], F[i], fit[i], rounds[i] = expected_improve(case["recs"][sl], n, case["F"][i], case["loops"], *GATES,
                                                                 1.0)
        return dict(recs=want, F=F, num_fit=fit, num_rounds=rounds)

    def tmp_bytes(self, case, ncu):
        return 0


def _search_tmp(nsel, max_pts, loops, sample_params):
    """The layout of ransac_batch.hpp per entry: 4 coordinates and a valid flag per point of max_pts, a sample, a model
    and a count per hypothesis (both strides rounded up to 16), 4 words of meta; in 4-byte words."""
    return 4 * nsel * (5 * align16(max_pts) + (sample_params + 1) * align16(loops) + 4)


class FindFundamental(Step):
    """misift_find_fundamental_batch: three frames of 9, 8 and 40 records at 17 loops; the 15-entry batch of
    test_gpu_fundamental.py at 65 loops; and that batch under a max_pts of 79 999, which sizes the temp beyond every
    other step while the work stays what it was."""
    name = "find_fundamental_batch"
    sizes = SIZES

    def build(self, size):
        import fundamental_cases as FC
        if size == "small":
            fr = [FC.batch_records(9, 301, 9), FC.batch_records(8, 302), FC.batch_records(40, 303)]
            counts, sel, seeds, loops, max_pts = [9, 8, 40], [2, 0, 1], [7, 2 ** 32 - 1, 11], 17, 41
        else:
            fr, counts, sel, seeds, loops = _fundamental_batch(), FC.COUNTS, FC.SEL, FC.SEEDS, 65
            max_pts = FC.MAX_PTS if size == "large" else 79999
        recs, offs, _ = layout(fr, counts, False, min_stride=0, pad_error=-7.0)
        return dict(recs=recs, counts=i32(counts), offs=offs, sel=i32(sel), seeds=np.array(seeds, np.uint32), loops=loops,
                    max_pts=max_pts)

    def lists(self, case):
        return dict(frames=case["sel"].copy(), seeds=case["seeds"].copy())

    def other_lists(self, case):
        return dict(frames=np.roll(case["sel"], 1).copy(), seeds=case["seeds"] + np.uint32(5))

    def uploads(self, case):
        return {k: case[k] for k in ("recs", "counts", "offs")}

    def outputs(self, case):
        return dict(F=poisoned(9 * len(case["sel"])), num=poisoned(len(case["sel"])))

    def enqueue(self, ctx, case, dev, lists, loops=None, out=None):
        out = out or dev
        ctx.find_fundamental_batch(lists["frames"], lists["seeds"], dev["recs"], len(case["counts"]), dev["counts"],
                                   dev["offs"], 0, max_pts=case["max_pts"], num_loops=loops or case["loops"],
                                   min_score=GATES[0], max_ambiguity=GATES[1], thresh=1.0, fundamental=out["F"],
                                   num_inliers=out["num"])

    def expected(self, case, lists):
        from test_fundamental_cpu import expected_find
        ns = len(case["sel"])
        F, num = np.zeros((ns, 9), f32), np.zeros(ns, np.int32)
        for i, (f, s) in enumerate(zip(lists["frames"].tolist(), lists["seeds"].tolist())):
            n = int(case["counts"][f])
            F[i], num[i] = expected_find(case["recs"][span(case["offs"], 0, f, max(n, 0))], n, s, case["loops"], *GATES,
                                         1.0, case["max_pts"])
        return dict(F=F, num=num)

    def tmp_bytes(self, case, ncu):
        return _search_tmp(len(case["sel"]), case["max_pts"], case["loops"], 8 + 9)


@functools.lru_cache(maxsize=None)
def _fundamental_batch():
    import fundamental_cases as FC
    return FC.make_batch()


class FindHomography(Step):
    """misift_find_homography_batch: frames of 9, 8 and 40 records with 8, 8 and 33 valid ones at 17 loops; six frames of
    up to 1500 stored matches at 50 loops; and those under a max_pts of 199 999.  Expected: the oracle's FindHomography
    after srand(seed), what test_gpu_homography_batch.py holds the batch call to."""
    name = "find_homography_batch"
    sizes = SIZES
    FIND = dict(min_score=0.85, max_ambiguity=0.95, thresh=5.0)

    def build(self, size):
        if size == "small":
            fr = [gated_frame(9, 41, 8), gated_frame(8, 42, 8), gated_frame(40, 34, 33)]
            sel, seeds, loops, max_pts = [1, 2, 0], [7, 2 ** 32 - 1, 11], 17, 41
        else:
            fr = matched_frames([0, 7, 8, 40, 777, 1500], 3)
            sel, seeds, loops = [5, 0, 4, 1, 3, 2], [11, 12, 13, 0, 2 ** 32 - 1, 12345], 50
            max_pts = 1501 if size == "large" else 199999
        counts = [len(p) for p in fr]
        recs, offs, _ = layout(fr, counts, False, min_stride=1, pad_error=-7.0)
        return dict(recs=recs, counts=i32(counts), offs=offs, sel=i32(sel), seeds=np.array(seeds, np.uint32), loops=loops,
                    max_pts=max_pts)

    lists = FindFundamental.lists
    other_lists = FindFundamental.other_lists
    uploads = FindFundamental.uploads

    def outputs(self, case):
        return dict(H=poisoned(9 * len(case["sel"])), num=poisoned(len(case["sel"])))

    def enqueue(self, ctx, case, dev, lists):
        ctx.find_homography_batch(lists["frames"], lists["seeds"], dev["recs"], len(case["counts"]), dev["counts"],
                                  dev["offs"], 0, max_pts=case["max_pts"], num_loops=case["loops"], homography=dev["H"],
                                  num_matches=dev["num"], **self.FIND)

    def expected(self, case, lists):
        o = orc()
        ns = len(case["sel"])
        H, num = np.tile(np.eye(3, dtype=f32).reshape(9), (ns, 1)), np.zeros(ns, np.int32)
        for i, (f, s) in enumerate(zip(lists["frames"].tolist(), lists["seeds"].tolist())):
            n = max(int(case["counts"][f]), 0)
            if n > case["max_pts"]:
                num[i] = -1
            elif n >= 8:
                o.srand(s)
                He, ne, _ = o.find_homography(case["recs"][span(case["offs"], 0, f, n)].copy(), n,
                                              num_loops=case["loops"], **self.FIND)
                H[i], num[i] = np.asarray(He, f32).reshape(9), ne
        return dict(H=H, num=num)

    def tmp_bytes(self, case, ncu):
        return _search_tmp(len(case["sel"]), case["max_pts"], case["loops"], 4 + 8)


# ---- the calls only stream_table() holds: `small` alone, and no tmp_bytes() (the stream tests assert only that the temp
# does not change).  Their host lists (intrinsics, hold, group, ranges, seeds, frames) are arguments of the case, handed
# over as the case holds them: carries_lists is False and lists() empty.

def select_sizes(case):
    import select_cases as SC
    n, top, mp = len(case["counts"]), case["top"], case["max_pairs"]
    return dict(zip(SC.OUTPUTS, (n * top, n, n * n, 2 * mp, mp, 8)))


def select_tmp_bytes(case):
    """include/misift.h: the gathered descriptors, the keep flags, 24 bytes per frame, each part rounded up to 16, and
    16."""
    n, hp = len(case["counts"]), (case["top"] + 31) // 32 * 32
    return align16(n * hp * 128) + align16(n * n) + 16 * n + 2 * align16(4 * n) + 16


class SelectStep(Step):
    """misift_select_pairs_batch: a call that hands the library no host list."""
    name = "select_pairs_batch"
    carries_lists = False
    CASES = dict(small="ring_small", large="frames_65_top33")
    INPUTS = ("recs", "q", "counts", "offs")

    def build(self, size):
        import select_cases as SC
        return SC.all_cases()[self.CASES[size]]

    def uploads(self, case):
        return {k: case[k] for k in self.INPUTS if case[k] is not None}

    def zeroed(self, case):
        return dict(Step.zeroed(self, case), memo={})            # select_cases shares stage 1 and 2 among variants

    def outputs(self, case):
        return {k: poisoned(w) for k, w in select_sizes(case).items()}

    def enqueue(self, ctx, case, dev, lists):
        import select_cases as SC
        ctx.select_pairs_batch(dev["recs"], dev["q"], len(case["counts"]), dev["counts"], dev.get("offs"), case["stride"],
                               **{k: case[k] for k in SC.ARGS}, **{k: dev[k] for k in SC.OUTPUTS})

    def expected(self, case, lists):
        import select_cases as SC
        return SC.expected(case)

    def tmp_bytes(self, case, ncu):
        return select_tmp_bytes(case)


class _Small(Step):
    sizes = ("small",)
    carries_lists = False
    no_huge = "not in table(): the stream tests hold the temp to what it was"


def _without(e, *keys):
    return {k: v for k, v in e.items() if k not in keys}


class Bundle(_Small):
    """The four bundle adjusters on one planted scene of 4 images and 40 tracks, 2 steps of 4 CG iterations: plain, under
    a Huber loss, with one focal group, with one radial group."""
    CALLS = dict(plain="adjust_bundle_batch", robust="adjust_bundle_robust_batch", focal="adjust_bundle_focal_batch",
                 radial="adjust_bundle_radial_batch")
    KW = ("hold", "min_views", "min_obs", "num_loops", "cg_iters", "max_error", "lambda0", "orthonormalise")

    def __init__(self, kind):
        super().__init__()
        self.kind, self.name = kind, self.CALLS[kind]

    def mod(self):
        import bundle_cases as BC
        import bundle_focal_cases as BF
        import bundle_radial_cases as BD
        import bundle_robust_cases as BR
        return dict(plain=BC, robust=BR, focal=BF, radial=BD)[self.kind]

    def build(self, size):
        import bundle_cases as BC
        import bundle_focal_cases as BF
        import bundle_radial_cases as BD
        import bundle_robust_cases as BR
        base = BC.planted(40, 4, 1, num_loops=2, cg_iters=4)["case"]
        return dict(plain=lambda: base, robust=lambda: BR.robust(base, BR.HUBER, 2.0), focal=lambda: BF.one_group(base),
                    radial=lambda: BD.one_group(base))[self.kind]()

    def uploads(self, case):
        import filter_cases as FC
        return FC.inputs(case)

    def outputs(self, case):
        return {k: poisoned(n) for k, n in self.mod().sizes(case).items()}

    def enqueue(self, ctx, case, dev, lists):
        args = (case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"], dev["points"],
                dev["point_status"], case["nimages"], dev["cam"], dev["cam_pair"], case["intrinsics"])
        kw = dict({k: case[k] for k in self.KW}, **{k: dev[k] for k in self.mod().OUTPUTS})
        if self.kind == "plain":
            return ctx.adjust_bundle_batch(*args, **kw)
        kw.update(loss=case["loss"], loss_scale=case["loss_scale"])
        if self.kind == "robust":
            return ctx.adjust_bundle_robust_batch(*args, **kw)
        if self.kind == "focal":
            return ctx.adjust_bundle_focal_batch(*args, case["group"], ngroups=case["ngroups"], **kw)
        return ctx.adjust_bundle_radial_batch(*args, case["group"], ngroups=case["ngroups"], radial=case.get("radial"),
                                              k0=case.get("k0"), **kw)

    def expected(self, case, lists):
        m = self.mod()
        e = getattr(m, dict(plain="expected_bundle", robust="expected_bundle", focal="expected_focal",
                            radial="expected_radial")[self.kind])(case)
        return {k: e[k] for k in m.OUTPUTS}


class FilterTracks(_Small):
    """misift_filter_tracks_batch on tracks of 2 to 17 views over 8 images (beyond 8 views a track holds duplicates) under
    an error gate of 2 px."""
    name = "filter_tracks_batch"

    def build(self, size):
        import filter_cases as FC
        return FC.lengths_case((2, 3, 4, 9, 17, 5, 2, 8), max_error=2.0)

    def uploads(self, case):
        import filter_cases as FC
        return FC.inputs(case)

    def outputs(self, case):
        import filter_cases as FC
        return {k: poisoned(n) for k, n in FC.sizes(case).items()}

    def enqueue(self, ctx, case, dev, lists):
        import filter_cases as FC
        ctx.filter_tracks_batch(case["max_tracks"], case["max_obs"], dev["track_offsets"], dev["obs"], dev["export_summary"],
                                dev["points"], dev["point_status"], case["nimages"], dev["cam"], dev["cam_pair"],
                                case["intrinsics"], **{k: case[k] for k in FC.ARGS}, **{k: dev[k] for k in FC.OUTPUTS})

    def expected(self, case, lists):
        import filter_cases as FC
        return _without(FC.expected_filter(case), "res")


class CorrespondTracks(_Small):
    """misift_correspond_tracks_batch: 40 tracks of A against the tracks B makes of every second record, shifted by 5."""
    name = "correspond_tracks_batch"
    KEYS = ("record_obs", "track_offsets", "export_summary")

    def build(self, size):
        import align_cases as AC
        return AC.correspond_cases()["shift +5"]

    def uploads(self, case):
        return {s + "_" + k: i32(case[s][k]) for s in "ab" for k in self.KEYS}

    def zeroed(self, case):
        return dict(case, **{s: dict(case[s], **{k: np.zeros_like(i32(case[s][k])) for k in self.KEYS}) for s in "ab"})

    def outputs(self, case):
        return dict(track_map=poisoned(case["a"]["max_tracks"]), summary=poisoned(8))

    def enqueue(self, ctx, case, dev, lists):
        A, B = case["a"], case["b"]
        ctx.correspond_tracks_batch(A["max_records"], dev["a_record_obs"], A["max_tracks"], A["max_obs"],
                                    dev["a_track_offsets"], dev["a_export_summary"], B["max_records"], dev["b_record_obs"],
                                    B["max_tracks"], B["max_obs"], dev["b_track_offsets"], dev["b_export_summary"],
                                    shift=case["shift"], track_map=dev["track_map"], summary=dev["summary"])

    def expected(self, case, lists):
        import align_cases as AC
        e = AC.expected_correspond(case)
        return dict(track_map=e["map"], summary=e["summary"])


class AlignPoints(_Small):
    """misift_align_points_batch on four entries that end in status 0, 1, 2 and 0, each with its own dst_first."""
    name = "align_points_batch"
    INPUTS = ("src", "dst", "map", "src_status", "dst_status", "count")

    def build(self, size):
        import align_cases as AC
        return AC.gpu_cases()["four entries"]

    def uploads(self, case):
        return {k: np.ascontiguousarray(case[k], f32 if k in ("src", "dst") else np.int32) for k in self.INPUTS
                if case.get(k) is not None}

    def outputs(self, case):
        n = len(case["ranges"])
        return dict(sim=poisoned(16 * n), align_cand=poisoned(n), align_inliers=poisoned(n), align_status=poisoned(n),
                    summary=poisoned(8), inlier=poisoned(len(case["map"])))

    def enqueue(self, ctx, case, dev, lists):
        ctx.align_points_batch(dev["src"], dev["dst"], dev["map"], case["ranges"], case["seeds"],
                               src_status=dev.get("src_status"), dst_status=dev.get("dst_status"), count=dev.get("count"),
                               count_stride=case["count_stride"], num_loops=case["num_loops"], thresh=case["thresh"],
                               min_inliers=case["min_inliers"], refit_loops=case["refit_loops"],
                               **{k: dev[k] for k in self.outputs(case)})

    def expected(self, case, lists):
        import align_cases as AC
        return _without(AC.expected_align(AC.variant(case)), "entries")


class TransformScene(_Small):
    """misift_transform_scene_batch under a status word of 0: unset and root cameras, failed points, tracks behind T."""
    name = "transform_scene_batch"

    def build(self, size):
        import align_cases as AC
        return AC.transform_case()

    def uploads(self, case):
        return dict(sim=np.ascontiguousarray(case["sim"], f32), sim_status=i32([case["sim_status"]]),
                    export_summary=i32(case["export_summary"]), points=np.ascontiguousarray(case["points"], f32),
                    point_status=i32(case["point_status"]), cam=np.ascontiguousarray(case["cam"], f32),
                    cam_pair=i32(case["cam_pair"]))

    def zeroed(self, case):
        return dict(Step.zeroed(self, case), sim_status=0)

    def outputs(self, case):
        return dict(points_out=poisoned(4 * case["max_tracks"]), cam_out=poisoned(12 * case["nimages"]))

    def enqueue(self, ctx, case, dev, lists):
        ctx.transform_scene_batch(dev["sim"], case["max_tracks"], dev["export_summary"], dev["points"], dev["point_status"],
                                  case["nimages"], dev["cam"], dev["cam_pair"], sim_status=dev["sim_status"],
                                  points_out=dev["points_out"], cam_out=dev["cam_out"])

    def expected(self, case, lists):
        import align_cases as AC
        return AC.expected_transform(case)


class MergeScenes(_Small):
    """misift_merge_scenes_batch on two windows of 63 and 65 tracks over one world, every optional output wanted."""
    name = "merge_scenes_batch"

    def build(self, size):
        import merge_cases as MC
        case = MC.gpu_cases()["T 63 65"]
        assert all(case["want"].values())
        return case

    def uploads(self, case):
        import merge_cases as MC
        ins = MC.inputs(case)
        ups = {s + "_" + k: v for s in "ab" for k, v in ins[s].items() if v is not None}
        ups["map"] = ins["map"]
        if ins["accept"] is not None:
            ups["accept"] = ins["accept"]
        return ups

    def zeroed(self, case):
        import merge_cases as MC
        ins = MC.inputs(case)
        out = dict(case, map=np.zeros_like(ins["map"]))
        for s in "ab":
            out[s] = dict(case[s], **{k: np.zeros_like(v) for k, v in ins[s].items() if v is not None})
        if ins["accept"] is not None:
            out["accept"] = np.zeros_like(ins["accept"])
        return out

    def outputs(self, case):
        import merge_cases as MC
        return {k: poisoned(n) for k, n in MC.sizes(case).items()}

    def enqueue(self, ctx, case, dev, lists):
        import merge_cases as MC
        from cudasift_amd import capi

        def scene(s):
            S = case[s]
            d = {k: dev.get(s + "_" + k) for k in capi.MERGE_SCENE_KEYS}
            return dict(d, max_tracks=S["max_tracks"], max_obs=S["max_obs"], nimages=S["nimages"],
                        max_records=int(S.get("max_records") or 0))

        ctx.merge_scenes_batch(scene("a"), scene("b"), dev["map"], case["nimages_out"], case["max_tracks_out"],
                               case["max_obs_out"], accept=dev.get("accept"), fshift_a=case["fshift_a"],
                               fshift_b=case["fshift_b"], rshift_a=case["rshift_a"], rshift_b=case["rshift_b"],
                               max_records_out=case["max_records_out"], **{k: dev[k] for k in MC.OUTPUTS})

    def expected(self, case, lists):
        import merge_cases as MC
        return _without(MC.expected_merge(case), "res")


class RecoverPosePlanar(_Small):
    """misift_recover_pose_planar_batch without F, min_inliers 4: frames of count -1, 0, 3 (below min_inliers), 65 and 257
    records of planted planar scenes, a frame that is in no entry, the entries not in frame order."""
    name = "recover_pose_planar_batch"
    temp = False
    SHAPE = ([40, 0, 3, 65, 30, 257], [5, 0, 3, 1, 2])
    KW = dict(min_inliers=4)

    def build(self, size):
        import pose_cases as PC
        import pose_planar_cases as PP
        sizes, sel = self.SHAPE
        fr, H, K = [], [], []
        for f, n in enumerate(sizes):
            s = PP.planar_scene(seed=300 + f, n=max(n, 8), baseline=0.5 if f % 2 else 0.1, off=0.1,
                                k2=PC.K_B if f % 2 else PC.K_A)
            fr.append(PC.records(s["xy"], 300 + f, fail=0.1 if n >= 10 else 0.0)[:n])
            H.append(s["H"])
            K.append(s["K8"])
        counts = [-1] + sizes[1:]
        recs, offs, _ = layout(fr, counts, False, min_stride=0, pad_error=-7.0)
        return dict(recs=recs, counts=i32(counts), offs=offs, sel=i32(sel), fr=fr,
                    H=np.ascontiguousarray(np.stack([H[f] for f in sel]), f32).reshape(-1, 9),
                    K=np.ascontiguousarray(np.stack([K[f] for f in sel]), f32).reshape(-1, 8))

    def uploads(self, case):
        return {k: case[k] for k in ("recs", "counts", "offs", "H")}

    def zeroed(self, case):
        return dict(Step.zeroed(self, case), fr=[np.zeros_like(p) for p in case["fr"]])

    def sizes_of(self, case):
        ns = len(case["sel"])
        return dict(model=ns, hf=2 * ns, pose=12 * ns, num_front=ns, votes=4 * ns, xyz=4 * len(case["recs"]),
                    pose_alt=12 * ns, plane=4 * ns)

    def outputs(self, case):
        return {k: poisoned(n) for k, n in self.sizes_of(case).items()}

    def enqueue(self, ctx, case, dev, lists):
        import pose_planar_cases as PP
        ctx.recover_pose_planar_batch(case["sel"], case["K"], dev["recs"], len(case["counts"]), dev["counts"], dev["H"],
                                      None, dev["offs"], 0, model=dev["model"], hf_counts=dev["hf"], pose=dev["pose"],
                                      num_front=dev["num_front"], votes=dev["votes"], xyz=dev["xyz"],
                                      pose_alt=dev["pose_alt"], plane=dev["plane"], min_score=GATES[0],
                                      max_ambiguity=GATES[1], **dict(PP.PARAMS, **self.KW))

    def expected(self, case, lists):
        import pose_planar_cases as PP
        sel, ns = case["sel"].tolist(), len(case["sel"])
        exp = [PP.expected_planar(case["fr"][f], int(case["counts"][f]), case["H"][i], None, case["K"][i], **self.KW)
               for i, f in enumerate(sel)]
        want = dict(model=np.array([e["model"] for e in exp], np.int32).view(np.uint32),
                    hf=np.stack([e["hf"] for e in exp]).reshape(-1).view(np.uint32))
        for k, n in self.sizes_of(case).items():
            if k not in want:
                want[k] = np.full(n, POISON_WORD, np.uint32).reshape(ns if k != "xyz" else len(case["recs"]), -1)
        for i, (f, e) in enumerate(zip(sel, exp)):
            if e["model"] <= 0:                                  # general or invalid: everything keeps the poison
                continue
            for k in ("pose", "pose_alt", "plane"):
                want[k][i] = e[k].astype(f32).view(np.uint32)
            want["num_front"][i] = e["num_front"]
            want["votes"][i] = e["votes"].view(np.uint32)
            want["xyz"][span(case["offs"], 0, f, max(int(case["counts"][f]), 0))] = e["xyz"].view(np.uint32)
        return {k: v.reshape(-1) for k, v in want.items()}


class MatchBatch(_Small):
    """misift_match_batch (the set-1 records written in place) under the context's default options, and
    misift_match_batch_i8 on descriptors quantised on the host: five frames of set 1, one of them empty and one of count
    -1, each against a frame of set 2; a set-2 frame below the 32 columns of the reference's sweep."""
    SHAPES = ([130, 33, 64, 0, 77, 20], [70, 129, 31, 64, 0])
    PAIRS = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 4), (5, 1)]

    def __init__(self, i8):
        super().__init__()
        self.i8, self.name = i8, "match_batch_i8" if i8 else "match_batch"

    def build(self, size):
        s1, s2 = self.SHAPES
        c1 = list(s1)
        c1[-1] = -1
        r1, o1, _ = layout(frames(s1, 31, self.i8), c1, False, min_stride=0, pad_error=0.0)
        r2, o2, _ = layout(frames(s2, 32, self.i8), s2, False, min_stride=0, pad_error=0.0)
        case = dict(recs1=r1, counts1=i32(c1), offs1=o1, recs2=r2, counts2=i32(s2), offs2=o2, pairs=i32(self.PAIRS))
        if self.i8:
            case.update(q1=quantize_np(r1["data"]).reshape(len(r1), 128), q2=quantize_np(r2["data"]).reshape(len(r2), 128))
        return case

    def uploads(self, case):
        return {k: case[k] for k in ("recs1", "counts1", "offs1", "recs2", "counts2", "offs2") +
                (("q1", "q2") if self.i8 else ())}

    def outputs(self, case):
        return {}

    def enqueue(self, ctx, case, dev, lists):
        n1, n2 = len(case["counts1"]), len(case["counts2"])
        if self.i8:
            return ctx.match_batch_i8(case["pairs"], dev["recs1"], dev["q1"], n1, dev["counts1"], dev["offs1"], 0,
                                      dev["recs2"], dev["q2"], n2, dev["counts2"], dev["offs2"], 0)
        ctx.match_batch(case["pairs"], dev["recs1"], n1, dev["counts1"], dev["offs1"], 0, dev["recs2"], n2,
                        dev["counts2"], dev["offs2"], 0)

    def expected(self, case, lists):
        from batch_util import MATCH_FIELDS, match_np
        exp = case["recs1"].copy()
        for f1, f2 in case["pairs"].tolist():
            n1, n2 = max(int(case["counts1"][f1]), 0), max(int(case["counts2"][f2]), 0)
            if n1 == 0 or n2 == 0:
                continue
            a, b = span(case["offs1"], 0, f1, n1), span(case["offs2"], 0, f2, n2)
            if self.i8:
                exp[a] = match_np(case["recs1"][a], case["q1"][a], case["recs2"][b], case["q2"][b])
                continue
            ref = case["recs1"][a].copy()
            orc().match(ref, n1, case["recs2"][b].copy(), n2, full=False, exact=False)
            for k in MATCH_FIELDS:
                exp[k][a] = ref[k]
        return dict(recs1=exp)


class QuantizeBatch(_Small):
    """misift_quantize_batch into a buffer that holds a pattern: the frames' records quantised, the rest kept."""
    name = "quantize_batch"
    temp = False
    takes_slot = False                                           # no host side beyond the launch
    SIZES = [130, 0, 33, 64, 20]

    def build(self, size):
        counts = list(self.SIZES)
        counts[-1] = -1
        recs, offs, _ = layout(frames(self.SIZES, 33, True), counts, False, min_stride=0, pad_error=0.0)
        recs["data"][::7, ::5] = np.random.default_rng(1).normal(0, 0.4, recs["data"][::7, ::5].shape)
        recs["data"][3, :4] = [np.nan, np.inf, -np.inf, 127.5 / 256]
        return dict(recs=recs, counts=i32(counts), offs=offs)

    def uploads(self, case):
        return {k: case[k] for k in ("recs", "counts", "offs")}

    def outputs(self, case):
        return dict(q=np.random.default_rng(9).integers(-128, 128, (len(case["recs"]) + 3, 128)).astype(np.int8))

    def enqueue(self, ctx, case, dev, lists):
        ctx.quantize_batch(dev["recs"], len(case["counts"]), dev["counts"], dev["offs"], 0, dev["q"])

    def expected(self, case, lists):
        q = self.outputs(case)["q"]
        for f, c in enumerate(case["counts"].tolist()):
            sl = span(case["offs"], 0, f, max(c, 0))
            q[sl] = quantize_np(case["recs"]["data"][sl])
        return dict(q=q)


class ScoreFundamental(_Small):
    """misift_score_fundamental_batch on the frames and the start matrices of the improve step: match_error of the
    records is written in place."""
    name = "score_fundamental_batch"
    temp = False

    def build(self, size):
        return step("improve_fundamental_batch").case("small")

    def uploads(self, case):
        return {k: case[k] for k in ("recs", "counts", "offs", "F")}

    def outputs(self, case):
        return dict(num_fit=poisoned(len(case["sel"])))

    def enqueue(self, ctx, case, dev, lists):
        ctx.score_fundamental_batch(case["sel"], dev["recs"], len(case["counts"]), dev["counts"], dev["F"], dev["offs"], 0,
                                    num_fit=dev["num_fit"], min_score=GATES[0], max_ambiguity=GATES[1], thresh=1.0)

    def expected(self, case, lists):
        from test_fundamental_cpu import expected_score
        want, fit = case["recs"].copy(), np.zeros(len(case["sel"]), np.int32)
        for i, f in enumerate(case["sel"].tolist()):
            n = int(case["counts"][f])
            sl = span(case["offs"], 0, f, max(n, 0))
            want[sl], fit[i] = expected_score(case["recs"][sl], n, case["F"][i], *GATES, 1.0)
        return dict(recs=want, num_fit=fit)


class UndistortObs(_Small):
    """misift_undistort_obs_batch out of place: 257 of 300 slots over five images in three groups and one in none."""
    name = "undistort_obs_batch"
    temp = False

    def build(self, size):
        import bundle_radial_cases as BD
        from test_bundle_radial_cpu import _words
        return dict(BD.undistort_case(257), words=np.ascontiguousarray(_words([0.07, -0.11, 0.0], BD.HELD), np.uint32))

    def uploads(self, case):
        return dict(obs=np.ascontiguousarray(case["obs"][:case["max_obs"]]), export_summary=i32(case["export_summary"]),
                    words=case["words"])

    def outputs(self, case):
        return dict(obs_out=poisoned(4 * case["max_obs"]))

    def enqueue(self, ctx, case, dev, lists):
        ctx.undistort_obs_batch(case["max_obs"], dev["obs"], dev["export_summary"], case["nimages"], case["intrinsics"],
                                case["group"], dev["words"], ngroups=case["ngroups"], obs_out=dev["obs_out"])

    def expected(self, case, lists):
        import bundle_radial_cases as BD
        return dict(obs_out=BD.expected_undistort(case, case["obs"], case["words"]))


# ---- the tables

@functools.lru_cache(maxsize=None)
def stream_table():
    """table() and, at `small` only, the calls it does not hold: what the caller-stream tests run (stream_util.py)."""
    return table() + (SelectStep(), Bundle("plain"), Bundle("robust"), Bundle("focal"), Bundle("radial"), FilterTracks(),
                      CorrespondTracks(), AlignPoints(), TransformScene(), MergeScenes(), RecoverPosePlanar(),
                      MatchBatch(False), QuantizeBatch(), MatchBatch(True), ScoreFundamental(), UndistortObs())


@functools.lru_cache(maxsize=None)
def table():
    """The steps in the order of the issue's table; built once, their cases and expected bytes cached inside."""
    return (MatchPairs(), MatchPairsI8(), Guided("guided"), Guided("epipolar"), LinkTracks(), ExportTracks(), LinkPoses(),
            Triangulate(), Refine(), Resect(), RecoverPose(), ImproveFundamental(), FindFundamental(), FindHomography())


def step(name):
    return {s.name: s for s in stream_table()}[name]

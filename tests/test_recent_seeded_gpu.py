"""K20 rw rows (recent.hip) on seeded engine state: one engine, one rollover, every case a series of
its own (tests/seeded.py).  The engine's rows must equal the CPU oracle's and a reference that
shares no code with either (tests/recent_ref.py: list slices + sorted() + Fraction ranks + integer
halves), byte for byte, and recents() the reference's integers.

The seeded window of windowSizeInIntervals = 31 holds 32 buckets (entries 0 .. 31, 31 the newest);
a span is at most windowSizeInIntervals, so the spans [1, 6, 31] leave entry 0 outside every span:
that is where the "old load" and the out-of-span decoys of the largest span go."""
import collections
import copy
import random

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import recent_ref as R  # noqa: E402
import seeded as S  # noqa: E402

CAP = 8                # bucketCellCapacity: samples in the inline cell, the rest in the spill list
GROUP_MAX = 512        # recent.hip RW_GROUP_MAX: samples of the largest span a 32-lane group sorts
GROUP_WIN = 32         # recent.hip RW_GROUP_WIN: window buckets a group covers; longer windows: block pass
SPANS = [1, 6, 31]
PCTS = [0.001, 1, 50, 75, 90, 95, 99, 99.999]
QS = [1, 1000, 50000, 75000, 90000, 95000, 99000, 99999]
NAN = S.ELAPSED_NAN
TILE_NS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513]


class RwSeeded(S.Seeded):
    """Seeded with the rw stream on, on both sides (and wp as well when `wp` lists percentiles)."""

    def __init__(self, C, *a, spans=SPANS, pcts=PCTS, wp=None, **kw):
        self.rw, self.wp = [], []
        C = copy.deepcopy(C)
        C["gpu"]["recentWindows"] = {"buckets": list(spans), "percentiles": list(pcts)}
        if wp:
            C["gpu"]["windowPercentiles"] = list(wp)
        self.extra = ("rw", "wp") if wp else ("rw",)
        super().__init__(C, *a, **kw)

    def _seed_oracle(self):
        from apmbackend_amd.utils.config import recent_windows, window_percentiles
        super()._seed_oracle()
        rw = recent_windows(self.C)
        self.so.emit_recent = self.rw.append
        self.so.recent_buckets = rw["buckets"]
        self.so.recent_percentiles = rw["percentiles"]
        if "wp" in self.extra:
            self.so.emit_pct = self.wp.append
            self.so.percentiles = window_percentiles(self.C)

    def _seed_engine(self):
        from apmbackend_amd.models import pipeline
        real = pipeline.APMEngine
        extra = self.extra
        pipeline.APMEngine = lambda C, outputs=(): real(C, outputs=tuple(outputs) + extra)
        try:
            super()._seed_engine()
        finally:
            pipeline.APMEngine = real


def entries_of(C, buckets, key):
    """The window's bucket lists of a series, oldest first."""
    return [list(buckets.get(key, {}).get(b, [])) for b in S.window_labels(C)]


def reference(C, order, buckets, spans, qs):
    """(rows, per series id the integers per span or None) of the first rollover from the case table alone."""
    edge_ts = (S.LATEST + 1 - S.stats_settings(C)[2] - 1) * 10000
    rows, ints = [], []
    for key in order:
        if key not in buckets:
            ints.append(None)
            continue
        e = entries_of(C, buckets, key)
        ints.append(R.series_ints(e, spans, qs))
        rows += R.rows(edge_ts, key[0], key[1], e, spans, qs)
    return rows, ints


def check(sd, order, buckets, spans, qs, names):
    want, ints = reference(sd.C, order, buckets, spans, qs)
    sd.step()
    got = sd.eng.take("rw")
    assert sd.rw == want, "oracle and reference differ: " + str(S.first_difference(sd.rw, want, lambda i: ""))
    diff = S.first_difference(got, want, lambda i: want[i].split("|")[3] if i < len(want) else "")
    assert diff is None, "rw rows: " + diff
    sd.eng.eng.flush()
    dev = sd.eng.eng.recents()
    assert len(dev) >= len(order)
    for i, w in enumerate(ints):
        if w is None:
            assert dev[i] is None, f"series {i} ({names[i]}): records {dev[i]}, want none"
            continue
        assert dev[i] is not None and len(dev[i]) == len(spans), f"series {i} ({names[i]}): {dev[i]}"
        for k, (m, nan, total, sums), (gm, gn, gt, gs) in zip(spans, w, dev[i]):
            assert (gm, gn, gt) == (m, nan, total), f"series {i} ({names[i]}) span {k}: {gm, gn, gt}, want {m, nan, total}"
            assert list(gs) == sums, f"series {i} ({names[i]}) span {k}: sums {list(gs)}, want {sums}"
    return want


class Table:
    """Case builder: samples by window entry counted from the newest (0 = newest, n_win - 1 = oldest)."""

    def __init__(self, C):
        self.C = C
        self.labels = S.window_labels(C)
        self.order, self.buckets, self.names, self.sizes = [], {}, [], []

    def add(self, name, by_age, decoys=True):
        """by_age: {entries back from the newest: samples}."""
        b = collections.OrderedDict()
        for age in sorted(by_age, reverse=True):
            b[self.labels[len(self.labels) - 1 - age]] = list(by_age[age])
        if decoys:
            b = S.with_decoys(b, self.labels, len(self.order))
        return S.add_series(self.order, self.buckets, self.names, self.sizes, name, b)

    def over(self, vals, ages):
        """vals dealt evenly over the entries `ages` (newest first), the first of them getting the rest."""
        ages = list(ages)
        out = {a: [] for a in ages}
        for i, v in enumerate(vals):
            out[ages[i % len(ages)]].append(v)
        return out

    def inactive(self, name):
        self.order.append(S.key(name)); self.names.append(name); self.sizes.append(0)

    def pad_even(self):
        if len(self.order) % 2:
            self.add(f"pad{len(self.order)}", {0: [9]})


def case_table(C, spans=SPANS):
    T = Table(C)
    n_win = len(T.labels)
    kmax = min(spans[-1], n_win)
    out_age = kmax if kmax < n_win else None    # the newest entry outside every span (None: the span is the window)
    rng = random.Random(2020)
    V = lambda n: S._values(rng, n)

    def outside(vals):
        return {out_age: list(vals)} if out_age is not None else {}

    # tile boundary: the largest group-eligible span's sample count on both sides of every tier
    for n in TILE_NS:
        d = T.over(V(n), range(kmax))
        d.update(outside([1_900_000_000 + n, -77]))
        T.add(f"tile{n}", d)
    for n in (32, 33, 512, 513):              # the same counts in the newest bucket alone (spilled)
        T.add(f"newest{n}", {0: V(n)})
    # span edge: entry n_win - k is in, a distinct value in entry n_win - k - 1 is out
    for k in spans:
        kk = min(k, n_win)
        d = {kk - 1: [1000 + k]}
        if kk < n_win:
            d[kk] = [-(5000 + k)]
        T.add(f"edge{k}", d)
        d = {kk - 1: V(11) + [1000 + k]}
        if kk < n_win:
            d[kk] = V(10) + [-(5000 + k)]
        T.add(f"edge{k}_spilled", d)
    # prefix hazard: the larger values in the newest bucket, the smaller ones in the next five -- a
    # padded write-back of the first sort would replace them
    for n1, n6 in ((33, 60), (65, 120), (129, 250)):
        d = {0: [1_000_000 + i for i in range(n1)]}
        d.update(T.over([10 + i for i in range(n6 - n1)], range(1, 6)))
        T.add(f"hazard{n1}_{n6}", d)
        d = {0: [1_000_000 + i for i in range(n1)]}
        d.update(T.over([10 + i for i in range(n6 - n1)], range(1, 6)))
        if kmax > 6:
            d.update(T.over([-500 - i for i in range(40)], range(6, kmax)))
        T.add(f"hazard{n1}_{n6}_more", d)
    # old load: 20 000 samples outside every span, three inside (the span's own count decides)
    T.pad_even()
    if out_age is not None:
        T.add("old_load", {out_age: V(20000), 2: [5, 6], 0: [7]})
        T.add("old_load_neighbour", {0: [1, 2, 3]})
    T.add("newest_600", {0: V(600), 3: [4]})
    T.add("newest_600_neighbour", {0: [8]})
    # unequal halves of one wave (ids 2k, 2k + 1)
    T.pad_even()
    T.add("empty_spans", outside([3, 4]) or {kmax - 1: [3]})
    T.add("full_tile", T.over(V(512), range(kmax)))
    T.add("group_a", T.over(V(40), range(6)))
    T.add("deferred_b", T.over(V(700), range(6)))
    T.add("deferred_a", T.over(V(701), range(3)))
    T.add("group_b", T.over(V(41), range(3)))
    T.add("before_gap", {0: [1, 2, 3]})
    T.inactive("inactive")
    b = collections.OrderedDict({T.labels[len(T.order) % n_win]: []})
    S.add_series(T.order, T.buckets, T.names, T.sizes, "count0", S.with_decoys(b, T.labels, len(T.order)))
    T.add("after_gap", {1: [4, 5, 6] * 5})
    # spill
    T.add("spill8", {0: V(8)})
    T.add("spill9", {0: V(9)})
    T.add("spill8_older", {4: V(8), 0: [1]})
    T.add("spill9_older", {4: V(9), 0: [1]})
    d = {1: V(20)}
    d.update(outside(V(30)))
    T.add("spill_in_and_out", d)
    T.pad_even()
    T.add("spills_even", {0: V(12), 1: V(9), 3: V(30), 5: V(10), 7: V(64)})
    T.add("spills_odd", {0: V(9), 2: V(17), 4: V(100), 5: V(9), 20: V(33)})
    # NaN
    T.add("nan_inline", {0: [5, NAN, 7]})
    T.add("nan_spilled", {0: V(10) + [NAN] + V(9) + [NAN]})
    T.add("nan_inside_only", {0: [NAN, 3], 7: [1, 2]})
    T.add("nan_outside_1", {0: [3, 4], 2: [NAN, 9]})          # span 1: nan 0, spans 6 and 31: nan 1
    if out_age is not None:
        T.add("nan_outside_all", {0: [3, 4], out_age: [NAN, 9]})  # nan 0 in every span, the window NaN-poisoned
    T.add("all_nan_span", {0: [NAN] * 3, 8: [11]})            # span 1 and 6: m 0, nan 3
    T.add("all_nan_spilled", {0: [NAN] * 12})
    T.add("nan_block", {0: V(600) + [NAN] * 2 + V(50)})
    # values
    T.add("int32_max_x513", {0: [S.INT32_MAX] * 513})
    T.add("int32_max_x512", T.over([S.INT32_MAX] * 512, range(6)))
    T.add("minus_one_zero", {0: [-1, 0]})
    T.add("extremes", {0: [NAN + 1], 1: [S.INT32_MAX]})
    T.add("most_negative", {0: [NAN + 1] * 40})
    T.add("all_equal", T.over([777] * 40, range(kmax)))
    # quiet: every older entry holds samples, the newest six none
    T.add("quiet", {a: [100 + a, 200 + a] for a in range(6, n_win)})
    T.order.append(S.TRIGGER); T.names.append("trigger"); T.sizes.append(0)
    T.add("last_id_spills", {0: V(100)})
    if len(T.order) % 2 == 0:
        T.add("odd_tail", {0: V(20)})
    assert len(T.order) % 2 == 1, "the last wave's upper half must be past n_series"
    return T.order, T.buckets, T.names


def test_constants_are_the_kernels():
    from apmbackend_amd import _native
    N = _native.load(build_if_missing=False)
    assert N.recent_group_max() == GROUP_MAX == S.H2_TILE and N.recent_group_win() == GROUP_WIN == S.HW


def test_one_rollover_all_cases():
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    assert len(S.window_labels(C)) == 32 == GROUP_WIN
    order, buckets, names = case_table(C)
    sd = RwSeeded(C, order, buckets)
    want = check(sd, order, buckets, SPANS, QS, names)
    by = collections.defaultdict(list)
    for r in want:
        by[r.split("|")[3]].append(r.split("|", 4)[4])
    lab = [R.label(q) for q in QS]
    pairs = lambda v: ",".join(f"{p}:{v}" for p in lab)
    # span edge
    assert by["S:edge1"][0] == f"1|1|0|1001|{pairs(1001)}" and by["S:edge1"][1].startswith("6|2|0|-4000|")
    assert by["S:edge6"][0] == "1|0|0|0|" and by["S:edge6"][1] == f"6|1|0|1006|{pairs(1006)}"
    assert by["S:edge31"][1] == "6|0|0|0|" and by["S:edge31"][2] == f"31|1|0|1031|{pairs(1031)}"
    # prefix hazard: the 6-bucket minimum is one of the small values
    for n1, n6 in ((33, 60), (65, 120), (129, 250)):
        r1, r6, _r31 = by[f"S:hazard{n1}_{n6}"]
        assert r1.startswith(f"1|{n1}|0|") and r6.startswith(f"6|{n6}|0|")
        # (0.001 % of more than one sample reads the two smallest: their mean)
        assert r1.split("|")[4].startswith("0.001:1000000.5,") and r6.split("|")[4].startswith("0.001:10.5,")
    # old load, the block path, halves
    assert [r.split("|")[:3] for r in by["S:old_load"]] == [["1", "1", "0"], ["6", "3", "0"], ["31", "3", "0"]]
    assert by["S:old_load"][2].startswith("31|3|0|18|")
    assert by["S:newest_600"][0].startswith("1|600|0|") and by["S:newest_600"][1].startswith("6|601|0|")
    assert by["S:empty_spans"] == ["1|0|0|0|", "6|0|0|0|", "31|0|0|0|"]
    assert by["S:full_tile"][2].startswith("31|512|0|")
    # NaN
    assert by["S:nan_outside_1"][0].startswith("1|2|0|7|") and by["S:nan_outside_1"][1].startswith("6|3|1|16|")
    assert [r.split("|")[:3] for r in by["S:nan_outside_all"]] == [["1", "2", "0"], ["6", "2", "0"], ["31", "2", "0"]]
    assert by["S:all_nan_span"] == ["1|0|3|0|", "6|0|3|0|", f"31|1|3|11|{pairs(11)}"]
    assert by["S:all_nan_spilled"] == ["1|0|12|0|", "6|0|12|0|", "31|0|12|0|"]
    assert by["S:nan_block"][0].startswith("1|650|2|")
    # values
    assert by["S:int32_max_x513"][0] == f"1|513|0|{513 * S.INT32_MAX}|{pairs(S.INT32_MAX)}"
    assert by["S:int32_max_x512"][2] == f"31|512|0|{512 * S.INT32_MAX}|{pairs(S.INT32_MAX)}"
    assert by["S:minus_one_zero"][0] == "1|2|0|-1|0.001:-0.5,1:-0.5,50:-1,75:0,90:0,95:0,99:0,99.999:0"
    assert by["S:extremes"][1] == ("6|2|0|0|0.001:0,1:0,50:-2147483647,75:2147483647,90:2147483647,95:2147483647,"
                                   "99:2147483647,99.999:2147483647")
    assert by["S:most_negative"][0] == f"1|40|0|{-40 * S.INT32_MAX}|{pairs(-S.INT32_MAX)}"
    # quiet: two m == 0 rows and a normal 31-bucket row
    assert by["S:quiet"][:2] == ["1|0|0|0|", "6|0|0|0|"] and by["S:quiet"][2].startswith("31|50|0|")
    assert "S:count0" not in by and "S:inactive" not in by and "S:trigger" not in by
    # the st / fs rows are what an engine without the stream prints
    plain = S.Seeded(C, order, buckets, reference=False)
    plain.step()
    assert sd.eng.take("st") == plain.eng.take("st") == sd.st
    assert sd.eng.take("fs") == plain.eng.take("fs")
    assert plain.eng.take("rw") == [] and plain.eng.eng.recents() == []


def test_spans_one_and_six_alone():
    """The issue's hazard configuration itself, [1, 6]: entries older than six are outside every span."""
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    order, buckets, names = case_table(C, spans=[1, 6])
    sd = RwSeeded(C, order, buckets, spans=[1, 6], pcts=[50, 95, 99])
    want = check(sd, order, buckets, [1, 6], [50000, 95000, 99000], names)
    by = collections.defaultdict(list)
    for r in want:
        by[r.split("|")[3]].append(r.split("|", 4)[4])
    assert by["S:hazard33_60"][1].startswith("6|60|0|")
    assert by["S:old_load"][1].startswith("6|3|0|18|")


def test_consistency_with_wp():
    """Both streams on, the same percentiles, the span 31 and nothing in the window's oldest entry
    (a span is at most windowSizeInIntervals, one bucket short of the window): fields 5, 6 and 8 of
    every rw row are fields 5 to 7 of the series' wp row, and every wp row has its rw row."""
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    labels = S.window_labels(C)
    order, buckets, names, sizes = [], {}, [], []
    rng = random.Random(31)
    for n in TILE_NS + [1023, 1024, 1025, 20000]:
        vals = S._values(rng, n)
        if n in (33, 257, 1025):
            vals[n // 2] = NAN
        b = S.layout(vals, labels[1:], "spread", where=len(order))
        if n == 0:
            b[labels[3]] = []
        S.add_series(order, buckets, names, sizes, f"n{n}", S.with_decoys(b, labels, len(order)))
    S.add_series(order, buckets, names, sizes, "only_nan", S.with_decoys({labels[5]: [NAN] * 3}, labels, 1))
    sd = RwSeeded(C, order, buckets, spans=[31], pcts=PCTS, wp=PCTS)
    check(sd, order, buckets, [31], QS, names)
    rw = {tuple(r.split("|")[2:4]): r.split("|") for r in sd.rw}   # (check: the engine's rows are these)
    wp = [r.split("|") for r in sd.eng.take("wp")]
    assert [("|".join(f)) for f in wp] == sd.wp and len(wp) == len(order) - 2   # (n = 0 and only NaN: no wp row)
    for f in wp:
        g = rw[(f[2], f[3])]
        assert g[4] == "31" and [g[5], g[6], g[8]] == [f[4], f[5], f[6]], (f, g)
    assert len(rw) == len(order) - 1                                             # (only NaN: an rw row, m = 0)


def test_long_window_takes_the_block_pass():
    """A window of windowSizeInIntervals = 33 (34 buckets): longer than a group's 32 lanes, so every
    series is selected by a block; spans [1, 33]."""
    C = S.seeded_cfg(window=33, buffer=6, cell_cap=CAP)
    labels = S.window_labels(C)
    assert len(labels) == 34 > GROUP_WIN
    T = Table(C)
    rng = random.Random(33)
    for n in (0, 1, 2, 32, 33, 511, 512, 513):
        d = T.over(S._values(rng, n), range(33))
        d[33] = [1_800_000_000 + n]                  # the oldest entry: outside both spans
        T.add(f"long{n}", d)
    T.add("long_newest", {0: S._values(rng, 40) + [NAN], 1: [3]})
    T.add("long_edge", {32: [1033], 33: [-5033]})
    T.add("long_quiet", {a: [a] for a in range(1, 34)})
    T.inactive("inactive")
    sd = RwSeeded(C, T.order, T.buckets, spans=[1, 33])
    want = check(sd, T.order, T.buckets, [1, 33], QS, T.names)
    by = collections.defaultdict(list)
    for r in want:
        by[r.split("|")[3]].append(r.split("|", 4)[4])
    assert by["S:long_edge"][0] == "1|0|0|0|" and by["S:long_edge"][1].startswith("33|1|0|1033|")
    assert by["S:long_quiet"][0] == "1|0|0|0|" and by["S:long_quiet"][1].startswith("33|32|0|")
    assert by["S:long513"][1].startswith("33|513|0|")
    assert len(want) == 2 * (len(T.order) - 1)


def test_window_shortened_by_a_reload_clips_both_paths():
    """The engine is built for 32 window buckets and the spans [1, 6, 31]; a reload to
    windowSizeInIntervals = 3 before the rollover leaves 4.  The spans 6 and 31 then read the whole
    window, in the group (the second one a prefix that is sorted already) and in the block pass, and
    print the configured k."""
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    T = Table(C)
    rng = random.Random(4)
    for n in (0, 1, 5, 33, 200, 512, 513, 700):
        d = T.over(S._values(rng, n), range(4))
        d[4] = [1_700_000_000 + n]                   # inside the window the engine was built for, outside the new one
        d[20] = [-123, 456]
        T.add(f"short{n}", d)
    T.add("short_newest", {0: S._values(rng, 600) + [NAN], 3: [7]})
    T.add("short_quiet", {3: [5, NAN], 2: [6]})
    T.add("short_gone", {9: [1, 2, 3]})              # samples older than the new window only: no row
    sd = RwSeeded(C, T.order, T.buckets)
    C3 = copy.deepcopy(sd.C)
    C3["streamCalcStats"]["windowSizeInIntervals"] = 3
    assert len(S.window_labels(C3)) == 4 and S.window_labels(C3)[-1] == S.window_labels(C)[-1]
    assert sd.eng.reload(copy.deepcopy(C3), gen=1) == []
    sd.so.window, sd.so.keep = 3, 3 + sd.so.buffer
    sd.C = C3
    want = check(sd, T.order, T.buckets, SPANS, QS, T.names)
    by = collections.defaultdict(list)
    for r in want:
        by[r.split("|")[3]].append(r.split("|", 4)[4])
    for n in (1, 5, 33, 200, 512, 513, 700):
        r1, r6, r31 = by[f"S:short{n}"]
        assert r6.startswith(f"6|{n}|0|") and r31.startswith(f"31|{n}|0|") and r6[2:] == r31[3:]
    assert by["S:short_newest"][0].startswith("1|600|1|") and by["S:short_newest"][2].startswith("31|601|1|")
    assert by["S:short_quiet"] == ["1|0|0|0|", by["S:short_quiet"][1], by["S:short_quiet"][2]]
    assert by["S:short_quiet"][2].startswith("31|2|1|11|")
    assert "S:short_gone" not in by and "S:short0" not in by

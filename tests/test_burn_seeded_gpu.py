"""K21 sb rows (burn.hip) on seeded engine state: one engine, one rollover, every case a series of
its own (tests/seeded.py).  The engine's rows must equal the CPU oracle's and a reference that
shares no code with either (tests/burn_ref.py: list slices + Fraction), byte for byte, and burns()
the reference's integers.

The seeded window of windowSizeInIntervals = 31 holds 32 buckets (entries 0 .. 31, 31 the newest).
The objectives: the default {T = 1000, q = 99000} (b = 1000), S:* services named in NAMED with their
own, and one service named with null.  The rules [1 bucket at 14.4, 6 buckets at 6], minSamples 20.
With b = 1000 and f = 14400 a set of 125 samples burns from 18 bad ones on (18 * 10^8 = 14400 * 125
* 1000) and not with 17; at f = 6000 from 8 on (7.5)."""
import collections
import copy

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import burn_ref as R  # noqa: E402
import seeded as S  # noqa: E402

CAP = 8                # bucketCellCapacity: samples in the inline cell, the rest in the spill list
GROUP_MAX = 4096       # burn.hip SB_GROUP_MAX: window samples a 32-lane group counts itself
NAN = S.ELAPSED_NAN
T, Q = 1000, 99000
RULES = [(1, 14400), (6, 6000)]
MIN_SAMPLES = 20
NAMED = {"S:named_fires": (50, 99900), "S:shared": (200, 90000), "S:negative_T": (0, 99000)}
OFF = "S:class0"


def burn_key(rules=RULES, min_samples=MIN_SAMPLES):
    services = {n: {"threshold": t, "target": q / 1000} for n, (t, q) in NAMED.items()}
    services[OFF] = None
    return {"default": {"threshold": T, "target": Q / 1000}, "services": services,
            "rules": [{"short": k, "factor": f / 1000} for k, f in rules], "minSamples": min_samples}


class SbSeeded(S.Seeded):
    """Seeded with the sb stream on, on both sides."""

    def __init__(self, C, *a, key=None, **kw):
        self.sb = []
        C = copy.deepcopy(C)
        C["gpu"]["sloBurn"] = key or burn_key()
        super().__init__(C, *a, **kw)

    def _seed_oracle(self):
        from apmbackend_amd.utils.config import slo_burn
        super()._seed_oracle()
        self.so.emit_burn = self.sb.append
        self.so.burn = slo_burn(self.C)

    def _seed_engine(self):
        from apmbackend_amd.models import pipeline
        real = pipeline.APMEngine
        pipeline.APMEngine = lambda C, outputs=(): real(C, outputs=tuple(outputs) + ("sb",))
        try:
            super()._seed_engine()
        finally:
            pipeline.APMEngine = real


def objective_of(service):
    if service == OFF:
        return None
    return NAMED.get(service, (T, Q))


def reference(C, order, buckets, rules, min_samples):
    """(rows, per series id the integers or None) of the first rollover from the case table alone."""
    edge_ts = (S.LATEST + 1 - S.stats_settings(C)[2] - 1) * 10000
    labels = S.window_labels(C)
    rows, ints = [], []
    for key in order:
        obj = objective_of(key[1])
        if key not in buckets or obj is None:
            ints.append(None)
            continue
        e = [list(buckets[key].get(b, [])) for b in labels]
        ints.append(R.series_ints(e, obj[0], obj[1], rules, min_samples))
        r = R.row(edge_ts, key[0], key[1], e, obj[0], obj[1], rules, min_samples)
        if r is not None:
            rows.append(r)
    return rows, ints


def check(sd, order, buckets, names, rules=RULES, min_samples=MIN_SAMPLES):
    want, ints = reference(sd.C, order, buckets, rules, min_samples)
    sd.step()
    got = sd.eng.take("sb")
    assert sd.sb == want, "oracle and reference differ: " + str(S.first_difference(sd.sb, want, lambda i: ""))
    diff = S.first_difference(got, want, lambda i: want[i].split("|")[3] if i < len(want) else "")
    assert diff is None, "sb rows: " + diff
    sd.eng.eng.flush()
    dev = sd.eng.eng.burns()
    assert len(dev) >= len(order)
    for i, w in enumerate(ints):
        if w is None:
            assert dev[i] is None, f"series {i} ({names[i]}): record {dev[i]}, want none"
            continue
        assert dev[i] is not None, f"series {i} ({names[i]}): no record"
        m, bad, nan, per, mask = dev[i]
        assert (m, bad, nan, [tuple(p) for p in per], mask) == w, f"series {i} ({names[i]}): {dev[i]}, want {w}"
    assert sd.eng.metrics()["sb_rows"] == len(want)
    return want, ints


class Table:
    """Case builder: samples by window entry counted from the newest (0 = newest, n_win - 1 = oldest)."""

    def __init__(self, C):
        self.C = C
        self.labels = S.window_labels(C)
        self.order, self.buckets, self.names, self.sizes = [], {}, [], []

    def add(self, name, by_age, decoys=True, server=None):
        b = collections.OrderedDict()
        for age in sorted(by_age, reverse=True):
            b[self.labels[len(self.labels) - 1 - age]] = list(by_age[age])
        if decoys:
            b = S.with_decoys(b, self.labels, len(self.order))
        if server is None:
            return S.add_series(self.order, self.buckets, self.names, self.sizes, name, b)
        k = (server, S.key(name)[1])                 # the same service on another server
        self.order.append(k); self.buckets[k] = b; self.names.append(f"{server}/{name}"); self.sizes.append(0)
        return k

    def inactive(self, name):
        self.order.append(S.key(name)); self.names.append(name); self.sizes.append(0)

    def pad_even(self):
        if len(self.order) % 2:
            self.add(f"pad{len(self.order)}", {0: [9]})


def mix(n, bad, t=T, good=None):
    """n samples, `bad` of them above t (the first ones)."""
    return [t + 1 + i for i in range(bad)] + [(t - i % 7) if good is None else good for i in range(n - bad)]


def case_table(C, rules=RULES):
    Tb = Table(C)
    n_win = len(Tb.labels)
    k1, k6 = (min(k, n_win) for k, _f in rules)
    # values at the threshold: T is good, T + 1 bad, negative good, NaN apart
    Tb.add("at_T", {0: [T] * 20})                                       # m 20, bad 0: nothing fires
    Tb.add("at_T_plus_1", {0: [T + 1] * 20})                            # all bad: both rules
    Tb.add("negatives", {0: [-1, -50, -S.INT32_MAX] * 7})               # good
    Tb.add("nans", {0: [NAN] * 5 + [T + 1] * 20 + [NAN]})               # nan 6, m 20
    Tb.add("nans_only", {0: [NAN] * 30})                                # m 0
    Tb.add("nan_below_min", {0: [NAN] * 10 + [T + 1] * 19})             # m 19 < 20 with 29 samples
    Tb.add("negative_T", {0: [0] * 10 + [1] * 10 + [-3] * 5})           # T = 0 (named): 10 of 25 bad
    # span edges: bad samples just inside the span fire it, just outside they do not
    Tb.add("edge1_in", {k1 - 1: mix(40, 40), k1: mix(40, 0)})
    Tb.add("edge1_out", {k1 - 1: mix(40, 0), k1: mix(40, 40)})          # rule 1 misses; rule 2's span has them
    Tb.add("edge6_in", {k6 - 1: mix(40, 40), 0: mix(20, 0)})
    if k6 < n_win:
        Tb.add("edge6_out", {k6: mix(40, 40), 0: mix(20, 0)})           # the window burns, no span does
    # spill: a bucket of 9 (one spilled sample, the bad one), and a spilled run in the span's first entry
    Tb.add("spill9_bad_last", {0: mix(8, 0) + [T + 1], 1: mix(30, 0)})
    Tb.add("spill_first_entry", {k6 - 1: mix(8, 0) + [T + 5] * 30, 0: mix(20, 0)})
    Tb.add("spill_outside", {k6 if k6 < n_win else n_win - 1: mix(8, 0) + [T + 5] * 30, 0: mix(20, 0)})
    Tb.add("spill_newest", {0: mix(8, 0) + [T + 5] * 30 + [NAN] * 3})
    # the inequality met exactly and missed by one, in each window separately (q 99000, f 14400)
    Tb.add("exact_both", {0: mix(125, 18)})                             # window = span: 18 of 125
    Tb.add("miss_both", {0: mix(125, 17)})
    # span met exactly (18 / 125), the window met exactly too: 36 of 250
    Tb.add("exact_long_exact_short", {0: mix(125, 18), 9: mix(125, 18)})
    Tb.add("miss_long_exact_short", {0: mix(125, 18), 9: mix(125, 17)})   # window 35 / 250: one short (rule 2 fires)
    Tb.add("exact_long_miss_short", {0: mix(125, 17), 9: mix(125, 19)})   # span 17 / 125
    # rule 2 alone at its own edge: f 6000 needs 7.5 -> 8 of 125; the 6-bucket span and the window
    Tb.add("rule2_exact", {3: mix(100, 6), 0: mix(100, 6)})             # 12 / 200 = 6.0 % = 6 x 1 %: fires rule 2 only
    Tb.add("rule2_miss", {3: mix(100, 6), 0: mix(100, 5)})              # 11 / 200: nothing
    # long burns and short does not, and the reverse: no row
    Tb.add("long_only", {10: mix(100, 100), 0: mix(100, 0)})
    Tb.add("short_only", {10: mix(3000, 0), 0: mix(25, 25)})            # 25 / 3025 = 0.83 %: below 6 x 1 %
    # two rules, only the second fires
    Tb.add("second_only", {0: mix(100, 10), 4: mix(100, 10)})           # 10 %: 10 x, below 14.4, above 6
    # minSamples
    Tb.add("min_samples_19", {0: mix(19, 19)})
    Tb.add("min_samples_20", {0: mix(20, 20)})
    Tb.add("span_below_min", {0: mix(19, 19), 8: mix(50, 50)})          # the window has 69, both spans 19
    # classes
    Tb.add("class0", {0: mix(50, 50)})
    Tb.add("named_fires", {0: [51] * 2 + [50] * 98})                    # T 50, q 99900: 2 % / 0.1 % = 20 x
    Tb.add("default_next_to_named", {0: [51] * 2 + [50] * 98})          # the same samples under the default: good
    Tb.add("shared", {0: [201] * 30})                                   # both servers of one service share a class
    Tb.add("shared", {0: [200] * 30 + [201] * 30}, server="jvm01")      # 50 % / 10 % = 5 x: below both factors
    # empty window
    b = collections.OrderedDict({Tb.labels[3]: []})
    S.add_series(Tb.order, Tb.buckets, Tb.names, Tb.sizes, "count0", S.with_decoys(b, Tb.labels, len(Tb.order)))
    Tb.inactive("inactive")
    # above the group limit: the block pass, next to a group series in the same wave
    Tb.pad_even()
    Tb.add("big", {0: mix(3000, 600), 7: mix(GROUP_MAX - 3000 + 1, 0) + [NAN] * 4})
    Tb.add("big_neighbour", {0: mix(30, 30)})
    Tb.add("group_limit", {0: mix(96, 96), 7: mix(GROUP_MAX - 96, 0)})  # exactly SB_GROUP_MAX samples: the group
    Tb.add("big_quiet", {20: mix(GROUP_MAX + 50, 4000)})                # deferred, the window burns, no span does
    # two series in one wave where only one has work
    Tb.pad_even()
    Tb.add("class0", {0: mix(40, 40)}, server="jvm02")
    Tb.add("works_next_to_class0", {0: mix(40, 40)})
    Tb.add("works_next_to_inactive", {0: mix(40, 40), 2: mix(9, 9)})
    Tb.inactive("inactive2")
    Tb.order.append(S.TRIGGER); Tb.names.append("trigger"); Tb.sizes.append(0)
    Tb.add("last_id_spills", {0: mix(100, 50)})
    if len(Tb.order) % 2 == 0:
        Tb.add("odd_tail", {0: mix(20, 20)})
    assert len(Tb.order) % 2 == 1, "the last wave's upper half must be past n_series"
    return Tb


def by_service(rows):
    by = collections.defaultdict(list)
    for r in rows:
        by[(r.split("|")[2], r.split("|")[3])].append(r.split("|", 4)[4])
    return by


def test_constants_are_the_kernels():
    from apmbackend_amd import _native
    N = _native.load(build_if_missing=False)
    assert N.burn_group_max() == GROUP_MAX == N.slo_group_max()


def test_one_rollover_all_cases():
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    assert len(S.window_labels(C)) == 32
    Tb = case_table(C)
    sd = SbSeeded(C, Tb.order, Tb.buckets)
    want, ints = check(sd, Tb.order, Tb.buckets, Tb.names)
    by = by_service(want)
    J = S.SERVER
    g = lambda *groups: ",".join(groups)
    one = lambda name: by[(J, "S:" + name)]
    # threshold, negatives, NaN
    assert one("at_T") == [] and one("negatives") == [] and one("nans_only") == [] and one("nan_below_min") == []
    assert one("at_T_plus_1") == [f"{T}|{Q}|20|20|0|" + g("1:14400:20:20:1", "6:6000:20:20:1")]
    assert one("nans") == [f"{T}|{Q}|20|20|6|" + g("1:14400:20:20:1", "6:6000:20:20:1")]
    assert one("negative_T") == ["0|99000|25|10|0|" + g("1:14400:25:10:1", "6:6000:25:10:1")]
    # span edges
    assert one("edge1_in") == [f"{T}|{Q}|80|40|0|" + g("1:14400:40:40:1", "6:6000:80:40:1")]
    assert one("edge1_out") == [f"{T}|{Q}|80|40|0|" + g("1:14400:40:0:0", "6:6000:80:40:1")]
    assert one("edge6_in") == [f"{T}|{Q}|60|40|0|" + g("1:14400:20:0:0", "6:6000:60:40:1")]
    assert one("edge6_out") == []
    # spill
    assert one("spill9_bad_last") == [] and one("spill_outside") == []
    assert one("spill_first_entry") == [f"{T}|{Q}|58|30|0|" + g("1:14400:20:0:0", "6:6000:58:30:1")]
    assert one("spill_newest") == [f"{T}|{Q}|38|30|3|" + g("1:14400:38:30:1", "6:6000:38:30:1")]
    # the inequality at its edge
    assert one("exact_both") == [f"{T}|{Q}|125|18|0|" + g("1:14400:125:18:1", "6:6000:125:18:1")]
    assert one("miss_both") == [f"{T}|{Q}|125|17|0|" + g("1:14400:125:17:0", "6:6000:125:17:1")]
    assert one("exact_long_exact_short") == [f"{T}|{Q}|250|36|0|" + g("1:14400:125:18:1", "6:6000:125:18:1")]
    assert one("miss_long_exact_short") == [f"{T}|{Q}|250|35|0|" + g("1:14400:125:18:0", "6:6000:125:18:1")]
    assert one("exact_long_miss_short") == [f"{T}|{Q}|250|36|0|" + g("1:14400:125:17:0", "6:6000:125:17:1")]
    assert one("rule2_exact") == [f"{T}|{Q}|200|12|0|" + g("1:14400:100:6:0", "6:6000:200:12:1")]
    assert one("rule2_miss") == []
    assert one("long_only") == [] and one("short_only") == []
    assert one("second_only") == [f"{T}|{Q}|200|20|0|" + g("1:14400:100:10:0", "6:6000:200:20:1")]
    # minSamples
    assert one("min_samples_19") == [] and one("span_below_min") == []
    assert one("min_samples_20") == [f"{T}|{Q}|20|20|0|" + g("1:14400:20:20:1", "6:6000:20:20:1")]
    # classes
    assert (J, OFF) not in by and ("jvm02", OFF) not in by
    assert one("named_fires") == ["50|99900|100|2|0|" + g("1:14400:100:2:1", "6:6000:100:2:1")]
    assert one("default_next_to_named") == []
    assert one("shared") == ["200|90000|30|30|0|" + g("1:14400:30:30:0", "6:6000:30:30:1")]
    assert by[("jvm01", "S:shared")] == []
    assert one("count0") == [] and one("inactive") == []
    # block pass and its neighbours
    assert one("big") == [f"{T}|{Q}|{GROUP_MAX + 1}|600|4|" + g("1:14400:3000:600:1", "6:6000:3000:600:1")]
    assert len(one("big_neighbour")) == 1 and one("group_limit") == [] and one("big_quiet") == []
    assert one("works_next_to_class0") and one("works_next_to_inactive") and one("last_id_spills")
    # what burns() reports for series that print nothing
    idx = {k: i for i, k in enumerate(Tb.order)}
    assert ints[idx[(J, "S:count0")]] == (0, 0, 0, [(0, 0), (0, 0)], 0)
    assert ints[idx[(J, OFF)]] is None and ints[idx[(J, "S:inactive")]] is None
    assert ints[idx[(J, "S:long_only")]] == (200, 100, 0, [(100, 0), (100, 0)], 0)
    assert ints[idx[(J, "S:big_quiet")]][:3] == (GROUP_MAX + 50, 4000, 0)
    assert ints[idx[(J, "S:group_limit")]] == (GROUP_MAX, 96, 0, [(96, 96), (96, 96)], 0)
    # the st / fs rows are what an engine without the stream prints
    plain = S.Seeded(C, Tb.order, Tb.buckets, reference=False)
    plain.step()
    assert sd.eng.take("st") == plain.eng.take("st") == sd.st
    assert sd.eng.take("fs") == plain.eng.take("fs")
    assert plain.eng.take("sb") == [] and plain.eng.eng.burns() == []


@pytest.mark.parametrize("window", [39, 89])
def test_longer_windows_stay_in_the_group(window):
    """Windows of 40 and 90 entries: lane r owns entries r, r + 32 (, r + 64); the spans [1, 6, 33, w]
    cross the 32-entry strides."""
    C = S.seeded_cfg(window=window, buffer=6, cell_cap=CAP)
    n_win = len(S.window_labels(C))
    assert n_win == window + 1
    rules = [(1, 14400), (6, 6000), (33, 2000), (window, 1000)]
    Tb = Table(C)
    Tb.add("oldest_only", {n_win - 1: mix(40, 40)})                     # outside every span (k <= window = n_win - 1)
    Tb.add("oldest_in_longest", {n_win - 2: mix(40, 40)})
    Tb.add("stride_edge_in", {32: mix(40, 40), 0: mix(20, 0)})          # entry n_win - 33: the first of span 33
    Tb.add("stride_edge_out", {33: mix(40, 40), 0: mix(20, 0)})
    Tb.add("every_entry", {a: mix(3, 1 if a % 2 else 0) for a in range(n_win)})
    Tb.add("spilled_far", {n_win - 2: mix(8, 0) + [T + 9] * 25, 35: mix(30, 2), 0: mix(25, 25)})
    Tb.add("big", {34: mix(GROUP_MAX, 300), 0: mix(30, 30)})
    Tb.add("class0", {0: mix(40, 40)})
    Tb.inactive("inactive")
    sd = SbSeeded(C, Tb.order, Tb.buckets, key=burn_key(rules))
    want, _ints = check(sd, Tb.order, Tb.buckets, Tb.names, rules=rules)
    by = by_service(want)
    one = lambda name: by[(S.SERVER, "S:" + name)]
    w = window
    assert one("oldest_only") == []
    assert one("oldest_in_longest") == [f"{T}|{Q}|40|40|0|1:14400:0:0:0,6:6000:0:0:0,33:2000:0:0:0,{w}:1000:40:40:1"]
    assert one("stride_edge_in") == [f"{T}|{Q}|60|40|0|1:14400:20:0:0,6:6000:20:0:0,33:2000:60:40:1,{w}:1000:60:40:1"]
    assert one("stride_edge_out") == [f"{T}|{Q}|60|40|0|1:14400:20:0:0,6:6000:20:0:0,33:2000:20:0:0,{w}:1000:60:40:1"]
    assert len(one("every_entry")) == 1 and len(one("big")) == 1 and len(one("spilled_far")) == 1


def test_window_shortened_by_a_reload_clips_the_spans():
    """The engine is built for 32 window buckets and the rules [1, 6, 31]; a reload to
    windowSizeInIntervals = 3 before the rollover leaves 4.  The spans 6 and 31 then read the whole
    window and print the configured k."""
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    rules = [(1, 14400), (6, 6000), (31, 2000)]
    Tb = Table(C)
    Tb.add("short_all", {0: mix(30, 30), 3: mix(30, 0)})
    Tb.add("short_old_bad", {3: mix(40, 40), 0: mix(20, 0)})            # in spans 6 and 31 now, not in span 1
    Tb.add("short_gone_bad", {4: mix(400, 400), 0: mix(30, 1)})         # the bad load left the window
    Tb.add("short_spilled", {2: mix(8, 0) + [T + 1] * 40, 0: mix(20, 20)})
    Tb.add("short_big", {1: mix(GROUP_MAX + 10, 900), 0: mix(20, 20), 9: mix(50, 50)})
    Tb.add("short_gone", {9: mix(40, 40)})                              # samples older than the new window only
    sd = SbSeeded(C, Tb.order, Tb.buckets, key=burn_key(rules))
    C3 = copy.deepcopy(sd.C)
    C3["streamCalcStats"]["windowSizeInIntervals"] = 3
    assert len(S.window_labels(C3)) == 4 and S.window_labels(C3)[-1] == S.window_labels(C)[-1]
    assert sd.eng.reload(copy.deepcopy(C3), gen=1) == []
    sd.so.window, sd.so.keep = 3, 3 + sd.so.buffer
    sd.C = C3
    want, _ints = check(sd, Tb.order, Tb.buckets, Tb.names, rules=rules)
    by = by_service(want)
    one = lambda name: by[(S.SERVER, "S:" + name)]
    assert one("short_all") == [f"{T}|{Q}|60|30|0|1:14400:30:30:1,6:6000:60:30:1,31:2000:60:30:1"]
    assert one("short_old_bad") == [f"{T}|{Q}|60|40|0|1:14400:20:0:0,6:6000:60:40:1,31:2000:60:40:1"]
    assert one("short_gone_bad") == [f"{T}|{Q}|30|1|0|1:14400:30:1:0,6:6000:30:1:0,31:2000:30:1:1"]
    assert len(one("short_spilled")) == 1 and one("short_gone") == []
    assert one("short_big")[0].startswith(f"{T}|{Q}|{GROUP_MAX + 30}|920|0|1:14400:20:20:1,6:6000:{GROUP_MAX + 30}:920:1,")

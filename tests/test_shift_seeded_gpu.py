"""K24 ls rows (shift.hip) on seeded engine state: one engine, one rollover, every case a series of
its own (tests/seeded.py).  The engine's rows must equal the CPU oracle's and a reference that
shares no code with either (tests/shift_ref.py: list slices, sorted, Fraction), byte for byte, and
shifts() the reference's integers.

The seeded window of windowSizeInIntervals = 31 holds 32 buckets (entries 0 .. 31, 31 the newest).
Rules [1 bucket: p95 up 3 (z 3), 6 buckets: p95 up 3 z 4, 6 buckets: p25 down 2 (z 3)], minRecent 20,
minBaseline 100; the default minDelta 50, S:named 20, S:class0 null.

What the inequalities come to with these rules (S = 100000):
  ratio, p95 up 3      a >= 0.15 mR: with mR = 200, a = 30 meets it exactly and 29 misses
  ratio, p25 down 2    b >= 0.5 mR: with mR = 40, b = 20 exactly
  z 4 at p95           (20 a - mR)^2 >= 304 mR: with mR = 40 that is a >= 7.52, so a = 8 passes and
                       a = 7 fails while both pass the ratio (a >= 6).  304 mR is a square only at
                       mR = 19 j^2, and then 20 a = mR + 76 j has no integer a at any size a test of
                       seconds can hold: the exact equality is test_shift_model's, on the routine itself
  minDelta             X2 - T2 = 100 exactly against 98"""
import collections
import copy

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import seeded as S  # noqa: E402
import shift_ref as R  # noqa: E402

CAP = 8                # bucketCellCapacity: samples in the inline cell, the rest in the spill list
GROUP_MAX = 512        # shift.hip LS_GROUP_MAX: window samples a 32-lane group sorts itself
NAN = S.ELAPSED_NAN
RULES = [(1, 95000, 3000, 0, 3000), (6, 95000, 3000, 0, 4000), (6, 25000, 0, 2000, 3000)]
MIN_RECENT, MIN_BASELINE = 20, 100
DELTA = 50
NAMED = {"S:named": 20}
OFF = "S:class0"


def shift_key(rules=RULES):
    services = {n: {"minDelta": d} for n, d in NAMED.items()}
    services[OFF] = None
    out = []
    for k, q, ru, rd, z in rules:
        r = {"short": k, "percentile": q / 1000, "z": z / 1000}
        if ru:
            r["up"] = ru / 1000
        if rd:
            r["down"] = rd / 1000
        out.append(r)
    return {"default": {"minDelta": DELTA}, "services": services, "rules": out,
            "minRecent": MIN_RECENT, "minBaseline": MIN_BASELINE}


class LsSeeded(S.Seeded):
    """Seeded with the ls stream on, on both sides."""

    def __init__(self, C, *a, key=None, **kw):
        self.ls = []
        C = copy.deepcopy(C)
        C["gpu"]["latencyShift"] = key or shift_key()
        super().__init__(C, *a, **kw)

    def _seed_oracle(self):
        from apmbackend_amd.utils.config import latency_shift
        super()._seed_oracle()
        self.so.emit_shift = self.ls.append
        self.so.shift = latency_shift(self.C)

    def _seed_engine(self):
        from apmbackend_amd.models import pipeline
        real = pipeline.APMEngine
        pipeline.APMEngine = lambda C, outputs=(): real(C, outputs=tuple(outputs) + ("ls",))
        try:
            super()._seed_engine()
        finally:
            pipeline.APMEngine = real


def delta_of(service):
    if service == OFF:
        return None
    return NAMED.get(service, DELTA)


def reference(C, order, buckets, rules):
    """(rows, per series id the integers or None) of the first rollover from the case table alone."""
    edge_ts = (S.LATEST + 1 - S.stats_settings(C)[2] - 1) * 10000
    labels = S.window_labels(C)
    rows, ints = [], []
    for key in order:
        d = delta_of(key[1])
        if key not in buckets or d is None:
            ints.append(None)
            continue
        e = [list(buckets[key].get(b, [])) for b in labels]
        ints.append(R.series_ints(e, rules, d, MIN_RECENT, MIN_BASELINE))
        r = R.row(edge_ts, key[0], key[1], e, rules, d, MIN_RECENT, MIN_BASELINE)
        if r is not None:
            rows.append(r)
    return rows, ints


def check(sd, order, buckets, names, rules=RULES):
    want, ints = reference(sd.C, order, buckets, rules)
    sd.step()
    got = sd.eng.take("ls")
    assert sd.ls == want, "oracle and reference differ: " + str(S.first_difference(sd.ls, want, lambda i: ""))
    diff = S.first_difference(got, want, lambda i: want[i].split("|")[3] if i < len(want) else "")
    assert diff is None, "ls rows: " + diff
    sd.eng.eng.flush()
    dev = sd.eng.eng.shifts()
    assert len(dev) >= len(order)
    for i, w in enumerate(ints):
        if w is None:
            assert dev[i] is None, f"series {i} ({names[i]}): record {dev[i]}, want none"
            continue
        assert dev[i] is not None, f"series {i} ({names[i]}): no record"
        n, per = dev[i]
        assert (n, [tuple(p) for p in per]) == w, f"series {i} ({names[i]}): {dev[i]}, want {w}"
    assert sd.eng.metrics()["ls_rows"] == len(want)
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


def base(n, lo=100, step=1, ages=range(10, 20)):
    """n baseline samples lo, lo + step, ... dealt over the given ages (outside every span)."""
    ages = list(ages)
    out = {a: [] for a in ages}
    for i in range(n):
        out[ages[i % len(ages)]].append(lo + i * step)
    return {a: v for a, v in out.items() if v}


def with_(b, **recent):
    """A baseline plus the recent entries a0 = [...], a3 = [...]"""
    d = dict(b)
    for k, v in recent.items():
        d[int(k[1:])] = list(v)
    return d


def case_table(C):
    Tb = Table(C)
    flat = base(100, lo=100, step=0)        # 100 samples of 100: T2 = 200 at every percentile
    ramp = base(200)                        # 100 .. 299: p95 = rank 189 alone (289), p25 = rank 49 alone (149)
    hi, lo = [1000], [1]
    # plain verdicts through the group kernel
    Tb.add("up_all", with_(ramp, a0=hi * 40))                           # rules 1 and 2
    Tb.add("down_6", with_(ramp, a0=lo * 10, a2=lo * 10, a5=lo * 20))   # rule 3 only: the newest bucket holds 10
    Tb.add("steady", with_(ramp, a0=list(range(100, 300, 5))))
    # the ratio: mR = 200 in the newest bucket, a = 30 exactly, 29, 31
    for a in (29, 30, 31):
        Tb.add(f"ratio_{a}", with_(ramp, a0=[400] * a + [120] * (200 - a)))
    # ... and below: mR = 40 over the six buckets, b = 19, 20, 21 (X2 = p25 of the span well under T2 = 298)
    for b in (19, 20, 21):
        Tb.add(f"ratio_down_{b}", with_(ramp, a1=[5] * b, a4=[200] * (40 - b)))
    # z 4 at p95, mR = 40 over the span: a = 7 fails, a = 8 passes (both pass the ratio); one bucket
    # of 19 keeps rule 1 below minRecent
    for a in (7, 8):
        Tb.add(f"z_{a}", with_(ramp, a0=[900] * a + [110] * (19 - a), a3=[110] * 21))
    # minDelta: T2 = 200, X2 = 300 is 2 * 50 exactly; 298 misses; the named class needs 2 * 20
    Tb.add("delta_exact", with_(flat, a0=[150] * 30))
    Tb.add("delta_miss", with_(flat, a0=[149] * 30))
    Tb.add("delta_down_exact", with_(flat, a0=[50] * 30))
    Tb.add("delta_down_miss", with_(flat, a0=[51] * 30))
    Tb.add("named", with_(flat, a0=[120] * 30))                         # S:named: minDelta 20, X2 - T2 = 40
    Tb.add("default_next_to_named", with_(flat, a0=[120] * 30))
    Tb.add("class0", with_(flat, a0=[900] * 30))
    # minRecent and minBaseline, one sample either side; 100 baseline samples read one rank, 101 two
    for m in (19, 20, 21):
        Tb.add(f"recent_{m}", with_(ramp, a0=hi * m))
    for m in (99, 100, 101):
        Tb.add(f"baseline_{m}", with_(base(m, lo=100, step=3), a0=hi * 30))
    # ties: every sample equals the percentile on both sides, a = b = 0
    Tb.add("tied", with_(flat, a0=[100] * 40))
    Tb.add("tied_above_counts", with_(flat, a0=[100] * 20 + [101] * 20))   # a = 20: the tie counts on neither side
    # NaN samples
    Tb.add("nan_span", with_(ramp, a0=hi * 30 + [NAN] * 15))
    Tb.add("nan_span_below_min", with_(ramp, a0=hi * 19 + [NAN] * 15))
    Tb.add("nan_baseline", with_({**ramp, 25: [NAN] * 12, 7: [NAN]}, a0=hi * 30))
    Tb.add("nan_baseline_only", {12: [NAN] * 60, 13: [NAN] * 60, 0: hi * 30})
    Tb.add("nan_recent_only", with_(ramp, a0=[NAN] * 30))
    # negative samples and INT32_MAX
    Tb.add("negative_up", with_(base(120, lo=-5000), a0=[-100] * 30))
    Tb.add("negative_down", with_(base(120, lo=-500), a0=[-S.INT32_MAX] * 30))
    Tb.add("int32_max", with_(ramp, a0=[S.INT32_MAX] * 30))
    Tb.add("int32_max_both", with_(base(100, lo=S.INT32_MAX, step=0), a0=[S.INT32_MAX] * 30))
    # empty sides
    Tb.add("empty_recent", dict(ramp))
    Tb.add("empty_baseline", {0: hi * 30, 3: hi * 30})
    Tb.add("edge_in_6", with_(ramp, a5=hi * 30))                        # the oldest entry of the 6-bucket span
    Tb.add("edge_out_6", with_(ramp, a6=hi * 30))                       # ... and the newest of its baseline
    # start-up: the baseline buckets mostly absent (only entries of age < 8 exist), few baseline samples
    Tb.add("filling", {a: hi * 12 if a < 6 else [100] * 12 for a in range(8)})
    Tb.add("filling_judged", {a: hi * 25 if a < 1 else [100] * 15 for a in range(8)})   # rule 1: mB = 105
    # spills (cell capacity 8): a span bucket of 9, a baseline bucket of 9, long runs on both sides
    Tb.add("spill_span_9", with_(ramp, a0=hi * 9, a1=hi * 20))
    Tb.add("spill_baseline_9", with_({**base(100, ages=range(10, 30)), 30: list(range(500, 509))}, a0=hi * 30))
    Tb.add("spill_runs", with_({8: list(range(100, 250)), 9: list(range(100, 200))}, a0=hi * 60, a5=lo * 90))
    # the group / block boundary: exactly 512 and 513 window samples
    Tb.pad_even()
    Tb.add("n512", with_(base(472, lo=100), a0=hi * 40))
    Tb.add("n513", with_(base(473, lo=100), a0=hi * 40))
    Tb.add("n513_down", with_(base(473, lo=100), a0=lo * 40))
    Tb.add("big_neighbour", with_(ramp, a0=hi * 40))
    # one big series whose span alone is small
    Tb.add("big_small_span", with_(base(5000, lo=10, ages=range(6, 32)), a0=[40000] * 25))
    Tb.add("big_small_span_down", with_(base(5000, lo=1000, ages=range(6, 32)), a2=lo * 25))
    Tb.add("big_quiet", with_(base(5000, lo=10, ages=range(6, 32)), a0=list(range(10, 5010, 200))))
    Tb.add("big_nan_ties", {9: [100] * 600 + [NAN] * 7, 0: [100] * 30 + [NAN] * 3})
    Tb.add("class0", with_(base(600), a0=hi * 40), server="jvm02")      # big and class 0: no record
    # the named class on another server shares its class; empty window; inactive series
    Tb.add("named", with_(flat, a0=[119] * 30), server="jvm01")         # X2 - T2 = 38 < 40
    b = collections.OrderedDict({Tb.labels[3]: []})
    S.add_series(Tb.order, Tb.buckets, Tb.names, Tb.sizes, "count0", S.with_decoys(b, Tb.labels, len(Tb.order)))
    Tb.inactive("inactive")
    Tb.pad_even()
    Tb.add("works_next_to_inactive", with_(ramp, a0=hi * 40))
    Tb.inactive("inactive2")
    Tb.order.append(S.TRIGGER); Tb.names.append("trigger"); Tb.sizes.append(0)
    Tb.add("last_id", with_(ramp, a0=lo * 40))
    if len(Tb.order) % 2 == 0:
        Tb.add("odd_tail", with_(ramp, a0=hi * 40))
    assert len(Tb.order) % 2 == 1, "the last wave's upper half must be past n_series"
    return Tb


def by_service(rows):
    by = collections.defaultdict(list)
    for r in rows:
        by[(r.split("|")[2], r.split("|")[3])].append(r.split("|", 4)[4])
    return by


def verdicts(row):
    return "".join(g.split(":")[8] for g in row.split("|")[2].split(","))


def expectations(Tb, want, ints):
    """What the case table must come to, on the reference's rows and integers."""
    by = by_service(want)
    J = S.SERVER
    one = lambda name: by[(J, "S:" + name)]
    v = lambda name: verdicts(one(name)[0]) if one(name) else ""
    assert v("up_all") == "UUN" and v("down_6") == "NND" and v("steady") == ""
    assert one("up_all") == ["240|50|1:95:200:578:40:2000:40:0:U,6:95:200:578:40:2000:40:0:U,6:25:200:298:40:2000:40:0:N"]
    assert v("ratio_29") == "" and v("ratio_30") == "UUN" and v("ratio_31") == "UUN"
    assert v("ratio_down_19") == "" and v("ratio_down_20") == "NND" and v("ratio_down_21") == "NND"
    assert v("z_7") == "" and v("z_8") == "NUN"
    assert v("delta_exact") == "UUN" and v("delta_miss") == ""
    assert v("delta_down_exact") == "NND" and v("delta_down_miss") == ""
    assert one("named") == ["130|20|1:95:100:200:30:240:30:0:U,6:95:100:200:30:240:30:0:U,6:25:100:200:30:240:30:0:N"]
    assert by[("jvm01", "S:named")] == [] and one("default_next_to_named") == []
    assert (J, OFF) not in by and ("jvm02", OFF) not in by
    assert v("recent_19") == "" and v("recent_20") == "UUN" and v("recent_21") == "UUN"
    assert v("baseline_99") == "" and v("baseline_100") == "UUN" and v("baseline_101") == "UUN"
    idx = {k: i for i, k in enumerate(Tb.order)}
    rec = lambda name: ints[idx[(J, "S:" + name)]]
    assert rec("baseline_100")[1][0][6] == 2 * (100 + 3 * 94)           # one rank
    assert rec("baseline_101")[1][0][6] == (100 + 3 * 95) + (100 + 3 * 96)   # two ranks
    assert v("tied") == "" and rec("tied")[1][0][4:6] == (0, 0)
    assert rec("tied_above_counts")[1][0][4:6] == (20, 0)
    assert v("nan_span") == "UUN" and rec("nan_span")[1][0][2:4] == (30, 15) and v("nan_span_below_min") == ""
    assert v("nan_baseline") == "UUN" and rec("nan_baseline")[1][0][:2] == (200, 13)
    assert v("nan_baseline_only") == "" and rec("nan_baseline_only")[1][0][:2] == (0, 120)
    assert rec("nan_baseline_only")[1][0][4:8] == (0, 0, 0, 2000)
    assert v("nan_recent_only") == "" and rec("nan_recent_only")[1][0][2:4] == (0, 30)
    assert v("negative_up") == "UUN" and v("negative_down") == "NND"
    assert v("int32_max") == "UUN" and v("int32_max_both") == ""
    assert v("empty_recent") == "" and rec("empty_recent")[1][0][2:4] == (0, 0)
    assert v("empty_baseline") == "" and rec("empty_baseline")[1][1][:2] == (0, 0)
    assert v("edge_in_6") == "NUN" and v("edge_out_6") == ""
    assert v("filling") == "" and rec("filling")[1][1][0] == 24 and v("filling_judged") == "UNN"
    assert v("spill_span_9") == "NUN" and v("spill_baseline_9") == "UUN" and v("spill_runs")
    assert rec("n512")[0] == GROUP_MAX and rec("n513")[0] == GROUP_MAX + 1
    assert v("n512") == "UUN" and v("n513") == "UUN" and v("n513_down") == "NND" and v("big_neighbour") == "UUN"
    assert v("big_small_span") == "UUN" and v("big_small_span_down") == "NND" and v("big_quiet") == ""
    assert v("big_nan_ties") == "" and rec("big_nan_ties")[1][0] == (600, 7, 30, 3, 0, 0, 200, 200, "N")
    assert rec("count0") == (0, [(0, 0, 0, 0, 0, 0, 0, 0, "N")] * 3)
    assert ints[idx[(J, OFF)]] is None and ints[idx[(J, "S:inactive")]] is None
    assert v("works_next_to_inactive") == "UUN" and v("last_id") == "NND"


def test_constants_are_the_kernels():
    from apmbackend_amd import _native
    N = _native.load(build_if_missing=False)
    assert N.shift_group_max() == GROUP_MAX and N.shift_group_win() == 32


def test_case_table_reaches_both_kernels():
    """(no engine) the table itself puts U and D through the group pass and through the block pass"""
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    Tb = case_table(C)
    C2 = copy.deepcopy(C)
    C2["gpu"]["latencyShift"] = shift_key()
    _rows, ints = reference(C2, Tb.order, Tb.buckets, RULES)
    seen = {"group": set(), "big": set()}
    for w in ints:
        if w is not None:
            seen["big" if w[0] > GROUP_MAX else "group"] |= {p[8] for p in w[1]}
    assert seen["group"] >= {"U", "D", "N"} and seen["big"] >= {"U", "D", "N"}
    expectations(Tb, _rows, ints)


def test_one_rollover_all_cases():
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    assert len(S.window_labels(C)) == 32
    Tb = case_table(C)
    sd = LsSeeded(C, Tb.order, Tb.buckets)
    want, ints = check(sd, Tb.order, Tb.buckets, Tb.names)
    expectations(Tb, want, ints)
    # the st / fs rows are what an engine without the stream prints
    plain = S.Seeded(C, Tb.order, Tb.buckets, reference=False)
    plain.step()
    assert sd.eng.take("st") == plain.eng.take("st") == sd.st
    assert sd.eng.take("fs") == plain.eng.take("fs")
    assert plain.eng.take("ls") == [] and plain.eng.eng.shifts() == []


def test_window_shortened_by_a_reload_leaves_no_baseline():
    """The engine is built for 32 window buckets; a reload to windowSizeInIntervals = 3 before the
    rollover leaves 4.  The spans of 6 then cover the whole window: mB = 0 and the rule says N; the
    1-bucket rule still judges."""
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    Tb = Table(C)
    Tb.add("short_up", {0: [1000] * 40, 1: list(range(100, 150)), 2: list(range(100, 150)), 3: list(range(100, 130))})
    Tb.add("short_gone", {0: [1000] * 40, 9: list(range(100, 300))})    # the baseline left the window
    Tb.add("short_big", {0: [1000] * 40, 2: list(range(100, 700))})
    sd = LsSeeded(C, Tb.order, Tb.buckets)
    C3 = copy.deepcopy(sd.C)
    C3["streamCalcStats"]["windowSizeInIntervals"] = 3
    assert len(S.window_labels(C3)) == 4 and S.window_labels(C3)[-1] == S.window_labels(C)[-1]
    assert sd.eng.reload(copy.deepcopy(C3), gen=1) == []
    sd.so.window, sd.so.keep = 3, 3 + sd.so.buffer
    sd.C = C3
    want, _ints = check(sd, Tb.order, Tb.buckets, Tb.names)
    by = by_service(want)
    one = lambda name: by[(S.SERVER, "S:" + name)]
    # rule 1's baseline: 100 .. 129 three times, 130 .. 149 twice; p95 of 130 reads ranks 123, 124 (146 + 147).
    # p25 of all 170 reads ranks 42, 43 (114 twice)
    assert one("short_up") == ["170|50|1:95:130:293:40:2000:40:0:U,6:95:0:0:170:2000:0:0:N,6:25:0:0:170:228:0:0:N"]
    assert one("short_gone") == []
    assert verdicts(one("short_big")[0]) == "UNN"

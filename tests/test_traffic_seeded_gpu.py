"""K22 tf rows (traffic.hip) on seeded engine state: one engine, one rollover, every case a series of
its own (tests/seeded.py).  The engine's rows must equal the CPU oracle's and a reference that
shares no code with either (tests/traffic_ref.py: lists, sorted, Python integers), byte for byte,
and traffic() the reference's integers.

The seeded window of windowSizeInIntervals = 31 holds 32 buckets (entries 0 .. 31, 31 the newest).
The rules [1 bucket: drop 0.1, z 4] and [6 buckets: drop 0.5, surge 3, z 3], minBuckets 8; the
default minRate 5, one service with 50, one named with null.  Rule 1 has B = 31 baseline buckets
(odd: lo = hi = 15), rule 2 has B = 26 (even: lo = 12, hi = 13)."""
import collections
import copy
import random

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import seeded as S  # noqa: E402
import traffic_ref as R  # noqa: E402

CAP = 8                # bucketCellCapacity: samples in the inline cell, the rest in the spill list
TILE = 64              # traffic.hip TF_TILE: series per block of the group pass
GROUP_WIN = 128        # traffic.hip TF_GROUP_WIN: window buckets the group pass takes
NAN = S.ELAPSED_NAN
RATE = 5
RULES = [(1, 100, 0, 4000), (6, 500, 3000, 3000)]
MIN_BUCKETS = 8
NAMED = {"S:busy": 50}
OFF = "S:class0"


def traffic_key(rules=RULES, min_buckets=MIN_BUCKETS):
    services = {n: {"minRate": r} for n, r in NAMED.items()}
    services[OFF] = None
    out = []
    for k, r_d, r_s, z in rules:
        r = {"short": k, "z": z / 1000}
        if r_d:
            r["drop"] = r_d / 1000
        if r_s:
            r["surge"] = r_s / 1000
        out.append(r)
    return {"default": {"minRate": RATE}, "services": services, "rules": out, "minBuckets": min_buckets}


class TfSeeded(S.Seeded):
    """Seeded with the tf stream on, on both sides."""

    def __init__(self, C, *a, key=None, **kw):
        self.tf = []
        C = copy.deepcopy(C)
        C["gpu"]["trafficWatch"] = key or traffic_key()
        super().__init__(C, *a, **kw)

    def _seed_oracle(self):
        from apmbackend_amd.utils.config import traffic_watch
        super()._seed_oracle()
        self.so.emit_traffic = self.tf.append
        self.so.traffic = traffic_watch(self.C)

    def _seed_engine(self):
        from apmbackend_amd.models import pipeline
        real = pipeline.APMEngine
        pipeline.APMEngine = lambda C, outputs=(): real(C, outputs=tuple(outputs) + ("tf",))
        try:
            super()._seed_engine()
        finally:
            pipeline.APMEngine = real


def rate_of(service):
    if service == OFF:
        return None
    return NAMED.get(service, RATE)


def reference(C, order, buckets, rules, min_buckets):
    """(rows, per series id the integers or None) of the first rollover from the case table alone."""
    edge_ts = (S.LATEST + 1 - S.stats_settings(C)[2] - 1) * 10000
    labels = S.window_labels(C)
    rows, ints = [], []
    for key in order:
        rate = rate_of(key[1])
        if key not in buckets or rate is None:
            ints.append(None)
            continue
        counts = [len(buckets[key].get(b, [])) for b in labels]
        ints.append(R.series_ints(counts, rules, rate, min_buckets))
        r = R.row(edge_ts, key[0], key[1], counts, rules, rate, min_buckets)
        if r is not None:
            rows.append(r)
    # st order: the servers in the order of their first series, each with its series in theirs
    servers = list(collections.OrderedDict((k[0], 1) for k in order))
    rows.sort(key=lambda r: servers.index(r.split("|")[2]))
    return rows, ints


def check(sd, order, buckets, names, rules=RULES, min_buckets=MIN_BUCKETS):
    want, ints = reference(sd.C, order, buckets, rules, min_buckets)
    sd.step()
    got = sd.eng.take("tf")
    assert sd.tf == want, "oracle and reference differ: " + str(S.first_difference(sd.tf, want, lambda i: ""))
    diff = S.first_difference(got, want, lambda i: want[i].split("|")[3] if i < len(want) else "")
    assert diff is None, "tf rows: " + diff
    sd.eng.eng.flush()
    dev = sd.eng.eng.traffic()
    assert len(dev) >= len(order)
    for i, w in enumerate(ints):
        if w is None:
            assert dev[i] is None, f"series {i} ({names[i]}): record {dev[i]}, want none"
            continue
        assert dev[i] is not None, f"series {i} ({names[i]}): no record"
        n, per = dev[i]
        assert (n, [tuple(p) for p in per]) == w, f"series {i} ({names[i]}): {dev[i]}, want {w}"
    assert sd.eng.metrics()["tf_rows"] == len(want)
    return want, ints


class Table:
    """Case builder: a series from its per-bucket counts, oldest entry first."""

    def __init__(self, C):
        self.C = C
        self.labels = S.window_labels(C)
        self.order, self.buckets, self.names, self.sizes = [], {}, [], []

    def add(self, name, counts, nan_every=0, server=None, absent_zeros=True):
        assert len(counts) == len(self.labels), (name, len(counts))
        b = collections.OrderedDict()
        for lab, c in zip(self.labels, counts):
            if c or not absent_zeros:      # (a zero count: no bucket row, or a row with no samples)
                b[lab] = [NAN if nan_every and i % nan_every == 0 else 100 + i for i in range(c)]
        b = S.with_decoys(b, self.labels, len(self.order))
        if server is None:
            return S.add_series(self.order, self.buckets, self.names, self.sizes, name, b)
        k = (server, S.key(name)[1])
        self.order.append(k); self.buckets[k] = b; self.names.append(f"{server}/{name}"); self.sizes.append(0)
        return k

    def inactive(self, name):
        self.order.append(S.key(name)); self.names.append(name); self.sizes.append(0)

    def pad_to(self, n):
        while len(self.order) < n:
            self.add(f"pad{len(self.order)}", [7] * len(self.labels))


def last_R(base, k, rule, want, rate=RATE, min_buckets=MIN_BUCKETS):
    """The recent total R at the edge of rule's verdict `want` over the baseline `base`: the largest R
    that still drops ("D"), the smallest that surges ("S")."""
    says = lambda r: R.rule_ints(base + [r] + [0] * (k - 1), *rule, rate, min_buckets)[4]
    r = 0
    if want == "D":
        assert says(0) == "D"
        while says(r + 1) == "D":
            r += 1
    else:
        while says(r) != "S":
            r += 1
    return r


def spread(total, k):
    """`total` samples over k buckets."""
    return [total // k + (1 if i < total % k else 0) for i in range(k)]


def case_table(C, rules=RULES):
    Tb = Table(C)
    n = len(Tb.labels)
    assert n == 32
    Tb.add("steady_then_0", [10] * 31 + [0])                            # D with mad4 = 0
    # rule 1's ratio test: 2000 R <= 100 * 1 * 20
    Tb.add("drop_ratio_on", [10] * 31 + [1])
    Tb.add("drop_ratio_off", [10] * 31 + [2])
    # rule 1's MAD test binds when the baseline is noisy: the edge found with the reference
    noisy = [76, 124] * 15 + [100]                                      # median 100, MAD 24
    r1 = last_R(noisy, 1, RULES[0], "D")
    Tb.add("drop_mad_on", noisy + [r1])
    Tb.add("drop_mad_off", noisy + [r1 + 1])
    # rule 2's surge: 2000 R >= 3000 * 6 * 20 at R = 180, and its MAD test over a noisy baseline
    Tb.add("surge_ratio_on", [10] * 26 + [30] * 6)
    Tb.add("surge_ratio_off", [10] * 26 + [30] * 5 + [29])
    noisy2 = [2, 22] * 13                                               # median 12, MAD 10
    r2 = last_R(noisy2, 6, RULES[1], "S")
    Tb.add("surge_mad_on", noisy2 + spread(r2, 6))
    Tb.add("surge_mad_off", noisy2 + spread(r2 - 1, 6))
    # rule 2's drop at its edge: 2000 R <= 500 * 6 * 20 -> R <= 30
    Tb.add("drop6_on", [10] * 26 + spread(30, 6))
    Tb.add("drop6_off", [10] * 26 + spread(31, 6))
    # an alternating baseline: the MAD term keeps it quiet at z = 3 (and 4) even with the newest buckets empty
    Tb.add("alternating", [0, 20] * 13 + [0] * 6)
    Tb.add("alternating_rows", [0, 20] * 13 + [0] * 6, absent_zeros=False)   # (empty bucket rows instead of absent ones)
    # more than half of the baseline absent: the median is 0
    Tb.add("mostly_absent", [0] * 17 + [10] * 14 + [0])
    Tb.add("filling", [0] * 24 + [10] * 7 + [0])                        # a window that fills after a start
    # the minRate gate: med2 = 10 judged, 9 not (13 fours and 13 fives under rule 2)
    Tb.add("rate_on", [5] * 31 + [0])
    Tb.add("rate_off", [4, 5] * 13 + [0] * 6)
    # NaN samples count
    Tb.add("nans", [10] * 31 + [0], nan_every=3)
    Tb.add("nans_recent", [10] * 31 + [1], nan_every=1)
    # counts beyond the inline cell: part of every bucket sits in the spill list, only counts is read
    Tb.add("spilled", [20] * 31 + [1])
    Tb.add("spilled_flood", [9] * 26 + [60] * 6)
    # classes
    Tb.add("class0", [10] * 31 + [0])
    Tb.add("busy", [40] * 31 + [0])                                     # minRate 50: med2 80 < 100
    Tb.add("busy", [50] * 31 + [0], server="jvm01")                     # ... and the same class judged
    Tb.add("default_next_to_busy", [40] * 31 + [0])
    # nothing in the window
    b = collections.OrderedDict({Tb.labels[3]: []})
    S.add_series(Tb.order, Tb.buckets, Tb.names, Tb.sizes, "count0", S.with_decoys(b, Tb.labels, len(Tb.order)))
    Tb.inactive("inactive")
    rng = random.Random(5)
    for i in range(12):                                                 # random windows, some with a cliff
        c = [rng.choice([0, 3, 8, 9, 10, 11, 12, 30]) for _ in range(n)]
        if i % 3 == 0:
            tail = rng.choice([1, 3, 6])
            c[n - tail:] = [0] * tail
        Tb.add(f"random{i}", c)
    # a tile boundary: ids 63 and 64 fire, with a class-0 and an inactive series next to them
    Tb.pad_to(TILE - 2)
    Tb.add("class0", [10] * 31 + [0], server="jvm02")
    Tb.add("tile_last", [12] * 31 + [0])
    Tb.add("tile_first", [10] * 26 + [40] * 6)
    Tb.inactive("inactive2")
    Tb.add("after_inactive", [11] * 31 + [1])
    Tb.pad_to(TILE + 6)
    Tb.add("last_id", [10] * 31 + [0])
    assert len(Tb.order) % TILE and Tb.order.index(S.key("tile_last")) == TILE - 1
    return Tb


def by_service(rows):
    by = collections.defaultdict(list)
    for r in rows:
        by[(r.split("|")[2], r.split("|")[3])].append(r.split("|", 4)[4])
    return by


def test_constants_are_the_kernels():
    from apmbackend_amd import _native
    N = _native.load(build_if_missing=False)
    assert N.traffic_tile() == TILE and N.traffic_group_win() == GROUP_WIN


def test_one_rollover_all_cases():
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    assert len(S.window_labels(C)) == 32
    Tb = case_table(C)
    sd = TfSeeded(C, Tb.order, Tb.buckets)
    want, ints = check(sd, Tb.order, Tb.buckets, Tb.names)
    by = by_service(want)
    J = S.SERVER
    one = lambda name: by[(J, "S:" + name)]
    assert one("steady_then_0") == ["310|5|1:31:0:20:0:D,6:26:50:20:0:N"]
    assert one("drop_ratio_on") == ["311|5|1:31:1:20:0:D,6:26:51:20:0:N"] and one("drop_ratio_off") == []
    # the MAD edge of rule 1: the ratio test alone would still pass one sample further
    (row,) = one("drop_mad_on")
    g = [x.split(":") for x in row.split("|")[2].split(",")]
    R1, med2, mad4 = int(g[0][2]), int(g[0][3]), int(g[0][4])
    assert g[0][5] == "D" and mad4 > 0 and 4000 * R1 <= 2000 * med2 - 4000 * mad4 < 4000 * (R1 + 1)
    assert 2000 * (R1 + 1) <= 100 * med2 and one("drop_mad_off") == []
    assert one("surge_ratio_on") == ["440|5|1:31:30:20:0:N,6:26:180:20:0:S"] and one("surge_ratio_off") == []
    (row,) = one("surge_mad_on")
    g = [x.split(":") for x in row.split("|")[2].split(",")]
    R2, med2, mad4 = int(g[1][2]), int(g[1][3]), int(g[1][4])
    assert g[1][5] == "S" and mad4 > 0 and 4000 * (R2 - 1) < 6 * (2000 * med2 + 3000 * mad4) <= 4000 * R2
    assert 2000 * (R2 - 1) >= 3000 * 6 * med2 and one("surge_mad_off") == []
    assert one("drop6_on") == ["290|5|1:31:5:20:0:N,6:26:30:20:0:D"] and one("drop6_off") == []
    assert one("alternating") == [] and one("alternating_rows") == []
    assert one("mostly_absent") == [] and one("filling") == []
    assert one("rate_on") == ["155|5|1:31:0:10:0:D,6:26:25:10:0:N"] and one("rate_off") == []
    assert one("nans") == one("steady_then_0") and one("nans_recent") == one("drop_ratio_on")
    assert one("spilled") == ["621|5|1:31:1:40:0:D,6:26:101:40:0:N"]
    assert one("spilled_flood") == ["594|5|1:31:60:18:0:N,6:26:360:18:0:S"]
    assert (J, OFF) not in by and ("jvm02", OFF) not in by
    assert one("busy") == [] and by[("jvm01", "S:busy")] == ["1550|50|1:31:0:100:0:D,6:26:250:100:0:N"]
    assert one("default_next_to_busy") == ["1240|5|1:31:0:80:0:D,6:26:200:80:0:N"]
    assert one("count0") == [] and one("inactive") == []
    assert one("tile_last") and one("tile_first") and one("after_inactive") and one("last_id")
    # what traffic() reports for series that print nothing
    idx = {k: i for i, k in enumerate(Tb.order)}
    assert ints[idx[(J, "S:count0")]] == (0, [(31, 0, 0, 0, "N"), (26, 0, 0, 0, "N")])
    assert ints[idx[(J, OFF)]] is None and ints[idx[(J, "S:inactive")]] is None
    assert ints[idx[(J, "S:alternating")]] == (260, [(31, 0, 0, 0, "N"), (26, 0, 20, 40, "N")])
    assert ints[idx[(J, "S:rate_off")]][1][1] == (26, 0, 9, 2, "N")
    assert ints[idx[(J, "S:mostly_absent")]][1][0][2] == 0
    # the st / fs rows are what an engine without the stream prints
    plain = S.Seeded(C, Tb.order, Tb.buckets, reference=False)
    plain.step()
    assert sd.eng.take("st") == plain.eng.take("st") == sd.st
    assert sd.eng.take("fs") == plain.eng.take("fs")
    assert plain.eng.take("tf") == [] and plain.eng.eng.traffic() == []


@pytest.mark.parametrize("window", [30, 39, 89, GROUP_WIN + 1])
def test_window_lengths(window):
    """Windows of 31, 40, 90 and 130 entries: one, two and four entries a lane in the register sort,
    and the counting path past its limit; the spans [1, 6, 20, 30] leave odd and even baselines."""
    C = S.seeded_cfg(window=window, buffer=6, cell_cap=CAP)
    n = len(S.window_labels(C))
    assert n == window + 1
    rules = [(1, 100, 0, 4000), (6, 500, 3000, 3000), (20, 500, 2000, 0), (30, 900, 1100, 1000)]
    Tb = Table(C)
    Tb.add("stopped", [10] * (n - 1) + [0])
    Tb.add("stopped6", [10] * (n - 6) + [0] * 6)
    Tb.add("flood20", [10] * (n - 20) + [25] * 20)
    Tb.add("oldest_only", [50] + [0] * (n - 1))
    Tb.add("ramp", [i % 17 + 3 for i in range(n)])
    Tb.add("spilled", [30 + (i * 7) % 11 for i in range(n - 1)] + [2])
    rng = random.Random(window)
    for i in range(10):
        c = [rng.choice([0, 5, 9, 10, 11, 12, 13, 40]) for _ in range(n)]
        if i % 2:
            tail = rng.choice([1, 6, 20, 30])
            c[n - tail:] = [rng.choice([0, 0, 1, 60])] * tail
        Tb.add(f"random{i}", c)
    Tb.add("class0", [10] * (n - 1) + [0])
    Tb.inactive("inactive")
    Tb.add("odd_tail", [10] * (n - 1) + [0])
    sd = TfSeeded(C, Tb.order, Tb.buckets, key=traffic_key(rules))
    want, ints = check(sd, Tb.order, Tb.buckets, Tb.names, rules=rules)
    by = by_service(want)
    one = lambda name: by[(S.SERVER, "S:" + name)]
    t = 10 * (n - 1)
    assert one("stopped") == [f"{t}|5|1:{n - 1}:0:20:0:D,6:{n - 6}:50:20:0:N,20:{n - 20}:190:20:0:N,30:{n - 30}:290:20:0:N"]
    assert one("stopped6")[0].split(",")[1:3] == [f"6:{n - 6}:0:20:0:D", f"20:{n - 20}:140:20:0:N"]
    assert one("flood20")[0].split(",")[2] == f"20:{n - 20}:500:20:0:S"
    assert one("oldest_only") == [] and len(one("odd_tail")) == 1
    verdicts = {p[4] for w in ints if w for p in w[1]}
    assert verdicts == {"D", "S", "N"}


def test_window_shortened_by_a_reload_clips_the_spans():
    """The engine is built for 32 window buckets and the rules [1, 6]; a reload to
    windowSizeInIntervals = 3 before the rollover leaves 4.  Span 6 then covers the whole window
    (short >= n_win: no baseline, B = 0) and prints the configured k; span 1 has B = 3."""
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    Tb = Table(C)
    Tb.add("short_stop", [9] * 28 + [10, 10, 10, 0])
    Tb.add("short_same", [0] * 28 + [10, 10, 10, 10])
    Tb.add("short_gone", [10] * 20 + [0] * 12)                          # samples older than the new window only
    sd = TfSeeded(C, Tb.order, Tb.buckets, key=traffic_key(min_buckets=3))
    C3 = copy.deepcopy(sd.C)
    C3["streamCalcStats"]["windowSizeInIntervals"] = 3
    assert len(S.window_labels(C3)) == 4 and S.window_labels(C3)[-1] == S.window_labels(C)[-1]
    assert sd.eng.reload(copy.deepcopy(C3), gen=1) == []
    sd.so.window, sd.so.keep = 3, 3 + sd.so.buffer
    sd.C = C3
    want, ints = check(sd, Tb.order, Tb.buckets, Tb.names, min_buckets=3)
    by = by_service(want)
    one = lambda name: by[(S.SERVER, "S:" + name)]
    assert one("short_stop") == ["30|5|1:3:0:20:0:D,6:0:30:0:0:N"]
    assert one("short_same") == [] and one("short_gone") == []
    assert ints[1] == (40, [(3, 10, 20, 0, "N"), (0, 40, 0, 0, "N")])

"""K23 po rows (peers.hip) on seeded engine state: one engine, one rollover, every case a service of
its own whose members are series on different servers (tests/seeded.py).  The engine's rows must
equal the CPU oracle's and a reference that shares no code with either (tests/peers_ref.py: lists,
sorted, Python integers), byte for byte, and peers() the reference's integers.  With the wp stream
on at the same percentile, a po row's x is twice the value its series' wp row prints.

Settings: percentile 95, high 2, low 0.25, z 3, minDelta 10, minPeers 5, minSamples 4; the default
minValue 20, S:lowgate 1, S:class0 null.  A member of value v holds the samples [v] * 4 unless the
case says otherwise, so its x is 2 v."""
import copy
import random
from fractions import Fraction

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import seeded as S  # noqa: E402
import peers_ref as R  # noqa: E402

CAP = 8
GROUP_MAX = 128        # peers.hip: 32 lanes x PEER_E members; larger groups take the block pass
NAN = S.ELAPSED_NAN
INACTIVE = None
SET = R.Settings(95000, 2000, 250, 3000, 10, 5, 4)
MIN_VALUE = 20
NAMED = {"S:lowgate": 1}
OFF = "S:class0"
MAXV = S.INT32_MAX
XM = 2 * MAXV


def peer_key():
    services = {n: {"minValue": v} for n, v in NAMED.items()}
    services[OFF] = None
    return {"percentile": 95, "default": {"minValue": MIN_VALUE}, "services": services, "high": 2, "low": 0.25, "z": 3,
            "minDelta": 10, "minPeers": 5, "minSamples": 4}


class PoSeeded(S.Seeded):
    """Seeded with the po and wp streams on, on both sides."""

    def __init__(self, C, *a, **kw):
        self.po, self.wp = [], []
        C = copy.deepcopy(C)
        C["gpu"]["peerOutliers"] = peer_key()
        C["gpu"]["windowPercentiles"] = [95]
        super().__init__(C, *a, **kw)

    def _seed_oracle(self):
        from apmbackend_amd.utils.config import peer_outliers, window_percentiles
        super()._seed_oracle()
        self.so.emit_peer = self.po.append
        self.so.peer = peer_outliers(self.C)
        self.so.emit_pct = self.wp.append
        self.so.percentiles = window_percentiles(self.C)

    def _seed_engine(self):
        from apmbackend_amd.models import pipeline
        real = pipeline.APMEngine
        pipeline.APMEngine = lambda C, outputs=(): real(C, outputs=tuple(outputs) + ("po", "wp"))
        try:
            super()._seed_engine()
        finally:
            pipeline.APMEngine = real


def min_value_of(service):
    if service == OFF:
        return None
    return NAMED.get(service, MIN_VALUE)


class Cases:
    """Services and their members.  Member k of a service lives on server jvm<k>; the servers are
    created in index order, so the emission order is server by server, each with its services in
    case order."""

    def __init__(self, C):
        self.C, self.labels = C, S.window_labels(C)
        self.names = []
        self.members = []    # (server index, case index, service, samples or INACTIVE)

    def add(self, name, *members):
        """members: a value v (samples [v] * 4), a sample list, or INACTIVE."""
        ci = len(self.names)
        self.names.append("S:" + name)
        for k, m in enumerate(members):
            if m is not INACTIVE and not isinstance(m, list):
                m = [m] * 4
            self.members.append((k, ci, "S:" + name, m))

    def table(self):
        order, buckets, samples = [], {}, {}
        for k, ci, svc, vals in sorted(self.members, key=lambda m: m[:2]):
            key = (f"jvm{k:03d}", svc)
            order.append(key)
            if vals is not INACTIVE:
                b = S.layout(list(vals), self.labels, "spread", where=ci + k)
                if not vals:
                    b[self.labels[(ci + k) % len(self.labels)]] = []
                buckets[key] = S.with_decoys(b, self.labels, ci + k)
            samples[key] = vals
        order.append(S.TRIGGER)
        return order, buckets, samples


def outlier_group(n):
    """n members at 100; from five on the last one is high (1000) and the second low (10)."""
    v = [100] * n
    if n >= 5:
        v[-1] = 1000
        v[1] = 10
    return v


SIZES = (1, 2, SET.min_peers - 1, SET.min_peers, 8, 31, 32, 33, GROUP_MAX - 1, GROUP_MAX, GROUP_MAX + 1, 3 * GROUP_MAX)


def case_table(C):
    T = Cases(C)
    for n in SIZES:
        T.add(f"size{n}", *outlier_group(n))
    T.add("all_equal", *[100] * 7)                                       # MAD 0, nobody differs
    T.add("even_middles", 100, 110, 120, 140, 150, 900)                  # X2 = 2 (120 + 140)
    T.add("dup_median", 50, 100, 100, 100, 100, 100, 400)                # duplicates astride the median
    T.add("short_member", 100, 100, [5000] * 3, 100, 100, 100)           # m = minSamples - 1: no peer, no row
    T.add("nan_lowers_m", 100, 100, [5000, NAN, 5000, 5000], 100, 100, 1000)
    T.add("four_and_a_short", 100, 100, 100, 1000, [100] * 3)            # E = minPeers - 1: not judged
    T.add("inactive_member", 100, INACTIVE, 100, 100, 100, 1000)
    T.add("inactive_first", INACTIVE, 100, 100, 100, 100, 10)
    T.add("class0", 100, 100, 100, 100, 1000)
    T.add("width", [MAXV] * 4, [MAXV] * 4, [MAXV] * 4, [-MAXV] * 4, [-MAXV] * 4)   # X2 = 2 (2^32 - 2), L rows
    T.add("width_even", *([[MAXV] * 4] * 3 + [[-MAXV] * 4] * 3))         # X2 = 0, D4 = 4 (2^32 - 2): not judged
    T.add("width_mixed", [MAXV] * 4, [-MAXV] * 4, 100, 100, 100, 100, 100)
    T.add("high_and_low", 80, 85, 90, 95, 100, 400, 20)
    T.add("lowgate", 4, 4, 4, 4, 9, 4, 4, 4, 4, 14)                      # ratio and MAD pass; 2 x - X2 = 20 < 40, 40 >= 40
    T.add("delta_on", 20, 20, 20, 20, 45)                                # 2 x - X2 = 100 >= 40
    T.add("gate_off", 19, 19, 19, 19, 100)                               # X2 = 76 < 80
    T.add("gate_on", 20, 20, 20, 20, 100)
    T.add("mad_keeps_quiet", 20, 60, 100, 140, 180, 220, 300)            # above twice the median, inside 3 MADs
    T.add("count0_member", 100, [], 100, 100, 100, 1000)
    T.add("pair_rank", [10, 20, 30, 40, 50, 60, 70, 80, 90, 100] * 2, *[[30] * 20] * 5)   # m = 20: rank 18 alone
    T.add("odd_value", [1, 2, 3, 4, 5, 6, 7], 100, 100, 100, 100)        # m = 7: ranks 6, 6
    rng = random.Random(23)
    for g in range(10):
        base = rng.choice([30, 200, 5000, 100000])
        mem = []
        for _ in range(rng.choice([5, 6, 9, 16, 40])):
            v = base * rng.choice([3, 4]) if rng.random() < 0.15 else base // 6 if rng.random() < 0.1 else \
                base + rng.randint(-base // 20, base // 20)
            n = rng.choice([3, 4, 5, 9, 12])
            mem.append([v + rng.randint(-2, 2) for _ in range(n)] + [NAN] * rng.choice([0, 0, 1]))
        T.add(f"random{g}", *mem)
    return T


def reference(C, order, samples):
    """(rows, per series id the integers or None) of the first rollover from the case table alone."""
    edge_ts = (S.LATEST + 1 - S.stats_settings(C)[2] - 1) * 10000
    mem = [(key[0], key[1], samples.get(key), min_value_of(key[1])) for key in order]
    return R.rows(edge_ts, mem, SET)


def test_constants_are_the_kernels():
    from apmbackend_amd import _native
    N = _native.load(build_if_missing=False)
    assert N.peer_group_max() == GROUP_MAX


def test_one_rollover_all_cases():
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    T = case_table(C)
    order, buckets, samples = T.table()
    assert len(order) == len(set(order)) <= 4096
    want, ints = reference(C, order, samples)
    sd = PoSeeded(C, order, buckets)
    sd.step()
    got = sd.eng.take("po")
    assert sd.po == want, "oracle and reference differ: " + str(S.first_difference(sd.po, want, lambda i: ""))
    diff = S.first_difference(got, want, lambda i: "|".join(want[i].split("|")[2:4]) if i < len(want) else "")
    assert diff is None, "po rows: " + diff
    sd.eng.eng.flush()
    dev = sd.eng.eng.peers()
    assert len(dev) >= len(order)
    for i, w in enumerate(ints):
        assert (None if dev[i] is None else tuple(dev[i])) == w, f"series {i} {order[i]}: {dev[i]}, want {w}"
    assert sd.eng.metrics()["po_rows"] == len(want)
    check_literals(want, ints, order)

    # with wp on at the same percentile, a po row's x is twice what the series' wp row prints
    wp = {tuple(r.split("|")[2:4]): r.split("|")[6] for r in sd.eng.take("wp")}
    assert sd.wp and len(wp) == len(sd.wp)
    for r in want:
        f = r.split("|")
        label, value = wp[(f[2], f[3])].split(":")
        assert label == "95" and Fraction(value) * 2 == int(f[5].split(":")[1]), (r, wp[(f[2], f[3])])

    # the st / fs rows are what an engine without the stream prints, and that engine has no po state
    plain = S.Seeded(C, order, buckets, reference=False)
    plain.step()
    assert sd.eng.take("st") == plain.eng.take("st") == sd.st
    assert sd.eng.take("fs") == plain.eng.take("fs")
    assert plain.eng.take("po") == [] and plain.eng.eng.peers() == []


def check_literals(want, ints, order):
    """What the case table must give, spelled out."""
    by = {}
    for r in want:
        f = r.split("|")
        by.setdefault(f[3], []).append((f[2], "|".join(f[4:])))
    # group sizes: below minPeers nothing is judged; from it on the high and the low member print
    for n in SIZES:
        rows = by.get(f"S:size{n}", [])
        if n < SET.min_peers:
            assert rows == []
        else:
            assert rows == [("jvm001", f"4|95:20|{n}|400|0|L"), (f"jvm{n - 1:03d}", f"4|95:2000|{n}|400|0|H")], (n, rows)
    assert "S:all_equal" not in by and "S:class0" not in by and "S:four_and_a_short" not in by
    assert by["S:even_middles"] == [("jvm005", "4|95:1800|6|520|160|H")]
    assert by["S:dup_median"] == [("jvm006", "4|95:800|7|400|0|H")]
    assert "S:short_member" not in by and by["S:nan_lowers_m"] == [("jvm005", "4|95:2000|5|400|0|H")]
    assert by["S:inactive_member"] == [("jvm005", "4|95:2000|5|400|0|H")]
    assert by["S:inactive_first"] == [("jvm005", "4|95:20|5|400|0|L")]
    assert by["S:width"] == [("jvm003", f"4|95:{-XM}|5|{2 * XM}|0|L"), ("jvm004", f"4|95:{-XM}|5|{2 * XM}|0|L")]
    assert "S:width_even" not in by
    assert by["S:width_mixed"] == [("jvm000", f"4|95:{XM}|7|400|0|H"), ("jvm001", f"4|95:{-XM}|7|400|0|L")]
    assert [v[1][-1] for v in by["S:high_and_low"]] == ["H", "L"]
    assert by["S:lowgate"] == [("jvm009", "4|95:28|10|16|0|H")]
    assert by["S:delta_on"] == [("jvm004", "4|95:90|5|80|0|H")]
    assert "S:gate_off" not in by and by["S:gate_on"] == [("jvm004", "4|95:200|5|80|0|H")]
    assert "S:mad_keeps_quiet" not in by
    assert by["S:count0_member"] == [("jvm005", "4|95:2000|5|400|0|H")]
    assert by["S:pair_rank"] == [("jvm000", "20|95:200|6|120|0|H")]
    idx = {k: i for i, k in enumerate(order)}
    assert ints[idx[("jvm000", "S:width_even")]] == (4, XM, 6, 0, 4 * XM, "N")
    assert ints[idx[("jvm003", "S:four_and_a_short")]] == (4, 2000, 4, 400, 0, "N")
    assert ints[idx[("jvm002", "S:short_member")]] is None and ints[idx[("jvm001", "S:count0_member")]] is None
    assert ints[idx[("jvm000", OFF)]] is None and ints[idx[("jvm001", "S:inactive_member")]] is None
    assert ints[idx[("jvm006", "S:mad_keeps_quiet")]] == (4, 600, 7, 560, 640, "N")
    assert ints[idx[("jvm000", "S:odd_value")]][:2] == (7, 14)
    assert {v[5] for v in ints if v} == {"H", "L", "N"}
    assert any(r.split("|")[3].startswith("S:random") for r in want)


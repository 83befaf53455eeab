"""K19 sv rows (svcwin.hip) on seeded engine state: one engine, one rollover, every case a service of
its own whose members are series on different servers (tests/seeded.py).  The engine's rows must
equal the CPU oracle's and a reference that shares no code with either (tests/svcwin_ref.py:
concatenate + sorted() + Fraction ranks + integer halves), byte for byte, and svcwins() the
reference's integers."""
import copy
import random

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import seeded as S  # noqa: E402
import svcwin_ref as R  # noqa: E402

CAP = 8                # bucketCellCapacity: samples in the inline cell, the rest in the spill list
GROUP_MAX = 512        # svcwin.hip SV_GROUP_MAX: samples of a service a 32-lane group sorts; more: block pass
GROUP_WIN = 32         # svcwin.hip SV_GROUP_WIN: window buckets a group covers; longer windows: block pass
PCTS = [0.001, 1, 50, 75, 90, 95, 99, 99.999]
QS = [1, 1000, 50000, 75000, 90000, 95000, 99000, 99999]
NAN = S.ELAPSED_NAN
INACTIVE = None        # a member that is created and has no bucket row


class SvcSeeded(S.Seeded):
    """Seeded with the sv stream on, on both sides."""

    def __init__(self, C, *a, pcts=PCTS, **kw):
        self.sv = []
        C = copy.deepcopy(C)
        C["gpu"]["serviceWindow"] = {"percentiles": list(pcts)}
        super().__init__(C, *a, **kw)

    def _seed_oracle(self):
        from apmbackend_amd.utils.config import service_window
        super()._seed_oracle()
        self.so.emit_svc = self.sv.append
        self.so.svc_percentiles = service_window(self.C)

    def _seed_engine(self):
        from apmbackend_amd.models import pipeline
        real = pipeline.APMEngine
        pipeline.APMEngine = lambda C, outputs=(): real(C, outputs=tuple(outputs) + ("sv",))
        try:
            super()._seed_engine()
        finally:
            pipeline.APMEngine = real


class Cases:
    """Services and their members.  Member k of a service lives on server jvm<k> unless it names
    another; a server lists its series in case order, members with `late` after all others.  The
    servers are created in index order, so the emission order is server by server."""

    def __init__(self, C, seed):
        self.C, self.labels, self.rng = C, S.window_labels(C), random.Random(seed)
        self.names = []      # services in case order
        self.members = []    # (server index, late, case index, service, bucket dict or INACTIVE)

    def add(self, name, *members, how="spread", late=()):
        """members: sample lists (INACTIVE: created, no bucket row; []: active, count 0)."""
        ci = len(self.names)
        self.names.append("S:" + name)
        for k, vals in enumerate(members):
            b = INACTIVE
            if vals is not INACTIVE:
                b = S.layout(list(vals), self.labels, how, where=ci + k)
                if not vals:
                    b[self.labels[(ci + k) % len(self.labels)]] = []
                b = S.with_decoys(b, self.labels, ci + k)
            self.members.append((k, k in late, ci, "S:" + name, b))
        return ci

    def vals(self, n):
        return S._values(self.rng, n)

    def table(self):
        """(order, buckets) for Seeded: keys server by server, then the trigger (so the series
        count, and with it the service count, is the table's)."""
        order, buckets = [], {}
        for k, _late, _ci, svc, b in sorted(self.members, key=lambda m: m[:3]):
            key = (f"jvm{k:02d}", svc)
            order.append(key)
            if b is not INACTIVE:
                buckets[key] = b
        order.append(S.TRIGGER)
        return order, buckets


def window_samples(C, buckets, key):
    return [v for b in S.window_labels(C) for v in buckets.get(key, {}).get(b, [])]


def reference(C, order, buckets, qs):
    """(rows, {service: (servers, m, nan, sum, sums)}) of the first rollover from the case table alone."""
    edge_ts = (S.LATEST + 1 - S.stats_settings(C)[2] - 1) * 10000
    series = [(key[1], window_samples(C, buckets, key)) for key in order if key in buckets]
    return R.rows_from_series(edge_ts, series, qs)


def check(sd, order, buckets, qs):
    want, ints = reference(sd.C, order, buckets, qs)
    sd.step()
    got = sd.eng.take("sv")
    assert sd.sv == want, "oracle and reference differ: " + str(S.first_difference(sd.sv, want, lambda i: ""))
    diff = S.first_difference(got, want, lambda i: want[i].split("|")[2] if i < len(want) else "")
    assert diff is None, "sv rows: " + diff
    sd.eng.eng.flush()
    dev = sd.eng.eng.svcwins()
    by = {name: (servers, m, nan, total, list(sums)) for name, servers, m, nan, total, sums in dev}
    assert len(by) == len(dev)
    for svc, (servers, m, nan, total, sums) in ints.items():
        g = by[svc]
        assert g[:4] == (servers, m, nan, total), f"{svc}: servers, m, nan, sum {g[:4]}, want {(servers, m, nan, total)}"
        if m:
            assert g[4] == sums, f"{svc}: sums {g[4]}, want {sums}"
    return want, dev


def case_table(C):
    """Every case of the issue, each a service of its own, decoys on both sides of the window in
    every member."""
    T = Cases(C, 1919)
    v = T.vals
    # totals around the group's tile: one member; two members each under the limit; beside a member
    # that is over the limit on its own
    for n in (1, 2, 32, 33, GROUP_MAX - 1, GROUP_MAX, GROUP_MAX + 1):
        T.add(f"tot{n}_single", v(n))
        a = 300 if n == GROUP_MAX + 1 else n - n // 2   # (513 = 300 + 213: deferred by the total)
        T.add(f"tot{n}_split", v(a), v(n - a))
        T.add(f"tot{n}_beside_big", v(GROUP_MAX + 8), v(n))
    # member counts: more members than lanes, members of one sample
    for k in (1, 2, 33, 65):
        T.add(f"members{k}", *[v(1 + (j % 3)) for j in range(k)])
    T.add("members33_deferred", *[v(16 + j % 2) for j in range(33)])        # 33 members, 544 samples
    T.add("union16385", v(8192), v(8193))
    # pairs spanning members
    T.add("split_even_p50", [1, 2, 3, 4], [101, 102, 103, 104])               # m = 8: p50 reads rank 3 alone
    T.add("split_pair_p50", [1, 2, 3, 4], [101, 102, 103])                    # m = 7: p50 reads ranks 3 and 4
    T.add("all_equal", [777] * 20, [777] * 20, [777])
    T.add("minus_one_zero", [-1], [0])                                        # -0.5, sum -1
    T.add("int32_max_group", [S.INT32_MAX] * 100, [S.INT32_MAX] * 100)        # sum beyond 2^32
    T.add("int32_max_block", [S.INT32_MAX] * 200, [S.INT32_MAX] * 200, [S.INT32_MAX] * 200)
    T.add("int32_min_plus1", [NAN + 1, 5], [NAN + 1])
    T.add("int32_min_plus1_block", [NAN + 1] * 300, [NAN + 1] * 300)
    # NaN: inline in one member, in a spill run of another
    T.add("nan_inline_and_spilled", [5, NAN, 7], v(30) + [NAN] + v(9), how="one")
    T.add("nan_block", v(600) + [NAN] * 2, [NAN, 1])
    T.add("only_nan", [NAN] * 3, [NAN])                                       # st rows, no sv row
    T.add("only_nan_block", [NAN] * 520, [NAN])
    T.add("one_finite_among_nan", [NAN, NAN], [NAN, 42, NAN], how="one")
    # membership and order
    T.add("inactive_middle", [1, 2, 3], INACTIVE, [4, 5, 6, 7])
    T.add("inactive_first", INACTIVE, [10, 20], [30])                         # the row stands at the second member
    T.add("inactive_first_block", INACTIVE, v(400), v(400))
    T.add("count0_member", [], [1, 2, 3])
    T.add("count0_only", [], [])                                              # servers 2, m 0: no row
    T.add("all_inactive", INACTIVE, INACTIVE)                                 # no row
    T.add("opposite_a", [1, 2], [3, 4], late=(1,))                            # jvm00: a, b; jvm01: b, a
    T.add("opposite_b", [5, 6], [7, 8])
    # a deferred and a small service in one wave (groups 2 k, 2 k + 1), both parities
    if len(T.names) % 2:
        T.add("pad", [9])
    T.add("even_block", v(400), v(300))
    T.add("odd_group", v(7), v(5))
    T.add("even_group", v(6), v(7))
    T.add("odd_block", v(401), v(300))
    # with the trigger's service (created last) the group count is odd: the last wave's upper half
    # is past the end
    if len(T.names) % 2:
        T.add("tail", v(20), v(3))
    return T


def test_constants_are_the_kernels():
    from apmbackend_amd import _native
    N = _native.load(build_if_missing=False)
    assert N.svcwin_group_max() == GROUP_MAX and N.svcwin_group_win() == GROUP_WIN


def test_one_rollover_all_cases():
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    T = case_table(C)
    order, buckets = T.table()
    assert order.index(("jvm01", "S:opposite_b")) < order.index(("jvm01", "S:opposite_a"))
    assert order.index(("jvm00", "S:opposite_a")) < order.index(("jvm00", "S:opposite_b"))
    sd = SvcSeeded(C, order, buckets)
    want, dev = check(sd, order, buckets, QS)
    by = {r.split("|")[2]: r for r in want}
    # the groups stand in the order of their first member: the case order, then the trigger's
    names = [d[0] for d in dev]
    assert names == T.names + [S.TRIGGER[1]] and len(names) % 2 == 1
    for name, parity in (("even_block", 0), ("odd_group", 1), ("even_group", 0), ("odd_block", 1)):
        assert names.index("S:" + name) % 2 == parity
    assert by["S:minus_one_zero"].endswith("|2|2|0|-1|0.001:-0.5,1:-0.5,50:-1,75:0,90:0,95:0,99:0,99.999:0")
    assert by["S:split_even_p50"].split("|")[3:7] == ["2", "8", "0", "420"] and ",50:4," in by["S:split_even_p50"]
    assert by["S:split_pair_p50"].split("|")[3:7] == ["2", "7", "0", "316"] and ",50:52.5," in by["S:split_pair_p50"]
    assert by["S:int32_max_group"].split("|")[3:7] == ["2", "200", "0", str(200 * S.INT32_MAX)]
    assert by["S:int32_max_block"].split("|")[3:7] == ["3", "600", "0", str(600 * S.INT32_MAX)]
    assert by["S:int32_min_plus1_block"].split("|")[6] == str(600 * (NAN + 1))
    assert by["S:one_finite_among_nan"].endswith("|2|1|4|42|" + ",".join(f"{R.label(q)}:42" for q in QS))
    assert by["S:inactive_middle"].split("|")[3:7] == ["2", "7", "0", "28"]
    assert by["S:inactive_first"].split("|")[3:7] == ["2", "3", "0", "60"]
    assert by["S:count0_member"].split("|")[3:7] == ["2", "3", "0", "6"]
    assert by["S:union16385"].split("|")[3:5] == ["2", "16385"]
    assert by["S:members65"].split("|")[3] == "65" and by["S:members33_deferred"].split("|")[3:5] == ["33", "544"]
    for gone in ("only_nan", "only_nan_block", "count0_only", "all_inactive", "trigger"):
        assert "S:" + gone not in by
    rows = [r.split("|")[2] for r in want]
    assert rows.index("S:opposite_a") < rows.index("S:opposite_b")
    # a service whose first member is inactive prints where its second member stands: behind every
    # service with a row on the first server
    moved = ["S:inactive_first", "S:inactive_first_block"]
    assert rows == [n for n in T.names if n in by and n not in moved] + moved
    dv = {d[0]: d for d in dev}
    assert dv["S:all_inactive"][1:4] == (0, 0, 0) and dv["S:count0_only"][1:4] == (2, 0, 0)
    assert dv["S:only_nan"][1:4] == (2, 0, 4) and dv["S:only_nan_block"][1:4] == (2, 0, 521)
    # the st / fs rows are what an engine without the stream prints, and that engine has no sv state
    plain = S.Seeded(C, order, buckets, reference=False)
    plain.step()
    assert sd.eng.take("st") == plain.eng.take("st") == sd.st
    assert sd.eng.take("fs") == plain.eng.take("fs")
    assert plain.eng.take("sv") == [] and plain.eng.eng.svcwins() == []


def test_long_window_takes_the_block_pass():
    """A window of 40 buckets: longer than a group's 32 lanes, so every service is selected by a block."""
    C = S.seeded_cfg(window=39, buffer=6, cell_cap=CAP)
    assert len(S.window_labels(C)) == 40 > GROUP_WIN
    T = Cases(C, 40)
    v = T.vals
    T.add("one_sample", [], v(1))
    T.add("n33", v(20), v(13))
    T.add("n513", v(300), v(213))
    T.add("nan_long", v(70) + [NAN], [NAN, NAN])
    T.add("ends", v(41), INACTIVE, v(2), how="ends")
    T.add("empty", [], INACTIVE)
    order, buckets = T.table()
    sd = SvcSeeded(C, order, buckets)
    want, dev = check(sd, order, buckets, QS)
    assert [r.split("|")[2:6] for r in want] == [["S:one_sample", "2", "1", "0"], ["S:n33", "2", "33", "0"],
                                                ["S:n513", "2", "513", "0"], ["S:nan_long", "2", "70", "3"],
                                                ["S:ends", "2", "43", "0"]]

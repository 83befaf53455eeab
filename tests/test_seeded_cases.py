"""CPU checks that keep the seeded K8 / K10 case tables (tests/seeded.py) honest."""
import math

import numpy as np
import pytest

import seeded as S
from apmbackend_amd.models import oracle


def test_fraction_ranks_equal_the_js_formula():
    """The independent rank function (exact rationals on p*n/100 - 1) against the oracle's port of
    calcPercentile's double arithmetic, for every n the seeded tests can reach.  Were a double
    quirk of the JS formula to make them differ for some n, the JS behaviour (the oracle) would be
    the specification and that n would have to leave the case tables: none does."""
    ns = list(range(1, 1101)) + [n + d for n in S.BIG_NS + S.LONG_NS for d in (-1, 0, 1) if n + d > 0]
    for n in ns:
        arr = list(range(0, 3 * n, 3))  # distinct, so the value identifies the ranks
        for p in (75, 95):
            lo, hi = S.frac_ranks(n, p)
            assert (lo, hi) == oracle.percentile_ranks(n, p), (n, p)
            assert 0 <= lo <= hi < n
            val = arr[lo] if lo == hi else (arr[lo] + arr[hi]) / 2
            assert val == oracle.calc_percentile(arr, p), (n, p)
    assert S.frac_ranks(0, 75) == oracle.percentile_ranks(0, 75) == (-1, -1)


def test_case_tables_bracket_every_tier_constant():
    def brackets(ns, c):
        return {c - 1, c, c + 1} <= set(ns)
    h2 = S.H2_NS
    assert brackets(h2, 32)      # HW: register network | half_sort_regs<2>
    assert brackets(h2, 64)      # 2 HW: half_sort_regs<2> | <4>
    assert brackets(h2, 128)     # 4 HW: half_sort_regs<4> | <8>
    assert brackets(h2, 256)     # 8 HW: half_sort_regs<8> | <16>
    assert brackets(h2, 512)     # H2_TILE: half_sort_regs<16> | block pass
    assert brackets(h2, 1024)    # WS_TILE (= 2 H2_TILE): inside the block pass for h2
    assert brackets(S.WAVE_NS, 64)     # APM_WAVE: k_window_stats registers | LDS bitonic
    assert brackets(S.WAVE_NS, 1024)   # WS_TILE: LDS bitonic | block pass
    assert brackets(S.BIG_NS, 16384)   # BIG_TILE: block bitonic | radix select
    assert 16385 in S.LONG_NS          # BIG_TILE + 1 through win_slots_ext
    assert (S.HW, S.H2_TILE, S.WS_TILE, S.BIG_TILE) == (32, 512, 1024, 16384)
    # percentile_ranks' integral-index branches (n % 4 == 0 for p75, n % 20 == 0 for p95), n == 1
    # and the "last element" branch are all among the sizes
    assert 1 in h2 and any(n % 20 == 0 and n for n in h2) and any(n % 4 == 0 and n % 20 for n in h2)
    assert any(0 < n and S.frac_ranks(n, 95)[0] == n - 1 and (95 * n) % 100 for n in h2)
    assert S.tier_name("h2", 32) != S.tier_name("h2", 33) != S.tier_name("h2", 65) and \
        S.tier_name("h2", 512) != S.tier_name("h2", 513) and S.tier_name("h2", 16384) != S.tier_name("h2", 16385)


def test_layouts_keep_every_sample_and_use_both_ends():
    C = S.seeded_cfg(window=70)
    labels = S.window_labels(C)
    assert len(labels) == 71
    for n in (0, 1, 2, 33, 71, 513):
        for how in ("one", "spread", "ends"):
            b = S.layout(list(range(n)), labels, how, where=5)
            assert sorted(v for x in b.values() for v in x) == list(range(n))
            assert set(b) <= set(labels)
            if how != "one" and n >= 2:
                assert b[labels[0]] and b[labels[-1]]
    d = S.with_decoys({}, labels)
    assert set(d) == {labels[0] - 1, labels[-1] + 1} == d.decoys


def test_window_reference_counts_only_the_window():
    """The Fraction reference and the oracle on a hand-made window with decoys on both sides."""
    C = S.seeded_cfg()
    labels = S.window_labels(C)
    k = S.key("x")
    b = S.with_decoys({labels[0]: [4, 1], labels[-1]: [3, 2]}, labels)
    sd = S.Seeded(C, [k], {k: b}, device=False)
    want, rows = sd.want_winstats()
    assert want[0] == S.Want(1, 4, 0.77, 2.5, 3.0, 4.0) and want[1].active == 0
    sd.step()
    assert sd.st == rows == [f"st|{(S.LATEST - 6) * 10000}|jvm00|S:x|0.77|2.5|3.0|4.0"]


def test_zscore_precondition_guard_rejects_a_bad_history():
    S.assert_half_multiples([0.0, 0.5, 127.5, None, float("nan"), 16.0])
    for bad in (0.3, 128.0, -0.5, 16.25):
        with pytest.raises(AssertionError):
            S.assert_half_multiples([16.0, bad])
    overrides, order, buckets, histories, _fed = S.zscore_case()
    histories[order[3]][6][0][2] = 0.3
    sd = S.Seeded(S.seeded_cfg(lags=S.Z_DEFAULTS, max_series=S.Z_MAX_SERIES, overrides=overrides), order, buckets,
                  histories, device=False)
    with pytest.raises(AssertionError):
        S.assert_half_multiples(sd.history_values())


def test_zscore_case_table_meets_its_precondition_and_its_shape():
    st, fs, final = S.zscore_reference()  # asserts the precondition on every appended value
    overrides, order, _buckets, histories, _fed = S.zscore_case()
    assert len(order) + 1 == S.Z_SERIES and S.Z_STEPS == 135
    assert [-(-lag // 64) for lag in S.Z_LAGS] == [1, 1, 1, 2, 3]  # per = ceil(LAG / RS_PARTS)
    lens = {k[1]: len(histories[k][130][0]) for k in order}
    assert lens["S:len0"] == 0 and lens["S:lenLm1"] == 129 and lens["S:lenL"] == 130
    rows = {}
    for l in fs:
        f = l.split("|")
        rows.setdefault((f[3], f[4]), []).append(l)
    # length LAG - 1: no mean at the first rollover, the first one at the second; length LAG: at once
    assert ":undefined:" in rows[("S:lenLm1", "130")][0] and ":undefined:" not in rows[("S:lenLm1", "130")][1]
    assert ":undefined:" not in rows[("S:lenL", "130")][0]
    # exactly on the bound does not signal, half a unit above does; both directions occur
    assert rows[("S:on_bound", "64")][0].endswith("24.0:16.0:8.0:24.0:0.0")
    assert "|24.5:16.0:8.0:24.0:1|" in rows[("S:over_bound_i1", "64")][0]
    sigs = {p.split(":")[4] for l in fs for p in l.split("|")[6:9]}
    assert {"1", "-1", "0", "1.0", "-1.0", "0.0"} <= sigs
    assert all(len(v) == S.Z_STEPS for (svc, _lag), v in rows.items() if svc != S.TRIGGER[1])
    assert len(st) * len(S.Z_LAGS) == len(fs)
    assert all(len(final[k][lag][0]) == min(lag, S.Z_STEPS + len(histories[k][lag][0])) for k in order for lag in S.Z_LAGS)


def test_bf16_round_to_nearest_even_helper():
    table = [
        (0x3F800000, 0x3F80),  # 1.0
        (0x3F807FFF, 0x3F80),  # just below the tie: down
        (0x3F808000, 0x3F80),  # tie, even below: down
        (0x3F808001, 0x3F81),  # just above the tie: up
        (0x3F818000, 0x3F82),  # tie, odd below: up to even
        (0x437F8000, 0x4380),  # 255.5: tie, the carry runs into the exponent (256)
        (0x3FFFFFFF, 0x4000),  # carry through the whole mantissa into the exponent (2.0)
        (0x7F7FFFFF, 0x7F80),  # the largest float rounds to infinity
        (0x7F800000, 0x7F80),  # infinity stays
        (0x7FC00000, 0x7FC0),  # quiet NaN
        (0x7F800001, 0x7FC0),  # a NaN whose payload would be rounded away stays NaN
        (0xFFC00000, 0x7FC0),  # negative NaN: canonical
        (0x80000000, 0x8000),  # -0
        (0xBF808000, 0xBF80),  # negative tie to even
        (0x00000000, 0x0000),
    ]
    got = S.bf16_bits_rne(np.array([a for a, _b in table], dtype=np.uint32))
    assert [int(x) for x in got] == [b for _a, b in table]
    r = S.ring_rounded([255.5, 256.5, 100.3, 255.9, 1e-3, 16.0, 127.5], "bfloat16")
    assert list(r[:2]) == [256.0, 256.0] and r[3] == 256.0 and r[5] == 16.0 and r[6] == 127.5
    assert r[2] == 100.5 and abs(r[4] - 1e-3) < 1e-3 * 2 ** -8
    assert S.ring_rounded([1.99999999], "float32")[0] == 2.0
    assert np.isnan(S.ring_rounded([float("nan")], "bfloat16")[0])
    assert S.ring_rounded([100.3], "float64")[0] == 100.3


# ------------------------------------------------------------------------------- K12 tables

def test_host_to_fixed_matches_decimal_on_the_number_table():
    """The host's js::to_fixed prints the whole number-printer table as Decimal does."""
    import format_cases as F
    from apmbackend_amd import _native
    N = _native.load(build_if_missing=False)
    for f in (1, 2):
        bad = [(x, g, w) for x in F.number_table()
               for g, w in [(N.js_to_fixed(x, f), F.jsfmt.to_fixed(x, f))] if g != w]
        assert not bad, bad[:5]


def test_number_table_flag_domains_and_boundaries():
    """The number-printer table: under 1 % of it may raise a flag and every boundary the printer
    branches on is in it (pure Python)."""
    import format_cases as F
    xs = F.number_table()
    assert len(xs) > 80000 and all(isinstance(x, float) for x in xs)
    have = set(x for x in xs if x == x)
    for x in (0.0, 5e-324, 0.04, -0.04, 0.125, 429496729.5, 42949672.95, 429496729.6, 42949672.96, 4294967296.0,
              2147483647.0, -2147483648.0, F.TWO52 / 10, F.TWO52 / 100, F.TWO52, F.TWO52 + 1, 2.0 ** 51 + 0.5,
              F.TWO53 - 1, F.TWO53, F.TWO53 + 2, 99999999999999.9, 1e14, 9999999999999.99, 1e13, 1e21,
              F.TWO127, 1.7976931348623157e308, F.INF, -F.INF):
        assert x in have, x
    assert any(math.copysign(1, x) < 0 and x == 0 for x in xs) and any(x != x for x in xs)
    for b in (429496729.5, 4294967296.0, F.TWO52 / 10, 1e21, F.TWO127):
        assert math.nextafter(b, 0.0) in have and math.nextafter(b, F.INF) in have
    assert F.fixed_nn(429496729.5, 1) == 2 ** 32 - 1 and F.fixed_nn(42949672.96, 2) == 2 ** 32
    assert F.fixed_nn(2147483647.0, 1) == 21474836470 > 0xffffffff
    assert F.ref_number(-0.04, 1, "nf") == "-0.0" and F.ref_number(-0.04, 1, "json") == "0"
    assert F.ref_number(0.125, 2, "nf") == "0.13" and F.ref_number(F.NAN, 1, "copy") == "\\N"
    assert F.ref_number(1e21, 1, "nf") == "1e+21" and F.ref_number(math.nextafter(1e21, 0), 2, "nf") == "999999999999999868928.00"
    for f in (1, 2):
        for mode in F.MODES:
            k = sum(F.may_flag(x, f, mode) for x in xs)
            assert 0 < k < len(xs) // 100, (mode, f, k)
        assert F.may_flag(99999999999999.9, f, "json") == (f == 2) and not F.may_flag(99999999999999.9, f, "nf")


def test_fleet_case_table_covers_the_row_formatter():
    import format_cases as F
    kept, tried = F.random_stats()
    assert tried >= 1000 and len(kept) * 100 >= tried * 99  # at most 1 % print differently fused / unfused
    assert all(1.0 <= s / n <= 1e4 for n, s, _q in kept)
    for i in range(50):  # the exact class: mean a multiple of 0.5, a dyadic sd, identical three ways
        n, s, q = F.exact_stat(i)
        (me, se), (m1, s1), (m2, s2) = F.stat_three_ways(n, s, q)
        assert m1 == m2 == float(me) and (m1 * 2).is_integer() and s1 == s2 == float(se) and (s1 * 4).is_integer()
    cases = {c.label: c for c in F.fleet_cases()}
    assert {cases[f"rows{r}"].n_rows() for r in (1, 15, 16, 17, 1040, 1056)} == {1, 15, 16, 17, 1040, 1056}
    for c in cases.values():
        for copy in (False, True):  # every input prints identically three ways (asserted inside)
            assert len(c.expected(copy)) > 0
    waves = lambda c: -(-c.n_rows() // F.FLEET_RPW)
    # 65 waves: the last one adds 64 totals, one per lane; 66: lane 0 of the last takes a second trip
    assert waves(cases["rows1040"]) == F.WAVE + 1 and waves(cases["rows1056"]) == F.WAVE + 2
    for label in ("rows1040", "rows1056"):
        lens = cases[label].row_lens(False)
        assert lens[0] == lens[1] == 0 and lens[-1] == lens[-2] == 0          # no row at the start / end
        assert not any(lens[16:32]) and all(lens[32:48])                      # a whole wave without rows
        assert any(a > 0 and b == 0 for a, b in zip(lens[0::2], lens[1::2]))  # one LAG of a slot only
        rows = cases[label].expected(False).split(b"\n")[:-1]
        lag_of = [int(r.split(b"|")[3]) for r in rows]
        assert cases[label].lag_values == [30, 6] and lag_of[:2] == [6, 30]   # emitted ascending
    assert cases["slice"].slot_lo > 0 and cases["slice"].slot_lo + cases["slice"].n_slots < len(cases["slice"].names)
    assert b"svc0006" not in cases["slice"].expected(False) and b"svc0007" in cases["slice"].expected(False)
    u = cases["undefined"]
    assert b":undefined|" in u.expected(False) and b'"per75mean":null,"per75std":null' in u.expected(True)
    ln = cases["long_names"]
    lens = ln.row_lens(True)
    assert sum(lens[:16]) > F.FLEET_LDS and 0 < sum(lens[16:]) <= F.FLEET_LDS  # wave 0 direct, wave 1 staged
    assert b"\\\\a\\tb\\rc\\nd" in ln.expected(True) and b"\\a\tb\rc\nd" in ln.expected(False)
    big = cases["big_counts"].expected(False).split(b"\n")[:-1]
    ns = [int(r.split(b"|")[4]) for r in big]
    assert any(2 ** 32 <= n < 10 ** 8 * (2 ** 32 - 1) for n in ns) and any(n >= 10 ** 8 * (2 ** 32 - 1) for n in ns)
    assert max(ns) > 10 ** 10 and b"|2147483647|" in big[1]


def test_format_case_table_covers_the_line_writer():
    cases = {c.label: c for c in S.format_cases()}
    assert {c.n for c in cases.values()} >= {1, 63, 64, 65, 129}
    assert {c.n_lags for c in cases.values()} == {1, 2, 3}
    assert {(c.n, c.n_lags) for c in cases.values()} >= {(63, 2), (64, 3), (65, 1), (65, 2), (65, 3), (129, 1), (129, 2)}
    stages, starts, name_mod, cap_mod, direct = set(), {"st": set(), "fs": set()}, set(), set(), 0
    for c in cases.values():
        assert c.order[-1] == S.TRIGGER and c.n == len(c.order) <= 200
        offs = c.name_offsets()
        assert offs[S.SERVER if c.n > 1 else S.TRIGGER[0]] == 0  # the first name of the table
        name_mod |= {o % 16 for o in offs.values()}
        longest = c.max_name_len()
        if c.n == 65:
            cap_mod.add(c.n * (176 + longest) % 4)
        for r in range(2):
            st, fs = c.line_lens(r)
            # the output bounds of Engine::format_rollover_text hold for every line
            assert max(st) <= 176 + longest and max(fs) <= (720 + 2 * longest if c.copy else 560 + longest)
            stage = c.stage(r)
            stages.add(stage)
            for kind, lens in (("st", st), ("fs", fs)):
                at = 0
                for x in lens:
                    if x:
                        starts[kind].add(at % 4)
                    at += x
                direct += sum(S.block_is_direct(g0, g1, stage) for g0, g1 in S.block_ranges(lens))
        # the oracle's mean / lb / ub of the LAG 2 rows at the first rollover are the seeded v
        for k, v3 in c.hist_v.items():
            for v in v3:
                _infl, avg, lb, ub, _sig = oracle.process_zscore_stats(2, 0.0, 0.0, 1.0, [v, v])
                same = lambda a, b: np.float64(a).tobytes() == np.float64(b).tobytes()
                assert same(avg, v) and (same(lb, v) and same(ub, v) if v > 0 else lb is None and ub is None), (k, v)
    # values inside the printer's flag domain: none, but for one COPY value of 16 digits
    assert sorted(c.flag_count() for c in cases.values()) == [0] * (len(cases) - 1) + [1]
    assert stages == set(S.FMT_STAGES)
    assert {c.stage(1) for c in cases.values()} == set(S.FMT_STAGES)  # each one chosen by a hint, too
    assert direct >= 2 and starts == {"st": {0, 1, 2, 3}, "fs": {0, 1, 2, 3}}
    assert name_mod == set(range(16)) and cap_mod == {0, 1, 2, 3}
    assert (S.fmt_stage(0), S.fmt_stage(7168), S.fmt_stage(7169), S.fmt_stage(12800), S.fmt_stage(12801),
            S.fmt_stage(16896), S.fmt_stage(16897)) == (12288, 8192, 12288, 12288, 16384, 16384, 24576)
    # inactive series: the first, the last (the trigger at the first rollover), a single one
    # between active ones, a whole aligned 64-line block
    assert cases["n63"].line_lens(0)[0][0] == 0 and all(cases["n63"].line_lens(0)[0][29:32:2]) and \
        cases["n63"].line_lens(0)[0][30] == 0
    assert all(c.line_lens(0)[0][-1] == 0 and c.line_lens(1)[0][-1] > 0 for c in cases.values())
    holes = cases["n129_holes"].line_lens(1)[0]
    assert not any(holes[64:128]) and all(holes[1:17]) and holes[128] > 0
    g = S.block_ranges(holes)[1]
    assert g[0] == g[1]  # that block's byte range is empty
    # short names, COPY escapes, NaN and empty windows, the int32 limits, the widest values
    assert (S.SERVER, "") in cases["n63"].order and (S.SERVER, "Q") in cases["n63"].order
    cp = cases["n129_copy"].expected(0)[1]
    assert b"\\\\" in cp and b"\\t" in cp and b"\\r" in cp and b"\\n" in cp and b'"average":null' in cp
    assert cp.count(b"\n") == len(cases["n129_copy"].expected_rows(0)[1])  # escaped in COPY rows ...
    st0 = cases["n129_copy"].expected_rows(0)[0]
    assert any(r.count(b"\n") == 2 for r in st0)                           # ... raw in the st rows
    text = b"".join(cases["n65_names200"].expected(0))
    assert b"|2147483647.0|" in text and b"-2147483647.0" in text and b"|undefined|" in text
    assert b":-999999999999999868928.0:undefined:undefined:" in text and text.count(b":999999999999999868928.0") >= 6
    assert b"1.7014118346046921e+38" in cp

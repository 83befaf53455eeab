"""CPU checks that keep the seeded K8 / K10 case tables (tests/seeded.py) honest."""
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

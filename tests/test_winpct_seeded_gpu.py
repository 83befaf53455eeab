"""K16 wp rows (winpct.hip) on seeded engine state: one engine, one rollover, every case a series of
its own (tests/seeded.py).  The engine's rows must equal the CPU oracle's and a reference that
shares no code with either (tests/winpct_ref.py: sorted() + Fraction ranks + integer halves), byte
for byte, and winpcts() the reference's integers."""
import collections
import copy
import random

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import seeded as S  # noqa: E402
import winpct_ref as R  # noqa: E402

CAP = 8                # bucketCellCapacity: samples in the inline cell, the rest in the spill list
GROUP_MAX = 512        # winpct.hip WP_GROUP_MAX: samples a 32-lane group sorts; more go to the block pass
GROUP_WIN = 32         # winpct.hip WP_GROUP_WIN: window buckets a group covers; longer windows: block pass
PCTS = [0.001, 1, 50, 75, 90, 95, 99, 99.999]
QS = [1, 1000, 50000, 75000, 90000, 95000, 99000, 99999]
NAN = S.ELAPSED_NAN


class PctSeeded(S.Seeded):
    """Seeded with the wp stream on, on both sides."""

    def __init__(self, C, *a, pcts=PCTS, **kw):
        self.wp = []
        C = copy.deepcopy(C)
        C["gpu"]["windowPercentiles"] = list(pcts)
        super().__init__(C, *a, **kw)

    def _seed_oracle(self):
        from apmbackend_amd.utils.config import window_percentiles
        super()._seed_oracle()
        self.so.emit_pct = self.wp.append
        self.so.percentiles = window_percentiles(self.C)

    def _seed_engine(self):
        from apmbackend_amd.models import pipeline
        real = pipeline.APMEngine
        pipeline.APMEngine = lambda C, outputs=(): real(C, outputs=tuple(outputs) + ("wp",))
        try:
            super()._seed_engine()
        finally:
            pipeline.APMEngine = real


def window_samples(C, buckets, key):
    return [v for b in S.window_labels(C) for v in buckets.get(key, {}).get(b, [])]


def reference(C, order, buckets, qs):
    """(rows, per series id (m, nan, sums)) of the first rollover from the case table alone."""
    edge_ts = (S.LATEST + 1 - S.stats_settings(C)[2] - 1) * 10000
    rows, ints = [], []
    for key in order:
        vals = window_samples(C, buckets, key)
        ints.append(R.window_sums(vals, qs))
        if key in buckets:
            r = R.row(edge_ts, key[0], key[1], vals, qs)
            if r is not None:
                rows.append(r)
    return rows, ints


def check(sd, order, buckets, qs, names):
    want, ints = reference(sd.C, order, buckets, qs)
    sd.step()
    got = sd.eng.take("wp")
    assert sd.wp == want, "oracle and reference differ: " + str(S.first_difference(sd.wp, want, lambda i: ""))
    diff = S.first_difference(got, want, lambda i: want[i].split("|")[3] if i < len(want) else "")
    assert diff is None, "wp rows: " + diff
    sd.eng.eng.flush()
    dev = sd.eng.eng.winpcts()
    assert len(dev) >= len(order)
    for i, (m, nan, sums) in enumerate(ints):
        gm, gn, gs = dev[i]
        assert (gm, gn) == (m, nan), f"series {i} ({names[i]}): m, nan {gm, gn}, want {m, nan}"
        if m:
            assert list(gs) == sums, f"series {i} ({names[i]}): sums {list(gs)}, want {sums}"
    return want


def case_table(C):
    """(order, buckets, names): every case of the issue, each its own series, decoys on both sides
    of the window everywhere."""
    labels = S.window_labels(C)
    rng = random.Random(1616)
    order, buckets, names, sizes = S.sized_cases(C, S.H2_NS + S.BIG_NS, ("spread",), seed=16)

    def add(name, vals, how="spread", decoys=True):
        b = S.layout(list(vals), labels, how, where=len(order))
        if not vals:
            b[labels[len(order) % len(labels)]] = []
        return S.add_series(order, buckets, names, sizes, name, S.with_decoys(b, labels, len(order)) if decoys else b)

    # values
    add("all_equal", [777] * 40)
    for k in (1, 2, 33, GROUP_MAX + 88):
        add(f"int32_max_x{k}", [S.INT32_MAX] * k)                    # the int64 sum: 2 * INT32_MAX
    add("minus_one_zero", [-1, 0])                                     # -0.5
    add("extremes", [NAN + 1, S.INT32_MAX])
    add("extremes_block", [NAN + 1, S.INT32_MAX] * 300)
    add("two_samples", [10, 21])                                       # non-integral index: the pair's mean
    # NaN
    add("nan_inline", [5, NAN, 7], how="one")
    add("nan_spilled", S._values(rng, 30) + [NAN] + S._values(rng, 9), how="one")
    add("nan_block", S._values(rng, 600) + [NAN] * 2 + S._values(rng, 50))
    add("only_nan", [NAN] * 3)                                         # st row, no wp row
    add("one_finite_two_nan", [NAN, 42, NAN], how="one")
    # layout: an inactive id and an n == 0 series between reporting ones
    add("before_gap", [1, 2, 3])
    order.append(S.key("inactive")); names.append("inactive"); sizes.append(0)
    add("count0", [])
    add("after_gap", [4, 5, 6] * 5)
    # two series sharing a wave (ids 2k, 2k + 1), one of them deferred to the block pass: both parities
    if len(order) % 2:
        add("pad", [9])
    add("even_block", S._values(rng, 700))
    add("odd_group", S._values(rng, 12))
    add("even_group", S._values(rng, 13))
    add("odd_block", S._values(rng, 701))
    add("no_decoys", S._values(rng, 40), decoys=False)
    order.append(S.TRIGGER); names.append("trigger"); sizes.append(0)
    add("last_id_spills", S._values(rng, 100), how="one")
    if len(order) % 2 == 0:
        add("odd_tail", S._values(rng, 20))
    assert len(order) % 2 == 1, "the last wave's upper half must be past n_series"
    return order, buckets, names


def test_constants_are_the_kernels():
    from apmbackend_amd import _native
    N = _native.load(build_if_missing=False)
    assert N.winpct_group_max() == GROUP_MAX == S.H2_TILE and N.winpct_group_win() == GROUP_WIN == S.HW


def test_one_rollover_all_cases():
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    order, buckets, names = case_table(C)
    sd = PctSeeded(C, order, buckets)
    want = check(sd, order, buckets, QS, names)
    by = {r.split("|")[3]: r for r in want}
    assert by["S:minus_one_zero"].endswith("|2|0|0.001:-0.5,1:-0.5,50:-1,75:0,90:0,95:0,99:0,99.999:0")
    assert by["S:int32_max_x2"].endswith("|2|0|" + ",".join(f"{R.label(q)}:2147483647" for q in QS))
    assert by["S:extremes"].endswith("|2|0|0.001:0,1:0,50:-2147483647,75:2147483647,90:2147483647,95:2147483647,"
                                     "99:2147483647,99.999:2147483647")
    assert by["S:two_samples"].endswith("|2|0|0.001:15.5,1:15.5,50:10,75:21,90:21,95:21,99:21,99.999:21")
    assert by["S:one_finite_two_nan"].endswith("|1|2|" + ",".join(f"{R.label(q)}:42" for q in QS))
    assert "S:only_nan" not in by and "S:count0" not in by and "S:inactive" not in by and "S:n0_spread" not in by
    assert "|650|2|" in by["S:nan_block"]
    # the st / fs rows are what an engine without the stream prints
    plain = S.Seeded(C, order, buckets, reference=False)
    plain.step()
    assert sd.eng.take("st") == plain.eng.take("st") == sd.st
    assert sd.eng.take("fs") == plain.eng.take("fs")
    assert plain.eng.take("wp") == [] and plain.eng.eng.winpcts() == []


def test_agreement_with_st():
    """List [75, 95]: for every case without a NaN sample the wp values are the st row's p75 / p95
    as numbers -- the new kernel against K8 at every path boundary."""
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    order, buckets, names = case_table(C)
    sd = PctSeeded(C, order, buckets, pcts=[75, 95], reference=False)
    sd.step()
    wp = {tuple(r.split("|")[2:4]): r.split("|") for r in sd.eng.take("wp")}
    st = {tuple(r.split("|")[2:4]): r.split("|") for r in sd.eng.take("st")}
    checked = 0
    for key in order:
        vals = window_samples(C, buckets, key)
        if key not in buckets or not vals or NAN in vals:
            continue
        w, s = wp[key], st[key]
        assert int(w[4]) == len(vals) and w[5] == "0"
        p = dict(x.split(":") for x in w[6].split(","))
        assert list(p) == ["75", "95"]
        assert (float(p["75"]), float(p["95"])) == (float(s[6]), float(s[7])), (key, w, s)
        checked += 1
    assert checked >= len(S.H2_NS) + len(S.BIG_NS) + 10


@pytest.mark.parametrize("window", [39, 89])
def test_long_windows_take_the_block_pass(window):
    """Windows of 40 and 90 buckets (33 to 64, and more than K8_INLINE_SLOTS): longer than a
    group's 32 lanes, so every series is selected by a block."""
    C = S.seeded_cfg(window=window, buffer=6, cell_cap=CAP)
    labels = S.window_labels(C)
    assert len(labels) == window + 1 > GROUP_WIN
    order, buckets, names, _sizes = S.sized_cases(C, S.LONG_NS, ("spread",), seed=window)
    rng = random.Random(window)
    S.add_series(order, buckets, names, _sizes, "nan_long",
                 S.with_decoys(S.layout(S._values(rng, 70) + [NAN], labels, "spread"), labels, 3))
    S.add_series(order, buckets, names, _sizes, "ends",
                 S.with_decoys(S.layout(S._values(rng, 41), labels, "ends"), labels, 4))
    sd = PctSeeded(C, order, buckets)
    want = check(sd, order, buckets, QS, names)
    assert len(want) == len(order) - 1  # (n = 0 prints no row)

"""K8 window statistics on seeded engine state: every tier boundary of stats.hip, every pairing
of wave halves, the window's bucket range and the spill runs, one engine and one rollover per
case (tests/seeded.py).  winstats() is compared field by field for exact equality of doubles and
the st rows byte for byte, against the CPU oracle and an independent Fraction reference that must
agree with each other first.  No tolerance anywhere: the samples are integers."""
import collections
import random

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import seeded as S  # noqa: E402


def _present(want, sizes):
    """Every listed n is in the engine's output (no case dropped on the way)."""
    got = collections.Counter(w.n for w in want if w.active)
    need = collections.Counter(sizes)
    assert all(got[n] >= c for n, c in need.items()), (need - got)


def test_h2_tier_boundaries():
    """k_window_stats_h2 (window 31: 32 window buckets, two series per wave): n on both sides of
    every tier edge (register network <= 32, half_sort_regs<2|4|8|16> <= 64|128|256|512, block
    pass above), each n all in one bucket (all but 8 samples spill), spread evenly, and in the
    oldest + newest window bucket only; decoy buckets just outside both ends of the window."""
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=8)
    order, buckets, names, sizes = S.sized_cases(C, S.H2_NS, ("one", "spread", "ends"), seed=101)
    labels = S.window_labels(C)
    rng = random.Random(5)
    S.add_series(order, buckets, names, sizes, "all_equal", S.with_decoys(S.layout([777] * 100, labels, "spread"), labels))
    S.add_series(order, buckets, names, sizes, "int32_max",
                 S.with_decoys(S.layout(S._values(rng, 39) + [S.INT32_MAX], labels, "one", 7), labels))
    S.add_series(order, buckets, names, sizes, "negatives",
                 S.with_decoys(S.layout(S._values(rng, 70, -50, -1), labels, "ends"), labels))
    sd = S.Seeded(C, order, buckets)
    want = S.check_k8(sd, "h2", names)
    _present(want, sizes)
    assert len([w for w in want if w.active]) == 3 * len(S.H2_NS) + 3


def test_h2_wave_neighbours():
    """The two halves of a wave (series ids 2k, 2k + 1) in different tiers and states: every
    cross-lane step runs for both whatever each half does.  Inactive ids: created with
    import_series and given no bucket row (import_buckets marks only the series of its rows
    active; the trigger series, listed first, is such an id until its first tx)."""
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=8)
    labels = S.window_labels(C)
    rng = random.Random(77)
    order, buckets, names, sizes = [], {}, [], []

    def add(name, n, how, where=0, nan_at=None):
        vals = S._values(rng, n)
        if nan_at is not None:
            vals[nan_at] = S.ELAPSED_NAN
        S.add_series(order, buckets, names, sizes, name, S.with_decoys(S.layout(vals, labels, how, where), labels, len(order)))

    def inactive(k, name):
        order.append(k); names.append(name); sizes.append(None)

    inactive(S.TRIGGER, "inactive (trigger)"); add("w0_n64", 64, "spread")            # inactive | <2>
    add("w1_reg20", 20, "spread"); add("w1_regs16", 400, "spread")                    # register | <16>
    add("w2_block600", 600, "spread"); add("w2_reg5", 5, "ends")                      # block pass | register
    add("w3_nan10", 10, "spread", nan_at=4); add("w3_n33", 33, "spread")              # NaN window | <2>
    add("w4_spill30", 30, "one", 3); add("w4_inline30", 30, "spread")                 # spilling | not
    add("w5_regs16_512", 512, "ends"); add("w5_n33", 33, "one", 9)                    # <16> | <2>
    add("w6_n33", 33, "ends"); add("w6_nan40_spilled", 40, "one", 11, nan_at=30)      # <2> | NaN in a spill run
    add("w7_n64", 64, "one", 13); inactive(S.key("w7_inactive"), "inactive (no row)")  # <2> | inactive
    add("w8_block513", 513, "spread"); add("w8_block700", 700, "one", 15)             # block | block
    add("w9_empty", 0, "spread"); add("w9_regs4", 100, "spread")                      # empty | <4>
    buckets[S.key("w9_empty")][labels[5]] = []
    add("w10_regs8", 200, "ends")                                                     # <8> | past n_series
    assert len(order) % 2 == 1, "the last wave's upper half must be past n_series"
    sd = S.Seeded(C, order, buckets)
    want = S.check_k8(sd, "h2", names)
    assert [w.active for w in want] == [0 if n is None else 1 for n in sizes]
    assert [w.n for w in want if w.active] == [n for n in sizes if n is not None]


def _straddling(n, rng):
    """n samples whose p75 and p95 order statistics sit inside runs of equal keys, with negatives
    and with runs on both sides of a byte boundary of the sign-flipped radix key."""
    lo75, _ = S.frac_ranks(n, 75)
    lo95, _ = S.frac_ranks(n, 95)
    vals = [rng.choice((-50, -1, 0, 255, 256, 65535)) for _ in range(lo75 - 40)]
    vals += [65536] * 80                                  # the p75 ranks are inside this run
    vals += [rng.choice((65537, 2 ** 24 - 1)) for _ in range(lo95 - 30 - len(vals))]
    vals += [2 ** 24] * 60                                # ... and the p95 ranks inside this one
    vals += [rng.choice((2 ** 24 + 1, 10 ** 9)) for _ in range(n - len(vals))]
    assert len(vals) == n
    s = sorted(vals)
    assert s[lo75 - 1] == s[lo75 + 2] == 65536 and s[lo95 - 1] == s[lo95 + 2] == 2 ** 24
    rng.shuffle(vals)
    return vals


def test_big_pass_boundaries():
    """k_window_stats_big: block bitonic up to BIG_TILE = 16384 samples, 4-pass radix select
    above; 16384 and 16385 exactly, once all in one bucket and once spread."""
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=8)
    labels = S.window_labels(C)
    rng = random.Random(3)
    order, buckets, names, sizes = [], {}, [], []
    for n in S.BIG_NS:
        for how in ("one", "spread"):
            S.add_series(order, buckets, names, sizes, f"n{n}_{how}",
                         S.with_decoys(S.layout(_straddling(n, rng), labels, how, len(order) * 3), labels, len(order)))
        # ... and once with distinct samples: inside a run of equal keys a rank that is one off
        # reads the same value
        S.add_series(order, buckets, names, sizes, f"n{n}_distinct",
                     S.with_decoys(S.layout(rng.sample(range(-10 ** 6, 10 ** 9), n), labels, "spread"), labels, len(order)))
    sd = S.Seeded(C, order, buckets)
    want = S.check_k8(sd, "h2", names)
    _present(want, sizes)


def test_wave_kernel_tiers():
    """k_window_stats (window 40: 41 window buckets, one series per wave): registers up to 64
    samples, LDS bitonic up to WS_TILE = 1024, block pass above; a spilling and a NaN series."""
    C = S.seeded_cfg(window=40, buffer=6, cell_cap=8)
    labels = S.window_labels(C)
    assert len(labels) == 41
    order, buckets, names, sizes = S.sized_cases(C, S.WAVE_NS, ("spread",), seed=41)
    rng = random.Random(9)
    S.add_series(order, buckets, names, sizes, "spilling",
                 S.with_decoys(S.layout(S._values(rng, 100), labels, "one", 40), labels))
    vals = S._values(rng, 70)
    vals[33] = S.ELAPSED_NAN
    S.add_series(order, buckets, names, sizes, "nan", S.with_decoys(S.layout(vals, labels, "spread"), labels))
    sd = S.Seeded(C, order, buckets)
    want = S.check_k8(sd, "wave", names)
    _present(want, sizes)


def test_long_window_all_block_pass():
    """A window of 71 buckets (> 64, and > K8_INLINE_SLOTS: the slots come from win_slots_ext):
    every series goes to the block pass, samples in every bucket including the first and last."""
    C = S.seeded_cfg(window=70, buffer=6, cell_cap=8)
    labels = S.window_labels(C)
    assert len(labels) == 71 > S.K8_INLINE_SLOTS
    order, buckets, names, sizes = S.sized_cases(C, S.LONG_NS, ("spread",), seed=71)
    for k, n in zip(order, sizes):
        if n >= 33:
            assert buckets[k][labels[0]] and buckets[k][labels[-1]]
        if n >= 513:
            assert all(buckets[k][b] for b in labels)
    assert buckets[S.key("n1_spread")][labels[-1]]  # the one sample sits in the last (ext) slot
    sd = S.Seeded(C, order, buckets)
    want = S.check_k8(sd, "block", names)
    _present(want, sizes)


def test_spill_runs():
    """The binary search for a series' run in a slot's sorted spill list: series id 0, the largest
    id and ids in between spill 1, 8, 9 and 1000 samples in one bucket, a second bucket has an
    empty spill list, a third another mixture.  Every series' values are its own (id * 10^4 + ...),
    so a run that starts or ends one entry off changes its statistics."""
    cap = 8
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=cap, max_series=64)
    labels = S.window_labels(C)
    b1, b2, b3 = labels[4], labels[17], labels[29]
    spills1 = {0: 1, 2: 8, 3: 0, 5: 9, 6: 1000, 9: 8, 10: 1000, 11: 1, 14: 9}
    spills3 = {0: 9, 1: 1, 6: 8, 13: 1000, 14: 1}
    rng = random.Random(13)
    order, buckets, names, sizes = [], {}, [], []
    for i in range(15):
        if i == 7:  # the trigger series in the middle: the largest id is a spilling one
            order.append(S.TRIGGER); names.append("inactive (trigger)"); sizes.append(None)
            continue
        mine = lambda m: [i * 10000 + rng.randint(0, 5000) for _ in range(m)]
        b = collections.OrderedDict()
        if i in spills1:
            b[b1] = mine(cap + spills1[i])
        elif i % 2:
            b[b1] = mine(3)
        b[b2] = mine(rng.randint(1, cap))          # nobody spills here
        if i in spills3:
            b[b3] = mine(cap + spills3[i])
        S.add_series(order, buckets, names, sizes, f"id{i}", S.with_decoys(b, labels, i))
    assert order[-1] != S.TRIGGER and len(buckets[order[-1]][b1]) == cap + 9
    sd = S.Seeded(C, order, buckets)
    want = S.check_k8(sd, "h2", names)
    assert [w.n for w in want if w.active] == [n for n in sizes if n is not None]

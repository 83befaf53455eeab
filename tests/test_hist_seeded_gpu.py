"""K15 lh rows (hist.hip) on seeded engine state: one engine, one rollover, every case a series of
its own (tests/seeded.py).  The reported bucket is LATEST + 1 - buffer.  The engine's rows must equal
the CPU oracle's and a reference that shares no code with either (collections.Counter over a
bisect of the 120 lower bounds), byte for byte."""
import bisect
import collections
import random

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import seeded as S  # noqa: E402

CAP = 8                # bucketCellCapacity: samples in the inline cell, the rest in the spill list
HIST_LANES = 32        # hist.hip: lanes per series in the group pass
HIST_GROUP_MAX = 256   # hist.hip: samples the group pass counts itself; more go to the block pass
NS = [0, 1, 7, 8, 9, 16, 63, 64, 65, 1000, 5000,
      HIST_LANES - 1, HIST_LANES, HIST_LANES + 1, HIST_GROUP_MAX - 1, HIST_GROUP_MAX, HIST_GROUP_MAX + 1]

LOWS = [0, 1, 2, 3] + [2 ** e + j * 2 ** (e - 2) for e in range(2, 31) for j in range(4)]


class HistSeeded(S.Seeded):
    """Seeded with the lh stream on, on both sides."""

    def __init__(self, *a, **kw):
        self.lh = []
        super().__init__(*a, **kw)

    def _seed_oracle(self):
        super()._seed_oracle()
        self.so.emit_hist = self.lh.append

    def _seed_engine(self):
        from apmbackend_amd.models import pipeline
        real = pipeline.APMEngine
        pipeline.APMEngine = lambda C, outputs=(): real(C, outputs=tuple(outputs) + ("lh",))
        try:
            super()._seed_engine()
        finally:
            pipeline.APMEngine = real


def counter_rows(order, buckets, label):
    """The rows of bucket `label` from the case table alone."""
    rows = []
    for key in order:
        vals = buckets.get(key, {}).get(label)
        if not vals:
            continue
        c = collections.Counter(max(0, bisect.bisect_right(LOWS, v) - 1) for v in vals if v != S.ELAPSED_NAN)
        pairs = ",".join(f"{LOWS[b]}:{c[b]}" for b in sorted(c))
        rows.append(f"lh|{label * 10000}|{key[0]}|{key[1]}|{len(vals)}|{vals.count(S.ELAPSED_NAN)}|{pairs}")
    return rows


def check(sd, order, buckets, labels):
    want = [r for b in labels for r in counter_rows(order, buckets, b)]
    got = sd.eng.take("lh")
    assert sd.lh == want, "oracle and Counter reference differ: " + str(
        S.first_difference(sd.lh, want, lambda i: ""))
    diff = S.first_difference(got, want, lambda i: want[i].split("|")[3] if i < len(want) else "")
    assert diff is None, "lh rows: " + diff
    return want


def test_group_max_is_the_kernels():
    from apmbackend_amd import _native
    N = _native.load(build_if_missing=False)
    assert N.hist_group_max() == HIST_GROUP_MAX
    vals = [-5, 0, 1, 3, 4, 7, 8, 10, S.INT32_MAX] + [2 ** k + d for k in range(3, 31) for d in (-1, 0, 1)]
    assert [N.hist_bin(v) for v in vals] == [max(0, bisect.bisect_right(LOWS, v) - 1) for v in vals]
    assert [N.hist_lower(b) for b in range(120)] == LOWS


def test_one_rollover_all_cases():
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    R = S.LATEST + 1 - 6
    rng = random.Random(1515)
    order, buckets = [], {}

    def add(name, vals, decoys=True):
        k = S.key(name)
        b = collections.OrderedDict()
        if decoys:  # neighbours of the reported bucket: must not be counted
            b[R - 1] = [2_000_000_000, 77]
            b[R + 1] = [S.INT32_MAX, 1]
        b[R] = list(vals)
        order.append(k)
        buckets[k] = b
        return k

    # sample counts: inline cell, first spilled sample, group strides, the block pass
    for n in NS:
        if n == 0:
            add("n0", [])  # count 0: active, no row
        else:
            add(f"n{n}", S._values(rng, n, -50, 10 ** 6))
    # values
    add("all_equal", [777] * 1234)                                   # one bin, a 4-digit count
    add("every_bin", rng.sample(LOWS, len(LOWS)))                    # the widest row: 120 pairs
    add("every_bin_upper", [LOWS[b + 1] - 1 for b in range(119)] + [S.INT32_MAX])
    add("zero_negative", [0, -1, -2147483647, 0, -7])
    add("int32_max", [S.INT32_MAX])
    add("one_nan", [5, 6, S.ELAPSED_NAN, 7, 100000])
    add("only_nan", [S.ELAPSED_NAN] * 3)
    add("nan_spilled", S._values(rng, 30) + [S.ELAPSED_NAN] + S._values(rng, 9))
    add("nan_spilled_block", S._values(rng, 600) + [S.ELAPSED_NAN] * 2 + S._values(rng, 50))
    # layout: an inactive id and a count-0 series between two reporting ones
    add("before_gap", [1, 2, 3])
    order.append(S.key("inactive"))                                   # import_series only: inactive
    add("count0", [])
    add("after_gap", [4, 5, 6] * 5)
    # two series sharing a wave, one of them in the block pass (ids 2k, 2k + 1)
    if len(order) % 2:
        add("pad", [9])
    add("wave_block", S._values(rng, 700))
    add("wave_group", S._values(rng, 12))
    add("no_decoys_spill_first", S._values(rng, 40), decoys=False)
    # the trigger gets the next id; then the largest id spills too: first / middle / last of the list
    order.append(S.TRIGGER)
    add("last_id_spills", S._values(rng, 100))
    if len(order) % 2 == 0:
        add("odd_tail", S._values(rng, 20))
    assert len(order) % 2 == 1, "the last wave's upper half must be past n_series"
    assert buckets[order[0]][R] == [] and len(buckets[order[1]][R]) == 1

    sd = HistSeeded(C, order, buckets)
    sd.step()
    want = check(sd, order, buckets, [R])
    assert len(want) == len([k for k in order if buckets.get(k, {}).get(R)])
    widest = [r for r in want if "|S:every_bin|" in r][0]
    assert widest.count(":") == 120 + 1  # (one in the service name)
    assert any(r.endswith("|1234|0|768:1234") for r in want)
    # the st / fs rows are what an engine without the stream prints
    plain = S.Seeded(C, order, buckets, reference=False)
    plain.step()
    assert sd.eng.take("st") == plain.eng.take("st") == sd.st
    assert sd.eng.take("fs") == plain.eng.take("fs")
    assert plain.eng.take("lh") == []


def test_jump_reports_every_bucket_once():
    """Seeded at LATEST, triggered at LATEST + 3: buckets LATEST - 5, - 4, - 3 once each, ascending,
    series in emission order inside each; a second rollover does not repeat them."""
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=CAP)
    rng = random.Random(3)
    order, buckets = [], {}
    first = S.LATEST - 5
    for i in range(7):
        k = S.key(f"j{i}")
        b = collections.OrderedDict()
        b[first - 1] = [123456]                       # reported before the seed: never again
        for d in range(3):
            if (i + d) % 3 != 2:                      # not every series is in every bucket
                b[first + d] = S._values(rng, (300, 9)[(i + d) % 3], -5, 10 ** 5)
        b[first + 3] = [42]                           # enters the window at the next rollover
        order.append(k)
        buckets[k] = b
    sd = HistSeeded(C, order, buckets)
    sd.step_no = 2                                    # the next step's tx lies in bucket LATEST + 3
    sd.step()
    want = check(sd, order, buckets, [first, first + 1, first + 2])
    assert [r.split("|")[1] for r in want] == sorted(r.split("|")[1] for r in want)
    assert len({r.split("|")[1] for r in want}) == 3
    sd.lh.clear()
    sd.step()                                         # LATEST + 4: exactly bucket first + 3
    check(sd, order, buckets, [first + 3])

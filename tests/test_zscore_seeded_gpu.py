"""K10 z-score on seeded histories, compared exactly.

Every value that can enter a ring in these runs is a multiple of 0.5 in [0, 127.5] (asserted on
the reference side by seeded.zscore_reference): exact in fp64, fp32 and bf16, so every window sum
and count is exact in any summation order and the sequential mean, the Neumaier rolling sum, the
VALU resync and the matrix-core resync must all produce the doubles of the exact-mode oracle.  The
fs rows are compared byte for byte and the rings element for element: no tolerance, no tie
allowance.  LAG 3 / 6 / 64 / 65 / 130 give resync partitions of 1 (with empty partitions), 1, 1
exactly, 2 (last partition past LAG) and 3 entries; 37 series in a 64-series engine with resync
period 2 put a range boundary inside a 64-series block, at a 16-series tile edge, and leave 5
series in the last range; max LAG + 5 rollovers visit every head position, the wrap and every
resync phase."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import seeded as S  # noqa: E402

MODES = {"exact": ("exact", 360, False), "rolling_valu_2": ("rolling", 2, False),
         "rolling_mfma_2": ("rolling", 2, True), "rolling_360": ("rolling", 360, False)}


def _series_of(line):
    return line.split("|")[3]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("ring", ["float64", "float32", "bfloat16"])
def test_seeded_histories_match_exact_oracle(ring, mode):
    want_st, want_fs, want_hist = S.zscore_reference()
    overrides, order, buckets, histories, fed = S.zscore_case()
    mean_mode, every, mfma = MODES[mode]
    C = S.seeded_cfg(lags=S.Z_DEFAULTS, ring=ring, mode=mean_mode, resync_every=every, mfma=mfma,
                     max_series=S.Z_MAX_SERIES, overrides=overrides)
    sd = S.Seeded(C, order, buckets, histories, reference=False)  # (the reference run is shared)
    assert len(order) + 1 == S.Z_SERIES
    for _ in range(S.Z_STEPS):
        sd.step(fed)
    got_st, got_fs = sd.eng.take("st"), sd.eng.take("fs")
    diff = S.first_difference(got_st, want_st, lambda i: _series_of(want_st[i]))
    assert diff is None, "st rows: " + diff
    diff = S.first_difference(got_fs, want_fs, lambda i: f"{_series_of(want_fs[i])} LAG {want_fs[i].split('|')[4]}")
    assert diff is None, "fs rows: " + diff
    assert len(got_fs) == len(S.Z_LAGS) * len(got_st) > 0
    # ring content: every series and LAG, element for element, NaN = NaN
    keys = order + [S.TRIGGER]
    nat = sd.eng.eng
    assert [tuple(k) for k in nat.export_series()] == keys
    for li, lag in enumerate(S.Z_LAGS):
        lens, raw = nat.export_history(li, 0, len(keys))
        vals = np.frombuffer(raw, dtype=np.float64).reshape(len(keys), 3, lag)
        for i, k in enumerate(keys):
            for j, want in enumerate(want_hist[k][lag]):
                w = np.array([np.nan if v is None else v for v in want], dtype=np.float64)
                assert lens[i] == len(w), (k, lag, lens[i], len(w))
                assert np.array_equal(vals[i, j, :len(w)], w, equal_nan=True), (k, lag, j, vals[i, j, :len(w)], w)


# values that do round in a reduced ring: 255.5 is a bf16 tie (-> 256, even), 255.9 and
# 1.99999999 round up across a power of two (bf16 / fp32), 3.0e38 is near the top of the range
ROUNDING = [100.3, 0.1, 255.5, 256.5, 1e-3, 3.0e38, 255.9, 1.99999999, float("nan"), 0.0]
# the same kind of value as a window average (pushed by the kernel): (samples, average)
PUSHED = {"avg100_3": [100] * 7 + [101] * 3, "avg0_1": [0] * 9 + [1], "avg255_5": [255, 256],
          "avg256_5": [256, 257], "avg255_9": [256] * 9 + [255]}


@pytest.mark.parametrize("ring", ["float32", "bfloat16"])
def test_ring_store_rounding(ring):
    """What a reduced ring returns is float32(v), or the round-to-nearest-even bfloat16 of
    float32(v) (numpy bit operations in seeded.ring_rounded): the host's ring_store / ring_load
    (import_history / export_history) and the kernel's st / ld (values pushed as window averages
    for a few rollovers; the histories stay shorter than LAG, so what is stored is x itself)."""
    lag, pushes = 16, 4
    C = S.seeded_cfg(lags=((lag, 3.0, 0.5),), ring=ring, mode="rolling", max_series=64)
    labels = S.window_labels(C)
    order, buckets, histories = [], {}, {}
    for name, samples in PUSHED.items():
        k = S.key(name)
        order.append(k)
        # all samples in the newest bucket every window of the run still reads
        buckets[k] = {labels[0] + pushes - 1: list(samples)}
        histories[k] = {lag: (list(ROUNDING), list(ROUNDING[::-1]), list(ROUNDING))}
    sd = S.Seeded(C, order, buckets, histories)
    nat = sd.eng.eng

    def rings():
        lens, raw = nat.export_history(0, 0, len(order))
        return lens, np.frombuffer(raw, dtype=np.float64).reshape(len(order), 3, lag)

    lens, vals = rings()  # host ring_store -> ring_load
    for i in range(len(order)):
        assert lens[i] == len(ROUNDING)
        for j, src in enumerate((ROUNDING, ROUNDING[::-1], ROUNDING)):
            assert np.array_equal(vals[i, j, :len(src)], S.ring_rounded(src, ring), equal_nan=True), (i, j)
    for _ in range(pushes):
        sd.step()
    sd.eng.take("fs")
    lens, vals = rings()  # the kernel's st, read back by the host's ring_load
    x = {}
    for line in sd.st:  # the oracle's st rows: the x of every rollover
        f = line.split("|")
        if f[2] == S.SERVER:
            x.setdefault(f[3], []).append([float(v) for v in f[5:8]])
    for i, k in enumerate(order):
        assert lens[i] == len(ROUNDING) + pushes
        xs = np.array(x[k[1]])
        assert xs.shape == (pushes, 3) and not np.isnan(xs).any()
        assert xs[0, 0] == sum(PUSHED[k[1][2:]]) / len(PUSHED[k[1][2:]])
        for j, src in enumerate((ROUNDING, ROUNDING[::-1], ROUNDING)):
            want = S.ring_rounded(list(src) + list(xs[:, j]), ring)
            assert np.array_equal(vals[i, j, :len(want)], want, equal_nan=True), (k, j, vals[i, j, :len(want)], want)

"""Seeded-engine harness for the window-statistics (K8) and z-score (K10) kernels.

A fresh engine is seeded through the resume importers (import_series / import_buckets /
import_history) from plain Python data, one `tx` wire line of a dedicated trigger series in the
next bucket fires exactly one rollover (K8, K10, K11, K12 over the seeded state), and the result
is read back (winstats / st / fs / export_history).  The CPU oracle (StatsOracle, ZScoreOracle) is
seeded with the same data and fed the same lines; for K8 there is also a reference that shares no
code with the oracle (sorted() + Fraction ranks + exact integer mean).

Nothing here needs a GPU at import time: the case tables and the references are checked by
tests/test_seeded_cases.py on any machine.
"""
import collections
import math
import random
from fractions import Fraction

import numpy as np

from apmbackend_amd.models import oracle
from apmbackend_amd.utils import jsfmt
from apmbackend_amd.utils.config import default_config, zscore_lag_settings

INT32_MAX = 2 ** 31 - 1
ELAPSED_NAN = -2 ** 31          # apm_types.h ELAPSED_NAN: the stored form of a NaN elapsed
LATEST = 157839200              # bucket label (endTs without its last 4 digits) of the seeded state
SERVER = "jvm00"
TRIGGER = ("jvmTR", "S:trigger")  # the series whose tx fire the rollovers, on a server of its own

# stats.hip constants the case tables bracket
HW = 32            # k_window_stats_h2: lanes per series, register network up to HW samples
H2_TILE = 512      # k_window_stats_h2: half_sort_regs up to H2_TILE, then the block pass
WS_TILE = 1024     # k_window_stats: LDS bitonic up to WS_TILE, then the block pass
BIG_TILE = 16384   # k_window_stats_big: block bitonic up to BIG_TILE, then the radix select
APM_WAVE = 64      # k_window_stats: registers up to one wave
K8_INLINE_SLOTS = 64

H2_NS = [0, 1, 2, 3, 4, 5, 19, 20, 21, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513,
         1023, 1024, 1025]
BIG_NS = [16383, 16384, 16385, 20000]
WAVE_NS = [0, 1, 63, 64, 65, 1023, 1024, 1025]
LONG_NS = [0, 1, 33, 513, 16385]


# ------------------------------------------------------------------------------- config

def seeded_cfg(window=31, buffer=6, cell_cap=8, lags=((6, 3.0, 0.5), (30, 2.0, 0.0)), ring="float64",
               mode="exact", resync_every=360, mfma=False, max_series=4096, overrides=None):
    """The small test config (tests/test_engine_gpu.py small_cfg) with the host join, so
    process_tx_lines feeds the stats stage directly, and the spill area the seeded cases need."""
    assert max_series <= 4096
    C = default_config(replay=True)
    C["streamCalcZScore"]["defaults"] = [{"LAG": l, "THRESHOLD": t, "INFLUENCE": i} for l, t, i in lags]
    C["streamCalcZScore"]["overrides"]["services"] = dict(overrides or {})
    C["streamCalcStats"]["windowSizeInIntervals"] = window
    C["streamCalcStats"]["bufferSizeInIntervals"] = buffer
    C["streamProcessAlerts"]["rollingAlertWindowSizeInIntervals"] = 10
    C["streamProcessAlerts"]["requiredNumberBadIntervalsInAlertWindowToTrigger"] = 3
    C["streamProcessAlerts"]["perServiceAlertCooldownInMinutes"] = 2
    C["gpu"].update({"emulateOverrideAliasing": False, "zscoreMeanMode": mode, "timezone": "UTC",
                     "maxSeries": max_series, "batchBytes": 4 << 20, "maxLinesPerBatch": 1 << 16,
                     "bucketCellCapacity": cell_cap, "bucketOverflowCapacity": 1 << 21, "joinOnDevice": False,
                     "ringDtype": ring, "exactRecomputeEveryIntervals": resync_every,
                     "resyncOnMatrixCores": mfma})
    return C


def stats_settings(C):
    sc = C["streamCalcStats"]
    return int(sc["intervalLengthInSeconds"]), int(sc["windowSizeInIntervals"]), int(sc["bufferSizeInIntervals"])


def window_labels(C, latest=LATEST + 1):
    """Bucket labels the rollover at `latest` reads: latest - keep <= b <= latest - buffer."""
    _iv, window, buffer = stats_settings(C)
    return list(range(latest - window - buffer, latest - buffer + 1))


# ------------------------------------------------------------------------------- K8 reference

def frac_ranks(n, pct):
    """calcPercentile's (lo, hi) ranks in exact rational arithmetic on p*n/100 - 1."""
    if n <= 0:
        return (-1, -1)
    idx = Fraction(pct * n, 100) - 1
    if n == 1 or idx.denominator == 1:
        i = int(idx)  # (n == 1: -0.25 / -0.05 truncate to 0, as `arr[parseInt(index)]` does)
        return (i, i)
    i = math.ceil(idx)
    return (i, i) if i == n - 1 else (i, i + 1)


def _js(v):
    return float("nan") if v == ELAPSED_NAN else v


def frac_window_stats(bucket_lists, tpm_div):
    """Raw (unrounded) n, tpm, avg, p75, p95 of a window given its buckets in key order, each in
    arrival order: exact integer mean, sorted() and Fraction ranks.  A NaN sample (ELAPSED_NAN)
    poisons the mean and leaves the JS insertion order (oracle.js_window_array) to the ranks."""
    flat = [v for b in bucket_lists for v in b]
    n = len(flat)
    nan = float("nan")
    if n == 0:
        return 0, 0.0, nan, nan, nan
    if ELAPSED_NAN in flat:
        arr = oracle.js_window_array([[_js(v) for v in b] for b in bucket_lists])
        avg = nan
    else:
        arr = sorted(flat)
        avg = float(Fraction(sum(flat), n))  # correctly rounded, as the double division of exact ints
    out = []
    for pct in (75, 95):
        lo, hi = frac_ranks(n, pct)
        out.append(float(arr[lo]) if lo == hi else (arr[lo] + arr[hi]) / 2)  # ints: exact halves
    # tpm is the JS double formula itself (count / (window * interval / 60)): nothing to rank
    return n, n / tpm_div, avg, out[0], out[1]


_native_mod = [None, False]


def _native():
    if not _native_mod[1]:
        _native_mod[1] = True
        try:
            from apmbackend_amd import _native as nat
            _native_mod[0] = nat.load(build_if_missing=False)
        except Exception:  # no extension here: the oracle's formatting rounds instead
            _native_mod[0] = None
    return _native_mod[0]


def round_fixed(x, f):
    """parseFloat(x.toFixed(f)): the project's JS-exact js_round_fixed where the extension is
    loaded (checked against the oracle's formatting), else the oracle's formatting."""
    if x != x:
        return x
    via_text = float(jsfmt.to_fixed(x, f))
    N = _native()
    if N is not None:
        r = N.js_round_fixed(float(x), f)
        assert r == via_text, (x, f, r, via_text)
        return r
    return via_text


def tier_name(kernel, n, nan=False):
    if nan:
        return "js (NaN window)"
    if kernel == "h2":
        if n <= HW:
            return "h2 register network"
        if n <= H2_TILE:
            e = 2
            while HW * e < n:
                e *= 2
            return f"h2 half_sort_regs<{e}>"
    elif kernel == "wave":
        if n <= APM_WAVE:
            return "wave registers"
        if n <= WS_TILE:
            return "wave LDS bitonic"
    return "block bitonic" if n <= BIG_TILE else "block radix select"


# ------------------------------------------------------------------------------- the harness

Want = collections.namedtuple("Want", "active n tpm avg p75 p95")


def same_double(a, b):
    return a == b or (a != a and b != b)


class Seeded:
    """One seeded engine + the identically seeded oracles.

    order:     series keys (server, service) in creation order; TRIGGER may be listed to give it a
               chosen id (it stays inactive until its first tx), else its first tx creates it last.
               A key without buckets is created and left inactive (no bucket row).
    buckets:   {key: {label: [samples in arrival order]}} -- every (label, list) pair is one
               import_buckets row, an empty list included (count 0: active, nothing to count).
    histories: {key: {lag: (avgList, per75List, per95List)}}, None / NaN = undefined.
    """

    def __init__(self, C, order, buckets, histories=None, latest=LATEST, device=True, reference=True):
        self.reference = reference  # False: the caller holds the reference already (a shared, cached run)
        self.C, self.order, self.buckets, self.latest = C, list(order), buckets, latest
        self.histories = histories or {}
        self.iv, self.window, self.buffer = stats_settings(C)
        self.lags = sorted(int(d["LAG"]) for d in C["streamCalcZScore"]["defaults"])
        self.st, self.fs = [], []
        self.step_no = 0
        self._seed_oracle()
        self.eng = None
        if device:
            self._seed_engine()

    # -- reference side
    def _seed_oracle(self):
        self.so = oracle.StatsOracle(self._on_st, lambda _l: None, self.iv, self.window, self.buffer)
        self.zo = oracle.ZScoreOracle(self.C, self.fs.append)
        self.so.latest = self.latest
        for key in self.order:
            srv, svc = key
            node = self.so.servers.setdefault(srv, collections.OrderedDict())
            if key in self.buckets:
                node[svc] = {int(b): [_js(v) for v in vals] for b, vals in self.buckets[key].items()}
        for key in self.order:
            if key not in self.histories:
                continue
            srv, svc = key
            settings = {int(el["LAG"]): el for el in zscore_lag_settings(self.C, svc, False)}
            node = {}
            for lag in self.lags:
                d = {"THRESHOLD": settings[lag]["THRESHOLD"], "INFLUENCE": settings[lag]["INFLUENCE"]}
                lists = self.histories[key].get(lag, ([], [], []))
                for name, vals in zip(("avgList", "per75List", "per95List"), lists):
                    assert len(vals) <= lag
                    d[name] = [None if v is None or v != v else float(v) for v in vals]
                node[lag] = d
            self.zo.servers.setdefault(srv, collections.OrderedDict())[svc] = node

    def _on_st(self, line):
        self.st.append(line)
        self.zo.consume(line)

    def history_values(self):
        """Every value currently in an oracle history list."""
        for srv in self.zo.servers.values():
            for lags in srv.values():
                for o in lags.values():
                    for name in ("avgList", "per75List", "per95List"):
                        yield from o[name]

    def newest_history_values(self):
        for srv in self.zo.servers.values():
            for lags in srv.values():
                for o in lags.values():
                    for name in ("avgList", "per75List", "per95List"):
                        if o[name]:
                            yield o[name][-1]

    # -- engine side
    def _seed_engine(self):
        from apmbackend_amd.models.pipeline import APMEngine
        self.eng = APMEngine(self.C, outputs=("st", "fs", "al"))
        nat = self.eng.eng
        self.ids = {key: nat.import_series(*key) for key in self.order}
        assert list(self.ids.values()) == list(range(len(self.order)))
        s_ids, bks, cnts, vals = [], [], [], []
        for key in self.order:
            for b, v in self.buckets.get(key, {}).items():
                s_ids.append(self.ids[key]); bks.append(int(b)); cnts.append(len(v)); vals += [int(x) for x in v]
        nat.import_buckets(self.latest, s_ids, bks, cnts, vals)
        for li, lag in enumerate(self.lags):
            ss, lens, blocks = [], [], []
            for key in self.order:
                lists = self.histories.get(key, {}).get(lag)
                if lists is None:
                    continue
                block = np.full((3, lag), np.nan)
                for k, a in enumerate(lists):
                    block[k, :len(a)] = [np.nan if v is None else v for v in a]
                ss.append(self.ids[key]); lens.append(max(len(a) for a in lists)); blocks.append(block)
            if ss:
                nat.import_history(li, ss, lens, np.stack(blocks).astype(np.float64).tobytes())

    # -- one rollover
    def step(self, feed=()):
        """The trigger's tx in the next bucket (one rollover), then `feed`: (key, elapsed) tx that
        land in the new bucket, in order.  The oracle consumes the same lines."""
        self.step_no += 1
        end = (self.latest + self.step_no) * 10000 + 1
        lines = [f"tx|{TRIGGER[0]}|{TRIGGER[1]}|t{self.step_no}|1|{end - 5}|{end}|5|Y"]
        for j, (key, elapsed) in enumerate(feed):
            lines.append(f"tx|{key[0]}|{key[1]}|f{self.step_no}_{j}|1|{end - 5}|{end + 1 + j % 9000}|{elapsed}|N")
        if self.reference:
            for ln in lines:
                self.so.consume(ln)
        if self.eng is not None:
            self.eng.eng.process_tx_lines(("\n".join(lines) + "\n").encode(), -1.0)

    # -- K8 expectations for the first rollover, from the Fraction reference
    def want_winstats(self):
        """Per series id (creation order, the trigger last unless listed): the WinStat the first
        rollover must produce, and the st rows it must print, from the independent reference."""
        labels = window_labels(self.C, self.latest + 1)
        tpm_div = self.window * self.iv / 60.0
        edge_ts = (self.latest + 1 - self.buffer - 1) * 10000
        want, rows = [], []
        keys = list(self.order) + ([] if TRIGGER in self.order else [TRIGGER])
        for key in keys:
            if key not in self.buckets:
                want.append(Want(0, 0, 0.0, 0.0, 0.0, 0.0))
                continue
            win = [self.buckets[key][b] for b in labels if b in self.buckets[key]]
            n, tpm, avg, p75, p95 = frac_window_stats(win, tpm_div)
            want.append(Want(1, n, round_fixed(tpm, 2), round_fixed(avg, 1), round_fixed(p75, 1), round_fixed(p95, 1)))
            rows.append(f"st|{edge_ts}|{key[0]}|{key[1]}|{jsfmt.nf(tpm, 2)}|{jsfmt.nf(avg)}|{jsfmt.nf(p75)}|{jsfmt.nf(p95)}")
        return want, rows

    def winstats(self):
        self.eng.eng.flush()
        return [Want(*w) for w in self.eng.eng.winstats()]


def first_difference(got, want, describe):
    """Index and description of the first differing entry of two sequences (None when equal)."""
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"entry {i} {describe(i)}:\n  got  {g}\n  want {w}"
    if len(got) != len(want):
        return f"{len(got)} entries, want {len(want)}"
    return None


def check_k8(sd, kernel, names):
    """One rollover of the seeded engine `sd` against both references.  names[i]: label of series
    i.  The references must agree with each other before the engine is looked at."""
    want, rows = sd.want_winstats()
    sd_cpu_st = run_oracle_only(sd)
    assert sd_cpu_st == rows, "case table: oracle and Fraction reference differ -- " + str(
        first_difference(sd_cpu_st, rows, lambda i: ""))
    sd.step()
    got_st = sd.eng.take("st")
    got = sd.winstats()
    assert len(got) == len(want), (len(got), len(want))

    def describe(i):
        w = want[i]
        nan = w.active and w.n > 0 and w.avg != w.avg
        return f"series {i} ({names[i] if i < len(names) else 'trigger'}, n={w.n}, {tier_name(kernel, w.n, nan)})"

    for i, (g, w) in enumerate(zip(got, want)):
        if not w.active:
            assert (g.active, g.n) == (0, 0), describe(i) + f": got {g}"
            continue
        ok = (g.active, g.n) == (w.active, w.n) and all(same_double(a, b) for a, b in zip(g[2:], w[2:]))
        assert ok, describe(i) + f":\n  got  {g}\n  want {w}"
    active = [i for i, w in enumerate(want) if w.active]
    diff = first_difference(got_st, rows, lambda i: describe(active[i]) if i < len(active) else "")
    assert diff is None, "st rows: " + diff
    return want


def run_oracle_only(sd):
    """The st rows the oracle prints for the first rollover of `sd`'s seed (a CPU twin, so the
    seeded engine's own oracle is still at the seeded state)."""
    twin = Seeded(sd.C, sd.order, sd.buckets, sd.histories, sd.latest, device=False)
    twin.step()
    return twin.st


# ------------------------------------------------------------------------------- K8 case tables

def _values(rng, n, lo=-50, hi=10 ** 6):
    """n seeded int32 samples in [lo, hi] with many duplicates."""
    pool = [rng.randint(lo, hi) for _ in range(n // 3 + 1)]
    return [rng.choice(pool) for _ in range(n)]


def layout(vals, labels, how, where=0):
    """Samples over the window buckets: 'one' (all in labels[where]), 'spread' (evenly over all,
    the first and last included), 'ends' (oldest and newest bucket only)."""
    n, w = len(vals), len(labels)
    out = collections.OrderedDict()
    if how == "one":
        out[labels[where % w]] = list(vals)
    elif how == "ends":
        out[labels[0]] = list(vals[:n // 2])
        out[labels[-1]] = list(vals[n // 2:])
    elif n >= w:
        at = 0
        for j, b in enumerate(labels):
            m = n // w + (1 if j < n % w else 0)
            out[b] = list(vals[at:at + m])
            at += m
    else:  # fewer samples than buckets: evenly spaced, both ends used once n >= 2
        for i, v in enumerate(vals):
            j = w - 1 if n == 1 else round(i * (w - 1) / (n - 1))
            out.setdefault(labels[j], []).append(v)
    return out


class Buckets(collections.OrderedDict):
    decoys = frozenset()  # labels of the buckets outside the window


def with_decoys(b, labels, k=0):
    """Two buckets just outside the window (2e9-scale values that must not be counted): the older
    one is dropped by the rollover's removeOldBuckets, the newer one is inside `keep` only."""
    b = Buckets(b)
    b[labels[0] - 1] = [2_000_000_000 + k, 1_999_999_999]
    b[labels[-1] + 1] = [2_000_000_007, 2_000_000_000 + k, INT32_MAX]
    b.decoys = {labels[0] - 1, labels[-1] + 1}
    return b


def key(name):
    return (SERVER, "S:" + name)


def sized_cases(C, ns, layouts, seed, decoys=True):
    """One series per (n, layout): (order, buckets, names, ns_by_series)."""
    rng = random.Random(seed)
    labels = window_labels(C)
    order, buckets, names, sizes = [], {}, [], []
    for n in ns:
        for how in layouts:
            k = key(f"n{n}_{how}")
            b = layout(_values(rng, n), labels, how, where=len(order))
            if n == 0:
                b[labels[len(order) % len(labels)]] = []  # count 0: active, empty window
            buckets[k] = with_decoys(b, labels, len(order)) if decoys else b
            order.append(k); names.append(f"n={n} {how}"); sizes.append(n)
    return order, buckets, names, sizes


def add_series(order, buckets, names, sizes, name, b):
    """Appends series `name` with buckets b (decoys included); its size is what lies between them."""
    k = key(name)
    order.append(k); buckets[k] = b; names.append(name)
    sizes.append(sum(len(v) for lab, v in b.items() if lab not in getattr(b, "decoys", ())))
    return k


# ------------------------------------------------------------------------------- K10 helpers

def assert_half_multiples(values):
    """The precondition of the exact K10 comparison: every defined value that can enter a ring is
    a multiple of 0.5 in [0, 127.5] -- exact in fp64, fp32 and bf16, so every window sum is exact
    in any summation order."""
    for v in values:
        if v is None or v != v:
            continue
        assert 0.0 <= v <= 127.5 and float(v * 2).is_integer(), f"{v!r} is not a multiple of 0.5 in [0, 127.5]"


def bf16_bits_rne(u32):
    """float32 bit patterns -> bfloat16 bit patterns, round to nearest even, NaN -> 0x7FC0."""
    u = np.asarray(u32, dtype=np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, 0x7FC0, r).astype(np.uint16)


def ring_rounded(values, ring):
    """float64 values as a ring of dtype `ring` returns them."""
    v = np.asarray(values, dtype=np.float64)
    if ring == "float64":
        return v
    with np.errstate(over="ignore"):
        f = v.astype(np.float32)
    if ring == "float32":
        return f.astype(np.float64)
    bits = bf16_bits_rne(f.view(np.uint32)).astype(np.uint32) << 16
    return bits.view(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------- K10 case table

Z_LAGS = (3, 6, 64, 65, 130)   # per = ceil(LAG / 64): 1 (empty partitions), 1, 1 exactly, 2, 3
Z_DEFAULTS = tuple(zip(Z_LAGS, (1.5, 2.0, 2.5, 3.0, 1.75), (0.5,) * 5))
Z_STEPS = max(Z_LAGS) + 5
Z_MAX_SERIES = 64              # resync period 2 -> ranges of 32 series
Z_SERIES = 37                  # the trigger included: the last range holds 5 series


def _ramp(L, mul, add):
    """A history of distinct-looking multiples of 0.5 in [10, 109.5]: dropping or double counting
    any entry changes the window sum (a constant history would hide a double count: the count
    moves with the sum)."""
    return [10.0 + ((i * mul + add) % 200) * 0.5 for i in range(L)]


def zscore_case():
    """The K10 case table: (overrides, order, buckets, histories, feed).

    Per series: a history per LAG (the same list for avg / p75 / p95), a window kind and an
    INFLUENCE.  Windows are constant (`const c`: one sample c per bucket) or two-valued (`two a b`:
    a and b once per bucket, avg (a+b)/2, p75 = p95 = b) and are kept alive by one or two tx per
    rollover, so avg / p75 / p95 never change while the window slides; `short c k` is a constant
    window seeded only in the k oldest window buckets (defined for k rollovers, then empty: the
    influence chain I*x + (1-I)*last stays on multiples of 0.5 for that many signals); `empty` is
    an active series without samples."""
    nan = float("nan")
    full = lambda v: (lambda L: [v] * L)
    def with_nan(v, where):
        def h(L):
            a = [v] * L
            a[where(L)] = nan
            return a
        return h
    S = []  # (name, history(L) -> list, window, INFLUENCE or None, THRESHOLD or None)
    S.append(("len0", lambda L: [], ("const", 20), None, None))
    S.append(("lenLm1", lambda L: [25.0] * (L - 1), ("const", 25), None, None))
    S.append(("lenL", full(25.0), ("const", 25), None, None))
    S.append(("nan_oldest", with_nan(16.0, lambda L: 0), ("const", 16), None, None))
    S.append(("nan_newest", with_nan(16.0, lambda L: L - 1), ("const", 16), None, None))
    S.append(("nan_interior", with_nan(16.0, lambda L: L // 2), ("const", 16), None, None))
    S.append(("all_nan", full(nan), ("const", 16), None, None))
    S.append(("all_zero", full(0.0), ("const", 9), None, None))
    S.append(("newest_nan_signal", with_nan(16.0, lambda L: L - 1), ("const", 80), 0.25, None))
    S.append(("empty_window", full(16.0), ("empty",), None, None))
    # |x - mean| == T * sd exactly: mean 16, sd 4, T 2, x 24 (no signal); x 24.5 / 25 (signal)
    S.append(("on_bound", full(16.0), ("const", 24), 0.5, 2.0))
    S.append(("over_bound_i0", full(16.0), ("two", 24, 25), 0.0, 2.0))
    S.append(("over_bound_i1", full(16.0), ("two", 24, 25), 1.0, 2.0))
    for infl, win_up, win_dn in ((0.0, ("const", 80), ("const", 36)), (0.25, ("short", 80, 2), ("short", 36, 2)),
                                 (0.5, ("short", 80, 3), ("short", 36, 3)), (1.0, ("const", 80), ("const", 36))):
        S.append((f"up_i{infl}", full(16.0), win_up, infl, None))
        S.append((f"down_i{infl}", full(100.0), win_dn, infl, None))
    # ramps (distinct entries) around the resync range boundary (id 32) and the 16-series tiles
    wins = [("const", 60), ("two", 15, 17), ("const", 10), ("const", 100), ("two", 59, 60), ("const", 35)]
    k = 0
    while len(S) < Z_SERIES - 1:
        mul, add = (7, 13, 37, 51, 73, 91)[k % 6], 11 * k
        cut = (lambda L: L, lambda L: L, lambda L: max(L - 2, 0), lambda L: L // 2, lambda L: L, lambda L: 1)[k % 6]
        def hist(L, mul=mul, add=add, cut=cut, k=k):
            a = _ramp(L, mul, add)[:cut(L)]
            if k % 4 == 1 and len(a) > 4:  # two adjacent NaN over a partition boundary (per = 3: 2 | 3)
                a[2] = a[3] = nan
            return a
        S.append((f"ramp{k}", hist, wins[k % len(wins)], float(k % 2), None))
        k += 1
    assert len(S) == Z_SERIES - 1
    C0 = seeded_cfg(lags=Z_DEFAULTS)
    labels = window_labels(C0)
    _iv, window, buffer = stats_settings(C0)
    overrides, order, buckets, histories, fed = {}, [], {}, {}, []
    for name, hist, win, infl, thr in S:
        kk = key(name)
        order.append(kk)
        if infl is not None or thr is not None:
            o = {}
            if infl is not None:
                o["INFLUENCE"] = infl
            if thr is not None:
                o["THRESHOLD"] = thr
            overrides[kk[1]] = {str(L): dict(o) for L in Z_LAGS}
        histories[kk] = {L: (hist(L), hist(L), hist(L)) for L in Z_LAGS}
        per_bucket = {"const": lambda w: [w[1]], "two": lambda w: [w[1], w[2]], "short": lambda w: [w[1]],
                      "empty": lambda w: []}[win[0]](win)
        if win[0] == "empty":
            buckets[kk] = {LATEST: []}
        elif win[0] == "short":
            buckets[kk] = {b: list(per_bucket) for b in labels[:win[2]]}
        else:  # every bucket any later window can still read
            buckets[kk] = {b: list(per_bucket) for b in range(LATEST - window - buffer, LATEST + 1)}
            fed += [(kk, v) for v in per_bucket]
    return overrides, order, buckets, histories, fed


_Z_REF = {}


def zscore_reference():
    """The exact-mode oracle over the whole K10 run (computed once; the same for every ring dtype
    and mean mode, which is the point of the precondition), with the precondition checked on every
    value that enters a history list.  Returns (st rows, fs rows, final history lists by key/lag)."""
    if "ref" not in _Z_REF:
        overrides, order, buckets, histories, fed = zscore_case()
        sd = Seeded(seeded_cfg(lags=Z_DEFAULTS, max_series=Z_MAX_SERIES, overrides=overrides), order, buckets,
                    histories, device=False)
        assert_half_multiples(sd.history_values())
        for _ in range(Z_STEPS):
            sd.step(fed)
            assert_half_multiples(sd.newest_history_values())
        final = {k: {L: tuple(list(sd.zo.servers[k[0]][k[1]][L][n]) for n in ("avgList", "per75List", "per95List"))
                     for L in Z_LAGS} for k in order + [TRIGGER]}
        _Z_REF["ref"] = (list(sd.st), list(sd.fs), final)
    return _Z_REF["ref"]


# ------------------------------------------------------------------------------- K12 case table
# Whole st / fs lines from a seeded engine (tests/test_format_seeded_gpu.py).  The point is line
# layout, so no printed value depends on how an expression is evaluated: window samples are
# int32 (exact sums, exact halves), every LAG 2 history is [v, v] (0 + v + v and / 2 are exact),
# THRESHOLD is 0 (lb = ub = mean - 0 * sd = mean) and INFLUENCE is 0 or 1 (the stored value is x
# or the last entry, exactly).  The other LAGs hold constant half-multiples or stay short.

FMT_WAVE_LINES = 64                              # format.hip: lines per block of the write pass
FMT_STAGES = (8192, 12288, 16384, 24576)         # format.hip: k_format_write's LDS stages
FMT_LAGS = {1: (2,), 2: (2, 5), 3: (2, 5, 9)}
FMT_WIDE = -math.nextafter(1e21, 0.0)            # toFixed(1) prints '-', 21 digits, '.0': 24 characters
FMT_WIDE_JSON = -math.nextafter(2.0 ** 127, 0.0)  # String(x) prints 23 characters, the widest exact one


def fmt_stage(hint):
    """apm_format_write: the stage for the hint note_fmt_block left (0: none yet)."""
    want = hint or 12288
    return 8192 if want <= 7168 else 12288 if want <= 12800 else 16384 if want <= 16896 else 24576


def fmt_hint(st_bytes, st_lines, fs_bytes, fs_lines):
    """Engine::note_fmt_block: 64 average lines of the longer stream (None: the hint stays)."""
    a = max(st_bytes // st_lines if st_lines else 0, fs_bytes // fs_lines if fs_lines else 0)
    return min(a * 64, 1 << 20) if a else None


def fmt_history_pool():
    """The boundary values of the number-printer table a history can hold: finite, outside every
    flag domain, v + v finite; -0.0 left out (0 + -0 + -0 is +0: the mean would not be v)."""
    import format_cases as F
    out = []
    for x in F.number_table()[:4000]:
        if x != x or abs(x) >= 2.0 ** 126 or (x == 0 and math.copysign(1, x) < 0):
            continue
        if any(F.may_flag(x, 1, m) for m in F.MODES):
            continue
        out.append(x)
    return out


WINDOWS = [
    [INT32_MAX, INT32_MAX, INT32_MAX],            # avg 2147483647.0: nn = 21474836470 (64-bit split_fixed)
    [-INT32_MAX, -INT32_MAX],                     # the most negative sample a window holds
    [INT32_MAX, INT32_MAX - 1],                   # 2147483646.5
    [ELAPSED_NAN, 7, 3],                          # NaN window: avg undefined
    [],                                           # active, nothing to count: all undefined
    [5], [1, 2, 4], [429496729, 429496730], [-1, 0, 1], [99, 100, 101, 1000000],
    [INT32_MAX, -INT32_MAX, 1], [12, 13],
]


class FormatCase:
    """One engine: n series (the trigger last), n_lags LAGs, two rollovers."""

    def __init__(self, label, n, n_lags, svc_len, inactive=(), copy=False, wide=(), specials=False):
        assert n >= 1
        self.label, self.n, self.n_lags, self.copy = label, n, n_lags, copy
        self.lags = FMT_LAGS[n_lags]
        pool = fmt_history_pool()
        C0 = seeded_cfg(lags=tuple((L, 0.0, 0.0) for L in self.lags))
        labels = window_labels(C0)
        mid = labels[len(labels) // 2]  # inside the window of both rollovers
        self.order, self.buckets, self.histories, self.overrides, self.hist_v = [], {}, {}, {}, {}
        seen = set()
        for i in range(n - 1):
            L = svc_len(i)
            tag = f"{i:03d}"
            svc = (tag + "abcdefghijklmnopqrstuvwxyz" * (L // 26 + 1))[:max(L, 3)]
            if L < 3 and "Q7"[:L] not in seen:  # an empty, a one- and a two-character name, once each
                svc = "Q7"[:L]
            if specials and i % 9 == 4 and L >= 12:  # all four COPY escapes; the st rows hold them raw
                svc = svc[:3] + "\n\\" + svc[5:7] + "\t" + svc[8:10] + "\r" + svc[11:]
            assert svc not in seen
            seen.add(svc)
            k = (SERVER, svc)
            self.order.append(k)
            if i in inactive:
                continue
            self.buckets[k] = {mid: list(WINDOWS[i % len(WINDOWS)])}
            if i in wide:
                # every number as wide as this line can print it: the most negative window, a
                # negative mean (24 characters, lb / ub undefined), positive ones (mean = lb = ub)
                self.buckets[k] = {mid: [-INT32_MAX, -INT32_MAX]}
                w = -(FMT_WIDE_JSON if copy else FMT_WIDE)
                v3 = (-w, w, w)
            else:
                v3 = tuple(pool[(i * 3 + j * 131) * 7 % len(pool)] for j in range(3))
            self.hist_v[k] = v3
            h = {2: tuple([v, v] for v in v3)}
            for L_ in self.lags[1:]:  # constant half-multiples at full length, or one entry short
                c = 0.5 * ((i * 11 + L_) % 255)
                h[L_] = tuple([c] * (L_ if i % 3 else L_ - 2) for _ in range(3))
            self.histories[k] = h
            if i % 2:
                self.overrides[svc] = {str(L_): {"INFLUENCE": 1.0} for L_ in self.lags}
        self.order.append(TRIGGER)

    def cfg(self):
        return seeded_cfg(lags=tuple((L, 0.0, 0.0) for L in self.lags), overrides=self.overrides, max_series=256)

    def reference(self):
        """[(st rows, fs wire rows)] of the two rollovers from the oracle."""
        if not hasattr(self, "_ref"):
            sd = Seeded(self.cfg(), self.order, self.buckets, self.histories, device=False)
            ref = []
            for _ in range(2):
                a, b = len(sd.st), len(sd.fs)
                sd.step()
                ref.append((sd.st[a:], sd.fs[b:]))
            self._ref = ref
        return self._ref

    def expected_rows(self, r):
        """(st rows, fs rows) of rollover r as bytes, each with its line feed: the fs wire rows, or
        what the Python COPY encoder (sinks.copy_encode_lines) makes of them.  (A name may hold a
        line feed itself, so rows are kept as a list and never recovered by splitting.)"""
        from apmbackend_amd.runtime import sinks
        st, fs = self.reference()[r]
        st_rows = [(l + "\n").encode() for l in st]
        if self.copy:
            rows = sinks.copy_encode_lines(fs)["fs"]
            assert len(rows) == len(fs)
            return st_rows, [x.encode() for x in rows]
        return st_rows, [(l + "\n").encode() for l in fs]

    def expected(self, r):
        """(st bytes, fs bytes) of rollover r."""
        st, fs = self.expected_rows(r)
        return b"".join(st), b"".join(fs)

    def active(self, r):
        """Emission positions with lines at rollover r (the trigger from the second one on)."""
        return [i for i, k in enumerate(self.order) if k in self.buckets or (k == TRIGGER and r > 0)]

    def line_lens(self, r):
        """(st, fs) line bytes per emission position / (position, LAG), 0 for an inactive series."""
        st_rows, fs_rows = self.expected_rows(r)
        act = set(self.active(r))
        st_it, fs_it = iter(st_rows), iter(fs_rows)
        st, fs = [], []
        for i in range(self.n):
            st.append(len(next(st_it)) if i in act else 0)
            fs += [len(next(fs_it)) if i in act else 0 for _ in range(self.n_lags)]
        assert next(st_it, None) is None and next(fs_it, None) is None
        return st, fs

    def stage(self, r):
        """The LDS stage rollover r uses: 12 KB without a hint, then from the bytes before it."""
        hint = 0
        for q in range(r):
            st, fs = self.line_lens(q)
            hint = fmt_hint(sum(st), len(st), sum(fs), len(fs)) or hint
        return fmt_stage(hint)

    def flag_count(self):
        """What metrics()["format_fallbacks"] must read after the two rollovers.  k_format_len adds
        one per lane that printed any value inside a flag domain of the number printer
        (format_cases.may_flag), and lane j prints st line j and fs line j: the st lines here
        hold no such value, so that is the number of fs lines holding one.  Read off the wire
        rows: toFixed's digits are its integer n.  COPY rows flag n >= 10^15 below 2^53; nothing
        here reaches 2^127, the only flag of wire rows."""
        k = 0
        for _st, fs in self.reference():
            for line in fs:
                f = line.split("|")
                hit = False
                for tok in [f[5]] + [t for g in f[6:9] for t in g.split(":")[:4]]:
                    if tok == "undefined" or "e" in tok:  # (from 1e21 toFixed prints String(x): exact)
                        continue
                    assert abs(float(tok)) < 2.0 ** 127
                    n = int(tok.replace("-", "").replace(".", ""))
                    hit = hit or (self.copy and abs(float(tok)) < 2.0 ** 53 and n >= 10 ** 15)
                k += hit
        return int(k)

    def max_name_len(self):
        return max(len(a.encode()) + len(b.encode()) for a, b in self.order)

    def name_offsets(self):
        """Engine::intern_name: names appended to one table in first-use order, each once."""
        off, at = {}, 0
        for k in self.order:
            for nm in k:
                if nm not in off:
                    off[nm] = at
                    at += len(nm.encode())
        return off


def block_ranges(lens, base=0):
    """(g0, g1) of every 64-line block of a stream whose line bytes are `lens`."""
    off = [base]
    for x in lens:
        off.append(off[-1] + x)
    return [(off[j], off[min(j + FMT_WAVE_LINES, len(lens))]) for j in range(0, len(lens), FMT_WAVE_LINES)]


def block_is_direct(g0, g1, stage):
    """k_format_write's test, on offsets inside the stream as the kernel takes them.  The stream
    itself need not start on a dword: fs_out lies st_cap bytes into the buffer, so with
    st_cap % 4 != 0 the stage's copy-out stores dwords that are unaligned in memory.  The
    n65_cap0..3 cases exist to show that the bytes come out right for each such start."""
    return g1 - (g0 & ~3) > stage


_FMT_CASES = []


def format_cases():
    if _FMT_CASES:
        return _FMT_CASES
    C = _FMT_CASES
    cyc = lambda *a: (lambda i: a[i % len(a)])
    # series counts around the 64-line block, LAG counts that move the fs blocks' edges
    C.append(FormatCase("n1", 1, 1, cyc(6)))
    C.append(FormatCase("n63", 63, 2, cyc(1, 0, 6, 7, 8, 9, 13, 22), inactive={0, 30}, wide={5}))
    C.append(FormatCase("n64", 64, 3, cyc(5, 6, 7, 8, 11), inactive={62}))
    # st_cap % 4 = (176 + longest name) % 4 with n = 65: the longest service name sets it
    for r in range(4):
        C.append(FormatCase(f"n65_cap{r}", 65, 1 + r % 3, lambda i, r=r: 40 + r if i == 9 else 3 + i % 17,
                            inactive={0} if r == 1 else (), copy=r == 2, specials=r == 2, wide={3}))
    # inactive: the first series, one between active ones, the whole second block (its byte range
    # is empty), and the trigger (the last series, inactive at the first rollover)
    C.append(FormatCase("n129_holes", 129, 1, cyc(4, 9, 14, 3, 21), inactive={0, 17} | set(range(64, 128))))
    # stage sizes by the average block of the first rollover; a block of long names over its stage
    C.append(FormatCase("n129_direct", 129, 2, lambda i: 1000 + i if 70 <= i < 80 else 3 + i % 5))
    C.append(FormatCase("n65_names50", 65, 2, lambda i: 70 + i % 33))
    C.append(FormatCase("n65_names200", 65, 3, lambda i: 200 + i % 29, wide={7}))
    C.append(FormatCase("n129_copy", 129, 2, cyc(12, 13, 15, 18, 30, 44), inactive={64}, copy=True, specials=True,
                        wide={11}))
    return C

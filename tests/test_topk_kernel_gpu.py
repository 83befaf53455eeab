"""K18 (topk.hip) through the topk_select test binding: the two kernels alone on caller-made WinStat
rows and permutations, against tests/topk_ref.py (sorted() by (-value, position)).  Sizes bracket
the tile, two tiles and the point where the final block has to loop; values cover ties across a
tile boundary and around the pivot, NaN, signed zeros, negatives, denormals, infinities and the
tpm floor to the ulp.  Four boards per call, each checked on its own; every comparison is ==."""
import math
import random

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

from apmbackend_amd import _native  # noqa: E402

import topk_ref as R  # noqa: E402

N = _native.load(build_if_missing=False)
T = N.apm_topk_tile()
SPAN = N.apm_topk_final_span()
NAN, INF = float("nan"), float("inf")
DEN = 5e-324
MIN_TPM = 12.25
BELOW, ABOVE = math.nextafter(MIN_TPM, 0.0), math.nextafter(MIN_TPM, INF)
BY = [0, 1, 2, 3]


def loop_n(k):
    """The smallest n at which tiles * k exceeds one sweep of the final block."""
    return (SPAN // k) * T + 1


def sizes(k):
    ns = {0, 1, k - 1, k, k + 1, T - 1, T, T + 1, 2 * T + 1, loop_n(k)}
    return sorted(n for n in ns if n >= 0)


# ---- value patterns: f(rng, n) -> n doubles
def all_equal(rng, n):
    return [7.5] * n


def few_values(rng, n):
    """Three distinct values: the pivot's ties lie in every tile, on both sides of a boundary."""
    return [rng.choice((1.0, 2.0, 3.0)) for _ in range(n)]


def all_nan(rng, n):
    return [NAN] * n


def nan_mixed(rng, n):
    return [NAN if rng.random() < 0.4 else rng.choice((-NAN, float(rng.randint(-5, 5)), rng.random())) for _ in range(n)]


def zeros(rng, n):
    return [rng.choice((-0.0, 0.0, -0.0, 0.0, DEN, -DEN)) for _ in range(n)]


def negatives(rng, n):
    return [-rng.choice((0.5, 1.0, 1e300, 1e-300, rng.random() * 1000)) for _ in range(n)]


def denormals(rng, n):
    return [rng.choice((1, -1)) * DEN * rng.randint(0, 6) for _ in range(n)]


def infinities(rng, n):
    return [rng.choice((INF, INF, -INF, 1.7976931348623157e308, -1.7976931348623157e308, 0.0, 1.0)) for _ in range(n)]


def wide(rng, n):
    return [rng.uniform(-1e6, 1e6) for _ in range(n)]


def tpm_at_floor(rng, n):
    return [rng.choice((MIN_TPM, BELOW, ABOVE, MIN_TPM, 0.0, 100.0)) for _ in range(n)]


def tpm_open(rng, n):
    return [rng.choice((0.0, 0.5, 6.0, 1e9)) for _ in range(n)]


# (tpm, average, per75, per95 patterns, min_tpm)
SCENARIOS = {
    "ties": (all_equal, few_values, all_equal, few_values, 0.0),
    "nan_zero": (tpm_open, all_nan, nan_mixed, zeros, 0.0),
    "range": (wide, negatives, denormals, infinities, 0.0),
    "floor": (tpm_at_floor, few_values, nan_mixed, infinities, MIN_TPM),
}


def make(rng, n, pats, extra=0, inactive=0.2):
    """(win_rows, perm, entries by position): n listed series among n + extra, in a seeded order."""
    S = n + extra
    cols = [p(rng, S) for p in pats]
    active = [0 if rng.random() < inactive else 1 for _ in range(S)]
    win = [(cols[0][s], cols[1][s], cols[2][s], cols[3][s], active[s]) for s in range(S)]
    perm = list(range(S))
    rng.shuffle(perm)
    perm = perm[:n]
    ents = [(bool(win[s][4]), win[s][:4]) for s in perm]
    return win, perm, ents


def check(win, perm, ents, k, min_tpm, by=BY, label=""):
    got = N.topk_select(win, perm, k, by, min_tpm)
    assert len(got) == len(by)
    for b, field in enumerate(by):
        want = [(perm[p], p) for p in R.select(ents, k, min_tpm, field)]
        assert [tuple(x) for x in got[b]] == want, f"{label} board {R.KEYS[field]}"
    return got


@pytest.mark.parametrize("name", list(SCENARIOS))
@pytest.mark.parametrize("k", [1, 20, 128])
def test_sizes_and_values(k, name):
    *pats, min_tpm = SCENARIOS[name]
    rng = random.Random(1000 * k + len(name))
    for n in sizes(k):
        if n == loop_n(k) and k == 1 and name != "ties":
            continue  # (half a million rows: once is enough; k = 20 and 128 loop in every scenario)
        win, perm, ents = make(rng, n, pats, extra=3 if n % 2 else 0)
        check(win, perm, ents, k, min_tpm, label=f"{name} n={n} k={k}")


def test_the_final_block_loops_where_the_sizes_say():
    for k in (1, 20, 128):
        n = loop_n(k)
        tiles = (n + T - 1) // T
        assert tiles * k > SPAN >= (tiles - 1) * k and n == (tiles - 1) * T + 1


def test_all_equal_takes_the_first_positions_across_a_tile_boundary():
    n = 2 * T + 1
    win = [(1.0, 5.0, 5.0, 5.0, 1)] * n
    perm = list(range(n))
    for k in (1, 20, 128):
        got = N.topk_select(win, perm, k, BY, 0.0)
        for b in range(4):
            assert [tuple(x) for x in got[b]] == [(p, p) for p in range(k)]
    # the first T - 3 positions are no candidates: the winners straddle the boundary
    win = [(1.0, 5.0, 5.0, 5.0, 0)] * (T - 3) + [(1.0, 5.0, 5.0, 5.0, 1)] * (n - T + 3)
    got = N.topk_select(win, perm, 20, BY, 0.0)
    for b in range(4):
        assert [tuple(x) for x in got[b]] == [(p, p) for p in range(T - 3, T + 17)]


def test_ties_straddle_the_pivot_in_two_tiles():
    """Five entries above the pivot value, the pivot value itself eight times in each of two tiles:
    k = 10 takes the five and the first five ties, all from the first tile."""
    n = 2 * T
    rows = [(1.0, 0.0, 0.0, 0.0, 1)] * n
    rows = [list(r) for r in rows]
    ties = [3, 100, 101, 700, 1500, 1501, 2000, T - 1] + [T, T + 1, T + 64, T + 65, T + 900, T + 1000, 2 * T - 2, 2 * T - 1]
    top = [5, T + 5, 99, 2 * T - 3, 1000]
    for p in ties:
        rows[p][1] = 50.0
    for j, p in enumerate(top):
        rows[p][1] = 60.0 + j
    win = [tuple(r) for r in rows]
    perm = list(range(n))
    ents = [(True, w[:4]) for w in win]
    got = check(win, perm, ents, 10, 0.0, by=[1])
    want_pos = [1000, 2 * T - 3, 99, T + 5, 5] + ties[:5]
    assert [p for _s, p in got[0]] == want_pos
    got = check(win, perm, ents, 14, 0.0, by=[1])
    assert [p for _s, p in got[0]] == [1000, 2 * T - 3, 99, T + 5, 5] + ties[:9]


def test_signed_zeros_are_one_value_and_order_by_position():
    win = [(1.0, -0.0, 0.0, -0.0, 1), (1.0, 0.0, -0.0, -0.0, 1), (1.0, -0.0, -0.0, 0.0, 1), (1.0, -DEN, DEN, NAN, 1)]
    perm = [2, 0, 3, 1]
    got = N.topk_select(win, perm, 3, [1, 2, 3], 0.0)
    assert [tuple(x) for x in got[0]] == [(2, 0), (0, 1), (1, 3)]     # the negative denormal loses
    assert [tuple(x) for x in got[1]] == [(3, 2), (2, 0), (0, 1)]     # the denormal wins, then position order
    assert [tuple(x) for x in got[2]] == [(2, 0), (0, 1), (1, 3)]     # NaN is no candidate


def test_the_tpm_floor_to_the_ulp_and_infinity():
    win = [(MIN_TPM, 1.0, INF, 1.0, 1), (BELOW, 9.0, 9.0, 9.0, 1), (ABOVE, INF, 3.0, -INF, 1), (NAN, 99.0, 99.0, 99.0, 1),
           (INF, 5.0, 5.0, 5.0, 0)]
    perm = [0, 1, 2, 3, 4]
    got = N.topk_select(win, perm, 5, BY, MIN_TPM)
    assert [tuple(x) for x in got[0]] == [(2, 2), (0, 0)]
    assert [tuple(x) for x in got[1]] == [(2, 2), (0, 0)]
    assert [tuple(x) for x in got[2]] == [(0, 0), (2, 2)]
    assert [tuple(x) for x in got[3]] == [(0, 0), (2, 2)]
    got = N.topk_select(win, perm, 5, [0], 0.0)   # without a floor: a NaN tpm is still no candidate
    assert [tuple(x) for x in got[0]] == [(2, 2), (0, 0), (1, 1)]


def test_the_binding_checks_its_arguments():
    win = [(1.0, 1.0, 1.0, 1.0, 1)]
    for args in ((win, [0], 0, [0]), (win, [0], 129, [0]), (win, [0], 1, []), (win, [0], 1, [0, 1, 2, 3, 0]),
                 (win, [0], 1, [4]), (win, [1], 1, [0]), (win, [-1], 1, [0])):
        with pytest.raises(ValueError):
            N.topk_select(*args, 0.0)
    assert [list(map(tuple, b)) for b in N.topk_select([], [], 5, [0, 3], 0.0)] == [[], []]

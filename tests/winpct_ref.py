"""An independent reference for the wp stream (docs/PERCENTILES.md): sorted() + Fraction ranks +
integer halves.  It shares no code with apmbackend_amd (no pct_ranks, no pct_text, no half_text)."""
import math
from decimal import Decimal
from fractions import Fraction

ELAPSED_NAN = -2 ** 31


def frac_ranks(m, q):
    """calcPercentile on p = q / 1000 in exact rationals: idx = p / 100 * m - 1."""
    if m == 1:
        return (0, 0)
    idx = Fraction(q, 100000) * m - 1
    if idx.denominator == 1:
        return (int(idx), int(idx))
    i = math.ceil(idx)
    assert i >= 0
    return (i, i) if i == m - 1 else (i, i + 1)


def label(q):
    """q / 1000 in plain decimal, shortest form."""
    s = format(Decimal(q) / Decimal(1000), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return s


def half(sum2):
    """sum2 / 2 printed exactly."""
    f = Fraction(sum2, 2)
    if f.denominator == 1:
        return str(f.numerator)
    whole = abs(f.numerator) // 2
    return ("-" if f < 0 else "") + f"{whole}.5"


def window_sums(samples, qs):
    """(m, nan, [sum of the ranks read per q]) of one window's samples (any order)."""
    fin = sorted(v for v in samples if v != ELAPSED_NAN)
    nan = len(samples) - len(fin)
    sums = []
    for q in qs:
        if not fin:
            break
        lo, hi = frac_ranks(len(fin), q)
        sums.append(fin[lo] + fin[hi])
    return len(fin), nan, sums


def row(ts, server, service, samples, qs):
    """The wp row of a window, None when it holds no finite sample."""
    m, nan, sums = window_sums(samples, qs)
    if m == 0:
        return None
    pairs = ",".join(f"{label(q)}:{half(v)}" for q, v in zip(qs, sums))
    return f"wp|{ts}|{server}|{service}|{m}|{nan}|{pairs}"

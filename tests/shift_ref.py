"""An independent reference for the ls rows (docs/SHIFT.md): list slices, sorted and
fractions.Fraction over Python integers, no code shared with the oracle, the record classes or the
engine.

A window is a list of bucket lists, oldest first (entry n_win - 1 is the newest).  A rule
(k, q, r_u, r_d, z) sets the newest min(k, n_win) entries (the recent span) against the other entries
(the baseline); q = percentile * 1000, r = ratio * 1000 (0: that side is not tested), z * 1000."""
from fractions import Fraction

ELAPSED_NAN = -2 ** 31
SCALE = 100000


def twice_percentile(fin, q):
    """x_lo + x_hi of the ascending finite samples, 0 without one: the position is q m / 100000; a
    whole position p reads sample p - 1, any other one the samples around it (the last sample
    twice when there is none above)."""
    if not fin:
        return 0
    pos = Fraction(q * len(fin), SCALE)
    if pos.denominator == 1:
        lo = hi = int(pos) - 1
    else:
        lo = pos.numerator // pos.denominator
        hi = min(lo + 1, len(fin) - 1)
    return fin[lo] + fin[hi]


def side(count, m, pred, ratio, z):
    """The share count / m against ratio times the predicted share and z binomial deviations over it."""
    share = Fraction(count, m)
    if share < Fraction(ratio, 1000) * pred or share < pred:
        return False
    return (share - pred) ** 2 >= Fraction(z, 1000) ** 2 * pred * (1 - pred) / m


def rule_ints(entries, rule, min_delta, min_recent, min_baseline):
    """(mB, nanB, mR, nanR, a, b, T2, X2, verdict) of one rule over one window."""
    k, q, r_u, r_d, z = rule
    cut = len(entries) - min(k, len(entries))
    base = [v for e in entries[:cut] for v in e]
    recent = [v for e in entries[cut:] for v in e]
    fb = sorted(v for v in base if v != ELAPSED_NAN)
    fr = sorted(v for v in recent if v != ELAPSED_NAN)
    T2, X2 = twice_percentile(fb, q), twice_percentile(fr, q)
    a = len([v for v in fr if 2 * v > T2]) if fb else 0
    b = len([v for v in fr if 2 * v < T2]) if fb else 0
    verdict = "N"
    if len(fb) >= min_baseline and len(fr) >= min_recent and fr:
        above = Fraction(SCALE - q, SCALE)  # the share the percentile predicts above itself
        if r_u and X2 - T2 >= 2 * min_delta and side(a, len(fr), above, r_u, z):
            verdict = "U"
        elif r_d and T2 - X2 >= 2 * min_delta and side(b, len(fr), 1 - above, r_d, z):
            verdict = "D"
    return len(fb), len(base) - len(fb), len(fr), len(recent) - len(fr), a, b, T2, X2, verdict


def series_ints(entries, rules, min_delta, min_recent, min_baseline):
    """(n, [rule_ints, ...]) of one window."""
    return (sum(len(e) for e in entries),
            [rule_ints(entries, r, min_delta, min_recent, min_baseline) for r in rules])


def pct_label(q):
    return ("%.3f" % (q / 1000.0)).rstrip("0").rstrip(".")


def row(ts, server, service, entries, rules, min_delta, min_recent, min_baseline):
    """The series' ls row, or None when every rule says N."""
    n, per = series_ints(entries, rules, min_delta, min_recent, min_baseline)
    if all(p[8] == "N" for p in per):
        return None
    groups = ",".join("%d:%s:%d:%d:%d:%d:%d:%d:%s" % (r[0], pct_label(r[1]), p[0], p[6], p[2], p[7], p[4], p[5], p[8])
                      for r, p in zip(rules, per))
    return "ls|%d|%s|%s|%d|%d|%s" % (ts, server, service, n, min_delta, groups)

"""A reference for the tf rows (docs/TRAFFIC.md) that shares no code with the oracle or the engine:
plain lists, sorted() and Python integers.

`counts` lists the per-bucket sample counts of one series' window, oldest first (entry r, the last
one the newest); a rule is (k, r_d, r_s, z) with r_d / r_s = 0 for a test that is not configured."""


def middle_sum(values):
    """b_lo + b_hi of the ascending values: twice their median."""
    b = sorted(values)
    return b[(len(b) - 1) // 2] + b[len(b) // 2]


def rule_ints(counts, k, r_d, r_s, z, min_rate, min_buckets):
    """(B, R, med2, mad4, verdict) of one rule."""
    n_win = len(counts)
    kk = k if k < n_win else n_win
    B = n_win - kk
    recent, base = counts[B:], counts[:B]
    R = 0
    for c in recent:
        R += c
    med2 = mad4 = 0
    if B > 0:
        med2 = middle_sum(base)
        mad4 = middle_sum([2 * c - med2 if 2 * c >= med2 else med2 - 2 * c for c in base])
    verdict = "N"
    if B >= min_buckets and med2 >= 2 * min_rate:
        drop = r_d != 0 and 2000 * R <= r_d * kk * med2 and 4000 * R <= kk * (2000 * med2 - z * mad4)
        surge = r_s != 0 and 2000 * R >= r_s * kk * med2 and 4000 * R >= kk * (2000 * med2 + z * mad4)
        assert not (drop and surge)
        verdict = "D" if drop else "S" if surge else "N"
    return B, R, med2, mad4, verdict


def series_ints(counts, rules, min_rate, min_buckets):
    """What Engine.traffic() reports for a series with a class: (n, [(B, R, med2, mad4, verdict)])."""
    return sum(counts), [rule_ints(counts, k, r_d, r_s, z, min_rate, min_buckets) for k, r_d, r_s, z in rules]


def row(edge_ts, server, service, counts, rules, min_rate, min_buckets):
    """The tf row of the series, or None when every rule says N."""
    n, per = series_ints(counts, rules, min_rate, min_buckets)
    if all(p[4] == "N" for p in per):
        return None
    groups = ",".join("%d:%d:%d:%d:%d:%s" % ((rules[j][0],) + per[j]) for j in range(len(rules)))
    return "tf|%d|%s|%s|%d|%d|%s" % (edge_ts, server, service, n, min_rate, groups)

"""An independent reference for the sb rows (docs/BURN.md): list slices and fractions.Fraction, no
code shared with the oracle, the record classes or the engine.

A window is a list of bucket lists, oldest first (entry n_win - 1 is the newest).  A rule (k, f)
looks at the newest min(k, n_win) entries.  A set of samples burns at f when it holds at least
min_samples finite samples and (bad / m) / (b / 100000) >= f / 1000 with b = 100000 - q."""
from fractions import Fraction

ELAPSED_NAN = -2 ** 31


def counts(samples, T):
    """(m, bad, nan) of a flat sample list."""
    fin = [v for v in samples if v != ELAPSED_NAN]
    return len(fin), len([v for v in fin if v > T]), len(samples) - len(fin)


def burns(m, bad, q, f, min_samples):
    if m < min_samples or m == 0:
        return False
    return Fraction(bad, m) / Fraction(100000 - q, 100000) >= Fraction(f, 1000)


def series_ints(entries, T, q, rules, min_samples):
    """(m, bad, nan, [(m_k, bad_k), ...], fired mask) of one window."""
    flat = [v for e in entries for v in e]
    m, bad, nan = counts(flat, T)
    per, mask = [], 0
    for j, (k, f) in enumerate(rules):
        tail = entries[len(entries) - min(k, len(entries)):]
        mk, badk, _ = counts([v for e in tail for v in e], T)
        per.append((mk, badk))
        if burns(m, bad, q, f, min_samples) and burns(mk, badk, q, f, min_samples):
            mask |= 1 << j
    return m, bad, nan, per, mask


def row(ts, server, service, entries, T, q, rules, min_samples):
    """The series' sb row, or None when no rule fires."""
    m, bad, nan, per, mask = series_ints(entries, T, q, rules, min_samples)
    if not mask:
        return None
    groups = ",".join("%d:%d:%d:%d:%d" % (k, f, mk, badk, (mask >> j) & 1)
                      for j, ((k, f), (mk, badk)) in enumerate(zip(rules, per)))
    return "sb|%d|%s|%s|%d|%d|%d|%d|%d|%s" % (ts, server, service, T, q, m, bad, nan, groups)

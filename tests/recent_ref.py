"""An independent reference for the rw stream (docs/RECENT.md): list slices + sorted() + the
Fraction ranks and integer halves of tests/winpct_ref.py.  It shares no code with apmbackend_amd."""
from winpct_ref import ELAPSED_NAN, frac_ranks, half, label


def span_ints(entries, k, qs):
    """(m, nan, sum, [sum of the ranks read per q]) of the newest min(k, len(entries)) window
    entries; ``entries`` are the window's bucket lists, oldest first (an absent bucket: [])."""
    take = entries[len(entries) - min(k, len(entries)):]
    samples = [v for b in take for v in b]
    fin = sorted(v for v in samples if v != ELAPSED_NAN)
    sums = []
    for q in qs if fin else ():
        lo, hi = frac_ranks(len(fin), q)
        sums.append(fin[lo] + fin[hi])
    return len(fin), len(samples) - len(fin), sum(fin), sums


def series_ints(entries, spans, qs):
    """Per span the integers of a series, or None when its whole window holds no sample."""
    if not any(entries):
        return None
    return [span_ints(entries, k, qs) for k in spans]


def rows(ts, server, service, entries, spans, qs):
    """The rw rows of a series that prints an st row: one per span, ascending, none when the whole
    window is empty."""
    ints = series_ints(entries, spans, qs)
    if ints is None:
        return []
    out = []
    for k, (m, nan, total, sums) in zip(spans, ints):
        pairs = ",".join(f"{label(q)}:{half(v)}" for q, v in zip(qs, sums))
        out.append(f"rw|{ts}|{server}|{service}|{k}|{m}|{nan}|{total}|{pairs}")
    return out

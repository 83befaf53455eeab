"""An independent reference for the sv stream (docs/SERVICEWINDOW.md): concatenate the members'
windows, sorted(), Fraction ranks, integer halves.  It shares no code with apmbackend_amd; the rank
rule and the two printers come from tests/winpct_ref.py, which is as independent."""
import collections

from winpct_ref import ELAPSED_NAN, frac_ranks, half, label


def union_stats(member_windows, qs):
    """(servers, m, nan, sum, [sum of the ranks read per q]) of a service whose contributing
    members hold the given windows (each a flat list of samples, any order)."""
    flat = [v for w in member_windows for v in w]
    fin = sorted(v for v in flat if v != ELAPSED_NAN)
    sums = []
    for q in qs:
        if not fin:
            break
        lo, hi = frac_ranks(len(fin), q)
        sums.append(fin[lo] + fin[hi])
    return len(member_windows), len(fin), len(flat) - len(fin), sum(fin), sums


def row(ts, service, member_windows, qs):
    """The sv row of a service, None when its members hold no finite sample."""
    servers, m, nan, total, sums = union_stats(member_windows, qs)
    if servers == 0 or m == 0:
        return None
    pairs = ",".join(f"{label(q)}:{half(v)}" for q, v in zip(qs, sums))
    return f"sv|{ts}|{service}|{servers}|{m}|{nan}|{total}|{pairs}"


def rows_from_series(ts, series, qs):
    """series: [(service, window samples)] of the series with an st row, in st row order.  The rows
    in the order of each service's first st row, and {service: union_stats}."""
    by = collections.OrderedDict()
    for service, win in series:
        by.setdefault(service, []).append(list(win))
    rows = [r for r in (row(ts, svc, wins, qs) for svc, wins in by.items()) if r is not None]
    return rows, {svc: union_stats(wins, qs) for svc, wins in by.items()}

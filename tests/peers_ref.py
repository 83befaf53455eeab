"""A reference for the po rows (docs/PEERS.md) that shares no code with the oracle or the engine:
plain lists, sorted() and Python integers.

A member is (server, service, samples or None, min_value or None): `samples` lists the series'
window samples (ELAPSED_NAN = -2^31 stands for a NaN one; None: the series has no st row),
`min_value` the gate of its service (None: class 0).  `S` holds the settings: q (percentile * 1000),
r_h, r_l (0: not configured), z (* 1000), min_delta, min_peers, min_samples."""
import collections

NAN = -2 ** 31
Settings = collections.namedtuple("Settings", "q r_h r_l z min_delta min_peers min_samples")


def ranks(m, q):
    """The one or two 0-based ranks calcPercentile reads among m ascending samples for q / 1000 %."""
    if m == 1:
        return 0, 0
    t = q * m
    if t % 100000 == 0:
        return t // 100000 - 1, t // 100000 - 1
    i = -(-t // 100000) - 1
    return (i, i) if i == m - 1 else (i, i + 1)


def member_value(samples, q):
    """(m, x): the finite samples and the sum of the ranks read (twice the percentile)."""
    fin = sorted(v for v in samples if v != NAN)
    if not fin:
        return 0, 0
    lo, hi = ranks(len(fin), q)
    return len(fin), fin[lo] + fin[hi]


def middle_sum(values):
    """v_lo + v_hi of the ascending values: twice their median."""
    b = sorted(values)
    return b[(len(b) - 1) // 2] + b[len(b) // 2]


def verdict(x, X2, D4, E, S, min_value):
    if E < S.min_peers or X2 < 4 * min_value:
        return "N"
    high = S.r_h != 0 and 2000 * x >= S.r_h * X2 and 4000 * x >= 2000 * X2 + S.z * D4 and 2 * x - X2 >= 4 * S.min_delta
    low = S.r_l != 0 and 2000 * x <= S.r_l * X2 and 4000 * x <= 2000 * X2 - S.z * D4 and X2 - 2 * x >= 4 * S.min_delta
    assert not (high and low)
    return "H" if high else "L" if low else "N"


def members_ints(members, S):
    """Per member what Engine.peers() reports: None, or (m, x, E, X2, D4, verdict)."""
    vals = []
    for _server, _service, samples, min_value in members:
        if samples is None or min_value is None:
            vals.append(None)
            continue
        m, x = member_value(samples, S.q)
        vals.append((m, x) if m >= S.min_samples else None)
    by = collections.OrderedDict()
    for (_server, service, _s, _mv), v in zip(members, vals):
        if v is not None:
            by.setdefault(service, []).append(v[1])
    out = []
    for (_server, service, _s, min_value), v in zip(members, vals):
        if v is None:
            out.append(None)
            continue
        xs = by[service]
        X2 = middle_sum(xs)
        D4 = middle_sum([2 * x - X2 if 2 * x >= X2 else X2 - 2 * x for x in xs])
        out.append((v[0], v[1], len(xs), X2, D4, verdict(v[1], X2, D4, len(xs), S, min_value)))
    return out


def label(q):
    """q / 1000 without trailing zeros."""
    whole, frac = divmod(q, 1000)
    if not frac:
        return str(whole)
    return ("%d.%03d" % (whole, frac)).rstrip("0")


def rows(edge_ts, members, S):
    """(po rows, per-member integers); members in st order."""
    ints = members_ints(members, S)
    out = []
    for (server, service, _s, _mv), v in zip(members, ints):
        if v is not None and v[5] != "N":
            out.append("po|%d|%s|%s|%d|%s:%d|%d|%d|%d|%s" % (edge_ts, server, service, v[0], label(S.q), v[1], v[2], v[3],
                                                          v[4], v[5]))
    return out, ints

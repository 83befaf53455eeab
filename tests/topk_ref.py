"""An independent reference for the tk stream (docs/LEADERBOARD.md): sorted() by
(-value, position) over the candidates.  It shares no code with apmbackend_amd."""
import math

KEYS = ("tpm", "average", "per75", "per95")


def select(entries, k, min_tpm=0.0, field=0):
    """entries: per emission position (active, (tpm, average, per75, per95)).  The positions of the
    best k candidates of key `field` (an index into KEYS), best first: candidates are active, have
    a value that is not NaN and tpm >= min_tpm; value descending, ties by position ascending."""
    cands = []
    for pos, (active, vals) in enumerate(entries):
        v = vals[field]
        if not active or math.isnan(v) or not vals[0] >= min_tpm:
            continue
        cands.append((v, pos))
    return [c[1] for c in sorted(cands, key=lambda c: (-c[0], c[1]))[:k]]


def st_number(text):
    """A number field of an st row as a float ('undefined' / 'NaN' -> NaN)."""
    try:
        return float(text)
    except ValueError:
        return float("nan")


def rows_from_st(st_rows, k, by, min_tpm=0.0):
    """The tk rows of one rollover from its st rows (in emission order): per key of `by`, ranks
    1.. of the selection over the st rows' own numbers, each row ending in its st row's fields 3.."""
    ents, tails, ts = [], [], None
    for r in st_rows:
        f = r.split("|")
        assert f[0] == "st" and len(f) == 8
        ts = f[1]
        ents.append((True, tuple(st_number(x) for x in f[4:8])))
        tails.append("|".join(f[2:]))
    out = []
    for name in by:
        for rank, pos in enumerate(select(ents, k, min_tpm, KEYS.index(name)), 1):
            out.append(f"tk|{ts}|{name}|{rank}|{tails[pos]}")
    return out

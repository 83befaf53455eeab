"""An independent reference for local wall time -> UTC milliseconds, and the case table of the
time-zone tests (tests/test_tz_table.py, tests/test_parse_tz_gpu.py).

Two references, neither sharing code with apmbackend_amd (no TzOffset, no make_date_ms, no
tz_table, no days_from_civil):

* ``utc_ms(zone, fields)``: an aware ``datetime(..., tzinfo=ZoneInfo(zone), fold=0)`` minus the
  epoch in integer arithmetic.  A local time that a transition skips gets the offset from before
  the transition (PEP 495), which is also what ECMA-262's LocalTime does.  Needs a zone database.
* ``utc_ms_listed(base, transitions, fields)``: the same answer from a list of transitions
  ``(utc_ms, offset_before, offset_after)`` by a linear scan for the gap or overlap the local
  time falls into.  Needs no zone database: ``LISTED`` holds the transitions of 2020..2040 as
  literals, for machines without one (tests/test_tz_table.py checks them against zoneinfo).

Fields are ``(year, month, day, hour, minute, second, millisecond)`` as written in the log line;
out-of-range values carry over as ``new Date(y, m - 1, d, h, mi, s, ms)`` does (MakeDay, MakeTime).
"""
import datetime as dt
import re

DST_ZONES = ("America/Chicago", "Europe/Berlin", "Australia/Lord_Howe")
ZONES = DST_ZONES + ("America/Sao_Paulo", "Asia/Kolkata")
FIXED = ("-06:00", "+05:30")
TRANSITION_YEARS = (2021, 2025, 2026, 2027, 2037)
LISTED_YEARS = (2020, 2040)

MS = dt.timedelta(milliseconds=1)
DAY_MS = 86400000
EPOCH = dt.datetime(1970, 1, 1)
EPOCH_UTC = dt.datetime(1970, 1, 1, tzinfo=dt.timezone.utc)


def have_zoneinfo():
    """False only where there is no zone database at all; one that is there but broken raises."""
    try:
        from zoneinfo import ZoneInfo, ZoneInfoNotFoundError
    except ImportError:
        return False
    try:
        ZoneInfo("America/Chicago")
    except ZoneInfoNotFoundError:
        return False
    return True


def tzinfo_of(zone):
    """tzinfo for an IANA name or a fixed ``+HH:MM`` spec."""
    if re.fullmatch(r"[+-]\d\d:\d\d", zone):
        m = int(zone[1:3]) * 60 + int(zone[4:6])
        return dt.timezone(dt.timedelta(minutes=-m if zone[0] == "-" else m))
    from zoneinfo import ZoneInfo
    return ZoneInfo(zone)


def fixed_offset_ms(zone):
    return tzinfo_of(zone).utcoffset(None) // MS


# ---------------------------------------------------------------- fields <-> wall time
def wall(fields):
    """The naive datetime the fields name, after carrying every out-of-range field."""
    y, mo, d, h, mi, s, ms = fields
    y, m0 = y + (mo - 1) // 12, (mo - 1) % 12
    total = ((h * 60 + mi) * 60 + s) * 1000 + ms
    return dt.datetime(y, m0 + 1, 1) + dt.timedelta(days=d - 1 + total // DAY_MS) + (total % DAY_MS) * MS


def local_ms(fields):
    return (wall(fields) - EPOCH) // MS


def fields_of_local(ms):
    t = EPOCH + ms * MS
    return (t.year, t.month, t.day, t.hour, t.minute, t.second, t.microsecond // 1000)


# ---------------------------------------------------------------- reference 1: zoneinfo
def utc_ms(zone, fields):
    w = wall(fields).replace(tzinfo=tzinfo_of(zone), fold=0)
    # aware - aware subtracts each side's own utcoffset(); fold=0 in a gap: the offset before it
    return (w - EPOCH_UTC) // MS


def offset_at(zone, utc):
    """The zone's offset at an instant, from the aware instant."""
    return (EPOCH_UTC + utc * MS).astimezone(tzinfo_of(zone)).utcoffset() // MS


def transitions(zone, year_lo, year_hi):
    """[(utc_ms, offset_before, offset_after)] with year_lo <= UTC year <= year_hi: a probe per
    day, then halving down to the millisecond."""
    if re.fullmatch(r"[+-]\d\d:\d\d", zone):
        return []
    lo = (dt.datetime(year_lo, 1, 1) - EPOCH) // MS
    hi = (dt.datetime(year_hi + 1, 1, 1) - EPOCH) // MS
    out = []
    prev = offset_at(zone, lo)
    for t in range(lo + DAY_MS, hi + DAY_MS, DAY_MS):
        cur = offset_at(zone, t)
        if cur != prev:
            a, b = t - DAY_MS, t
            while b - a > 1:
                m = (a + b) // 2
                a, b = (m, b) if offset_at(zone, m) == prev else (a, m)
            if b < hi:
                out.append((b, prev, cur))
            prev = cur
    return out


# ---------------------------------------------------------------- reference 2: listed transitions
def utc_ms_listed(base, trans, fields):
    loc = local_ms(fields)
    off = base
    for t, before, after in trans:
        if loc < t + min(before, after):
            break  # wholly before this transition, in local time
        if loc < t + max(before, after):
            off = before  # skipped or repeated: the offset from before the transition
            break
        off = after
    return loc - off


def offset_at_listed(base, trans, utc):
    off = base
    for t, _, after in trans:
        if utc >= t:
            off = after
    return off


# (offset before the first transition, transitions of LISTED_YEARS); tests/test_tz_table.py
# checks every entry against zoneinfo where a zone database exists
def _listed(first, second, utc_s):
    """Transitions at utc_s (seconds) that alternate first -> second -> first ... (offsets in ms)."""
    offs = (first, second)
    return first, [(s * 1000, offs[i % 2], offs[(i + 1) % 2]) for i, s in enumerate(utc_s)]


LISTED = {
    "America/Chicago": _listed(-21600000, -18000000, [
        1583654400, 1604214000, 1615708800, 1636268400, 1647158400, 1667718000, 1678608000, 1699167600,
        1710057600, 1730617200, 1741507200, 1762066800, 1772956800, 1793516400, 1805011200, 1825570800,
        1836460800, 1857020400, 1867910400, 1888470000, 1899360000, 1919919600, 1930809600, 1951369200,
        1962864000, 1983423600, 1994313600, 2014873200, 2025763200, 2046322800, 2057212800, 2077772400,
        2088662400, 2109222000, 2120112000, 2140671600, 2152166400, 2172726000, 2183616000, 2204175600,
        2215065600, 2235625200]),
    "Europe/Berlin": _listed(3600000, 7200000, [
        1585443600, 1603587600, 1616893200, 1635642000, 1648342800, 1667091600, 1679792400, 1698541200,
        1711846800, 1729990800, 1743296400, 1761440400, 1774746000, 1792890000, 1806195600, 1824944400,
        1837645200, 1856394000, 1869094800, 1887843600, 1901149200, 1919293200, 1932598800, 1950742800,
        1964048400, 1982797200, 1995498000, 2014246800, 2026947600, 2045696400, 2058397200, 2077146000,
        2090451600, 2108595600, 2121901200, 2140045200, 2153350800, 2172099600, 2184800400, 2203549200,
        2216250000, 2234998800]),
    "Australia/Lord_Howe": _listed(39600000, 37800000, [
        1586012400, 1601739000, 1617462000, 1633188600, 1648911600, 1664638200, 1680361200, 1696087800,
        1712415600, 1728142200, 1743865200, 1759591800, 1775314800, 1791041400, 1806764400, 1822491000,
        1838214000, 1853940600, 1869663600, 1885995000, 1901718000, 1917444600, 1933167600, 1948894200,
        1964617200, 1980343800, 1996066800, 2011793400, 2027516400, 2043243000, 2058966000, 2075297400,
        2091020400, 2106747000, 2122470000, 2138196600, 2153919600, 2169646200, 2185369200, 2201095800,
        2216818800, 2233150200]),
    # no transition in these years (Sao Paulo's summer time ended in 2019)
    "America/Sao_Paulo": (-10800000, []),
    "Asia/Kolkata": (19800000, []),
}


def zone_data(zone, listed=False):
    """(base offset, transitions) of a zone: from zoneinfo over 1990..2045, or the literals."""
    if re.fullmatch(r"[+-]\d\d:\d\d", zone):
        return fixed_offset_ms(zone), []
    if listed:
        return LISTED[zone]
    if zone not in _ZONE_DATA:
        _ZONE_DATA[zone] = (offset_at(zone, (dt.datetime(1990, 1, 1) - EPOCH) // MS), transitions(zone, 1990, 2045))
    return _ZONE_DATA[zone]


_ZONE_DATA = {}


# ---------------------------------------------------------------- the case table
FIXED_SHAPE, GENERIC = 0, 1
_STRICT = re.compile(r"\d{4}-\d{2}-\d{2} \d{2}:\d{2}:\d{2},\d{1,3}")


def render(fields, style=FIXED_SHAPE):
    """The log stamp for the fields: the fixed 10+12-byte shape, or unpadded numbers (the generic
    tokenizer path of the parse kernel; the same values)."""
    y, mo, d, h, mi, s, ms = fields
    if style == GENERIC:
        return f"{y}-{mo}-{d} {h}:{mi}:{s},{ms}"
    return f"{y:04d}-{mo:02d}-{d:02d} {h:02d}:{mi:02d}:{s:02d},{ms:03d}"


def is_strict(text):
    """The watermark rule: only a stamp of the exact log shape moves the batch clock."""
    return bool(_STRICT.fullmatch(text))


# text -> fields, for the cases the issue of this suite spells out as text
_SPELLED = (
    ("1999-12-31 23:59:59,999", (1999, 12, 31, 23, 59, 59, 999)),
    ("2028-02-29 00:00:00,000", (2028, 2, 29, 0, 0, 0, 0)),
    ("2100-02-28 23:59:59,999", (2100, 2, 28, 23, 59, 59, 999)),
    ("2100-03-01 00:00:00,000", (2100, 3, 1, 0, 0, 0, 0)),
    # fields that normalise across a transition (Chicago's 2026 ones; plain carries elsewhere)
    ("2026-03-07 26:30:00,000", (2026, 3, 7, 26, 30, 0, 0)),
    ("2026-11-00 25:30:00,000", (2026, 11, 0, 25, 30, 0, 0)),
    ("2026-13-01 00:00:00,000", (2026, 13, 1, 0, 0, 0, 0)),
    ("2026-03-08 01:59:60,000", (2026, 3, 8, 1, 59, 60, 0)),
    # the generic tokenizer path: a two-digit year is 19xx, unpadded fields, one-digit milliseconds
    ("26-03-08 02:30:00,000", (1926, 3, 8, 2, 30, 0, 0)),
    ("2026-3-8 2:30:0,5", (2026, 3, 8, 2, 30, 0, 5)),
    ("2026-03-08 01:59:59,7", (2026, 3, 8, 1, 59, 59, 7)),
    # six fields: new Date(y, m, d, h, mi, s, undefined) is NaN in every zone
    ("2026-03-08 02:30:00", None),
)


def cases(trans):
    """[(text, fields or None)] for a zone with these transitions; fields None: the result is NaN.
    Nothing here is typed as a date except what _SPELLED lists: the rest comes from ``trans``."""
    out = []
    for t, before, after in trans:
        if (EPOCH + t * MS).year not in TRANSITION_YEARS:
            continue
        lo, hi = t + min(before, after), t + max(before, after)  # the gap or overlap, local time
        for loc in (lo - 1, lo, (lo + hi) // 2, hi - 1, hi):
            f = fields_of_local(loc)
            out.append((render(f), f))
    for y in (1995, 2021, 2022, 2026, 2040):
        for mo in (1, 7):
            f = (y, mo, 1, 0, 0, 0, 0)
            out.append((render(f), f))
    out += list(_SPELLED)
    return out


def expected(zone, fields, listed=False):
    """Reference UTC ms as a float (NaN for fields None)."""
    if fields is None:
        return float("nan")
    if listed:
        base, trans = zone_data(zone, listed=True)
        return float(utc_ms_listed(base, trans, fields))
    return float(utc_ms(zone, fields))

"""Local time -> UTC in zones with summer time, on the CPU: the transition table that the parse
kernels and the host's js::convert_date search (ops/parse_ref.py tz_table -> kernels/common.h
TzTable / local_to_utc), the oracle's TzOffset and convert_string_date_to_ms, and the host join,
against the independent reference of tests/tz_ref.py (zoneinfo with fold=0; recorded answers of
node's ``new Date(y, m - 1, d, h, mi, s, ms)`` as a second one).  Every comparison is == on
integer-valued doubles."""
import bisect
import collections
import json
import math
import os
import shutil
import subprocess
import time
import warnings

import numpy as np
import pytest

import tz_ref as R
from tz_corpus import AUDIT_LOG, transition_corpus
from apmbackend_amd import _native
from apmbackend_amd.models.oracle import ParseOracle, file_kind
from apmbackend_amd.ops.parse_ref import TZ_FIRST_START, TZ_ROWS, parse_batch, tz_coverage, tz_rows, tz_table
from apmbackend_amd.utils import timeparse
from apmbackend_amd.utils.timeparse import TzOffset, convert_string_date_to_ms, parse_iso

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "tz_node.json")
KINDS = {"SOAP": 0, "SERVER": 1, "APP": 2}
# the centre of the one table an engine started in mid-2026 would build
CENTRE = R.local_ms((2026, 7, 1, 0, 0, 0, 0))

zoneinfo_only = pytest.mark.skipif(not R.have_zoneinfo(), reason="no zone database on this machine")

_TZ = {}


def tz_of(zone):
    if zone not in _TZ:
        _TZ[zone] = TzOffset(zone)
    return _TZ[zone]


def listed_tz(zone):
    base, trans = R.zone_data(zone, listed=True)
    return TzOffset.from_transitions(base, trans) if zone in R.LISTED else TzOffset(zone)


def table_utc(rows, loc):
    """A plain bisect over the rows: what local_to_utc (kernels/common.h) computes."""
    i = bisect.bisect_right([r[0] for r in rows], loc) - 1
    return float(loc - rows[i][1])


def same(a, b):
    return (a != a and b != b) or a == b


def check_rows(rows):
    assert 1 <= len(rows) <= TZ_ROWS and rows[0][0] == TZ_FIRST_START
    assert all(a[0] < b[0] and a[1] != b[1] for a, b in zip(rows, rows[1:]))


def check_case(N, tz, rows, text, fields, want, why):
    if fields is not None:
        assert table_utc(rows, R.local_ms(fields)) == want, ("table", text) + why
    got = N.js_convert_date(text, {"tz_table": rows})
    assert same(got, want), ("js::convert_date", text, got, want) + why
    got = convert_string_date_to_ms(text, tz)
    assert same(got, want), ("convert_string_date_to_ms", text, got, want) + why


@zoneinfo_only
@pytest.mark.parametrize("zone", R.ZONES + R.FIXED)
def test_table_host_and_oracle_match_reference(zone):
    """Every case of the case table: a bisect over the table's rows, the host's convert_date on
    those rows and the oracle's convert_string_date_to_ms all equal the reference.  The table is
    centred on the case's own year (the cases span 1926..2100, more than 64 rows hold), and
    again on mid-2026 for every case inside that table's stated coverage."""
    N = _native.load()
    tz = tz_of(zone)
    mid_rows, (lo, hi) = tz_coverage(tz, CENTRE)
    check_rows(mid_rows)
    n_mid = 0
    for text, fields in R.cases(R.zone_data(zone)[1]):
        want = R.expected(zone, fields)
        centre = CENTRE if fields is None else R.local_ms((fields[0], 1, 1, 0, 0, 0, 0))
        rows = tz_table(tz, centre)
        check_rows(rows)
        check_case(N, tz, rows, text, fields, want, (zone, "own year"))
        if fields is None or lo <= R.local_ms(fields) < hi:
            n_mid += 1
            check_case(N, tz, mid_rows, text, fields, want, (zone, "mid-2026"))
    # the mid-2026 table reaches every transition year of the case table
    assert n_mid >= len(R.cases(R.zone_data(zone)[1])) - 6


@pytest.mark.parametrize("zone", R.ZONES + R.FIXED)
def test_listed_zone_matches_listed_reference(zone):
    """The same with the zone given as data (TzOffset.from_transitions over the literals of
    tz_ref.LISTED), which needs no zone database: what the GPU tests run on."""
    N = _native.load()
    tz = listed_tz(zone)
    rows = tz_table(tz, CENTRE)
    check_rows(rows)
    assert len(rows) == 1 + len(R.zone_data(zone, listed=True)[1])
    for text, fields in R.cases(R.zone_data(zone, listed=True)[1]):
        check_case(N, tz, rows, text, fields, R.expected(zone, fields, listed=True), (zone, "listed"))


@zoneinfo_only
@pytest.mark.parametrize("zone", R.ZONES)
def test_listed_transitions_equal_zoneinfo(zone):
    base, trans = R.LISTED[zone]
    assert trans == R.transitions(zone, *R.LISTED_YEARS)
    assert base == R.offset_at(zone, R.local_ms((R.LISTED_YEARS[0], 1, 1, 0, 0, 0, 0)))
    # and the finder of the table builder sees the same transitions, to the millisecond
    found = [x for x in tz_of(zone).base_and_transitions()[1]
             if R.LISTED_YEARS[0] <= R.fields_of_local(x[0])[0] <= R.LISTED_YEARS[1]]
    assert found == trans


@zoneinfo_only
@pytest.mark.parametrize("zone", R.DST_ZONES)
def test_dense_sweep_over_the_tables_coverage(zone):
    """Every 30 minutes of local time over the stated coverage of the mid-2026 table, and every
    minute of each day with a transition in it: table == reference (and == TzOffset there)."""
    from zoneinfo import ZoneInfo
    zi = ZoneInfo(zone)
    tz = tz_of(zone)
    rows, (lo, hi) = tz_coverage(tz, CENTRE)
    assert len(rows) == TZ_ROWS
    years = (R.fields_of_local(lo)[0], R.fields_of_local(hi)[0])
    assert years[0] <= 2011 and years[1] >= 2042  # 32 transitions on each side of the centre
    starts = np.array([r[0] for r in rows], dtype=np.int64)
    offs = np.array([r[1] for r in rows], dtype=np.int64)

    def sweep(locs):
        got = offs[np.searchsorted(starts, locs, side="right") - 1]
        want = np.fromiter(((R.EPOCH + int(x) * R.MS).replace(tzinfo=zi).utcoffset() // R.MS for x in locs),
                           dtype=np.int64, count=len(locs))
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (zone, bad.size, [R.fields_of_local(int(locs[i])) for i in bad[:3]])

    first = -(-lo // 1800000) * 1800000
    sweep(np.arange(first, hi, 1800000, dtype=np.int64))
    days = sorted({(t + min(a, b)) // R.DAY_MS for t, a, b in R.transitions(zone, years[0], years[1])
                   if lo <= t + min(a, b) - R.DAY_MS and t + max(a, b) + R.DAY_MS < hi})
    assert len(days) >= 62
    minutes = np.concatenate([np.arange(d * R.DAY_MS, (d + 1) * R.DAY_MS, 60000, dtype=np.int64) for d in days])
    sweep(minutes)
    for loc in minutes[::7]:
        assert tz.local_to_utc(float(loc)) == table_utc(rows, int(loc))


def test_rows_rule_and_centre():
    """tz_rows is pure: row start T + max(before, after), 31 transitions kept before the centre and
    32 after it, spare rows given to the other side, and the coverage it states."""
    h = 3600000
    trans = [(i * 1000 * h, (-5 - i % 2) * h, (-6 + i % 2) * h) for i in range(1, 201)]
    rows, cover = tz_rows(-6 * h, trans, 100 * 1000 * h + 5)
    assert len(rows) == 64 and rows[0] == (TZ_FIRST_START, trans[69][1])
    assert rows[1:] == [(t + (-5) * h, b) for t, a, b in trans[69:132]]
    assert cover == (trans[68][0] - 5 * h, trans[132][0] - 5 * h)
    rows, cover = tz_rows(-6 * h, trans, 0)  # nothing before the centre: 63 after it
    assert rows[0] == (TZ_FIRST_START, -6 * h) and len(rows) == 64 and rows[-1][0] == trans[62][0] - 5 * h
    assert cover == (TZ_FIRST_START, trans[63][0] - 5 * h)
    rows, cover = tz_rows(-6 * h, trans, 10 ** 15)  # nothing after it: the last 63
    assert rows[1][0] == trans[137][0] - 5 * h and cover == (trans[136][0] - 5 * h, -TZ_FIRST_START)
    rows, cover = tz_rows(-6 * h, trans[:5], 0)
    assert len(rows) == 6 and cover == (TZ_FIRST_START, -TZ_FIRST_START)
    assert tz_rows(7 * h, [], 0) == ([(TZ_FIRST_START, 7 * h)], (TZ_FIRST_START, -TZ_FIRST_START))


def test_more_than_64_rows_is_an_error_and_a_warning(monkeypatch):
    from apmbackend_amd.ops import parse_ref
    N = _native.load()
    with pytest.raises(Exception):
        N.js_convert_date("2026-03-08 02:30:00,000", {"tz_table": [(i, i) for i in range(65)]})
    warned = []
    monkeypatch.setattr(parse_ref.log, "warning", lambda msg, *args: warned.append(msg % args))
    h = 3600000
    trans = [(i * 1000 * h, (-5 - i % 2) * h, (-6 + i % 2) * h) for i in range(1, 201)]
    monkeypatch.setattr(parse_ref, "_warned", set())
    big = TzOffset.from_transitions(-6 * h, trans)
    assert len(tz_table(big, 0)) == 64
    assert len(warned) == 1 and "200 transitions" in warned[0]
    tz_table(big, 0)  # the same zone and span again (a reload): said once
    assert len(warned) == 1
    tz_table(big, 10 ** 15)  # another span
    assert len(warned) == 2
    del warned[1:]
    tz_table(listed_tz("America/Chicago"), CENTRE)  # 42 transitions: they fit
    tz_table(TzOffset("-06:00"), CENTRE)
    assert len(warned) == 1


@zoneinfo_only
@pytest.mark.parametrize("zone", R.ZONES + R.FIXED)
def test_offset_for_utc_around_every_transition(zone):
    """offset_ms_for_utc (the synthetic corpora write their stamps with it) is the offset of the
    aware instant, 1 ms before, at and 1 ms after every transition of 1990..2045."""
    tz = tz_of(zone)
    base, trans = R.zone_data(zone)
    assert zone not in R.DST_ZONES or len(trans) > 100
    for t, before, after in trans:
        assert [tz.offset_ms_for_utc(u) for u in (t - 1, t, t + 1)] == [before, after, after]
        assert [R.offset_at(zone, u) for u in (t - 1, t, t + 1)] == [before, after, after]
    for u in (0, CENTRE, CENTRE + 0.5):
        assert tz.offset_ms_for_utc(u) == R.offset_at(zone, int(u))
    ltz = listed_tz(zone)
    lbase, ltrans = R.zone_data(zone, listed=True)
    for t, _, _ in ltrans:
        for u in (t - 1, t, t + 1):
            assert ltz.offset_ms_for_utc(u) == R.offset_at_listed(lbase, ltrans, u) == R.offset_at(zone, u)


# ---------------------------------------------------------------- ISO stamps
NO_ZONE = (("2026-07-01T10:00:01.959", (2026, 7, 1, 10, 0, 1, 959)),
           ("2026-11-01T01:30:00", (2026, 11, 1, 1, 30, 0, 0)),     # repeated in Chicago
           ("2026-03-08T02:30", (2026, 3, 8, 2, 30, 0, 0)),         # skipped in Chicago
           ("2026-03-29T02:30:00.5", (2026, 3, 29, 2, 30, 0, 500)),  # skipped in Berlin
           ("2026-01-01T00:00:00.000", (2026, 1, 1, 0, 0, 0, 0)))
OWN_ZONE = (("2026-11-01T01:30:00.000-06:00", "-06:00", (2026, 11, 1, 1, 30, 0, 0)),
            ("2026-11-01T01:30:00.000-05:00", "-05:00", (2026, 11, 1, 1, 30, 0, 0)),
            ("2026-03-08T02:30:00.959-06:00", "-06:00", (2026, 3, 8, 2, 30, 0, 959)),
            ("2026-07-01T10:00:01.959Z", None, None),
            ("2026-07-01T10:00:01.959+05:30", None, None))


@pytest.fixture
def utc_process(monkeypatch):
    """APM_TZ unset and the process zone UTC: nothing but the zone handed in can give the answer."""
    monkeypatch.delenv("APM_TZ", raising=False)
    monkeypatch.setenv("TZ", "UTC")
    time.tzset()
    monkeypatch.setattr(timeparse, "_DEFAULT_TZ", None)
    yield
    monkeypatch.undo()
    time.tzset()


@zoneinfo_only
@pytest.mark.parametrize("zone", R.ZONES + R.FIXED)
def test_iso_stamps_without_a_zone(zone, utc_process):
    """parse_iso reads a stamp without an offset as local time in the zone it is handed.  Through
    convertStringDateToMs no such stamp gets that far: its test /T.*-/ wants a '-' after the T,
    which only an offset supplies, so the stamp is split as a log date, one of whose fields is
    then no number, and is NaN -- in the oracle and on the host, whatever the zone.  (The
    zone-less branches of parse_iso and of the host's js::parse_iso are therefore unreachable
    from the pipeline; docs/ARCHITECTURE.md says so.)"""
    N = _native.load()
    tz = tz_of(zone)
    rows = tz_table(tz, CENTRE)
    for text, fields in NO_ZONE:
        assert parse_iso(text, tz) == R.utc_ms(zone, fields), (zone, text)
        assert math.isnan(convert_string_date_to_ms(text, tz)), (zone, text)
        assert math.isnan(N.js_convert_date(text, {"tz_table": rows})), (zone, text)
    assert parse_iso("2026-07-01T10:00:01.959") == R.utc_ms("+00:00", NO_ZONE[0][1])  # no zone given: the process zone


@zoneinfo_only
@pytest.mark.parametrize("zone", R.ZONES + R.FIXED)
def test_iso_stamps_with_their_own_zone(zone, utc_process):
    """A stamp with an offset is the same instant in every configured zone; 'Z' and '+HH:MM' have
    no '-' after the T, so convertStringDateToMs makes them NaN, in every zone."""
    N = _native.load()
    tz = tz_of(zone)
    rows = tz_table(tz, CENTRE)
    for text, own, fields in OWN_ZONE:
        want = float("nan") if own is None else float(R.utc_ms(own, fields))
        assert same(convert_string_date_to_ms(text, tz), want), (zone, text)
        assert same(N.js_convert_date(text, {"tz_table": rows}), want), (zone, text)
        if own is not None:
            assert parse_iso(text, tz) == want


# ---------------------------------------------------------------- node as a second reference
NODE_JS = r"""
const req = JSON.parse(require('fs').readFileSync(0, 'utf8'));
console.log(JSON.stringify({
  offsets: [new Date(2026, 0, 1).getTimezoneOffset(), new Date(2026, 6, 1).getTimezoneOffset()],
  dates: req.fields.map((f) => new Date(f[0], f[1] - 1, f[2], f[3], f[4], f[5], f[6]).getTime()),
}));
"""


def node_request(zone):
    return {"fields": [list(f) for _, f in R.cases(R.zone_data(zone)[1]) if f is not None]}


def node_answer(zone, req):
    r = subprocess.run(["node", "-e", NODE_JS], input=json.dumps(req), capture_output=True,
                       text=True, env=dict(os.environ, TZ=zone), timeout=120, check=True)
    return json.loads(r.stdout)


@zoneinfo_only
@pytest.mark.parametrize("zone", R.ZONES)
def test_node_agrees_with_the_reference(zone):
    """``new Date(y, m - 1, d, h, mi, s, ms).getTime()`` from a node process started with TZ=zone,
    over every time of the case table, equals the reference.  The answers are recorded in
    tests/golden/tz_node.json (APM_REF_RECORD=1 records them again); where node is installed it
    is asked again, and a node that does not honour TZ is reported with a warning."""
    req = node_request(zone)
    if os.environ.get("APM_REF_RECORD"):
        rec = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
        rec[zone] = {"request": req, "answer": node_answer(zone, req)}
        with open(GOLDEN, "w") as fh:
            json.dump(rec, fh, separators=(",", ":"), sort_keys=True)
            fh.write("\n")
    with open(GOLDEN) as fh:
        rec = json.load(fh)[zone]
    assert rec["request"] == req, "the case table changed: record node's answers again"
    answers = [rec["answer"]]
    # minutes west of UTC on 1 January and 1 July, as getTimezoneOffset gives them
    want_offsets = [-R.offset_at(zone, R.local_ms((2026, mo, 1, 12, 0, 0, 0))) // 60000 for mo in (1, 7)]
    assert rec["answer"]["offsets"] == want_offsets
    if shutil.which("node"):
        live = node_answer(zone, req)
        if live["offsets"] == want_offsets:
            answers.append(live)
        else:
            warnings.warn(f"node here does not honour TZ={zone} (getTimezoneOffset {live['offsets']}, zone "
                          f"{want_offsets}): only its recorded answers were compared")
    for ans in answers:
        assert ans["dates"] == [R.utc_ms(zone, f) for f in req["fields"]]


# ---------------------------------------------------------------- the host join across a transition
def test_host_join_across_the_autumn_transition():
    """The C++ host join with Chicago's table on traffic that starts 45 minutes before the 2026
    autumn transition: local times inside the repeated hour, which belong to the offset from
    before the transition, and audit stamps with an offset, with 'Z' and without a zone, some on
    lines the host reads itself.  Output == the oracle's, line for line."""
    N = _native.load()
    base, trans = R.LISTED["America/Chicago"]
    t_autumn = [t for t, a, b in trans if R.fields_of_local(t)[0] == 2026 and b < a][0]
    tz = TzOffset.from_transitions(base, trans)
    start = t_autumn - 45 * 60000
    lines, bl = transition_corpus(tz, start, 100, seed=4)
    # the stamps are in the repeated hour and the clock is the true instant
    assert all(" 2026-11-01 01:15:" in x[2] for x in lines[AUDIT_LOG][:1])
    assert all(start < now < start + 200_000 for now, _ in bl[1:20])  # (an hour off is 3 600 000)
    want = []
    po = ParseOracle(lambda q, l: want.append((q, l)), tz=tz)
    for now, chunks in bl:
        po.begin_batch(now)
        for fp, ls in chunks:
            for ln in ls:
                po.read_line(fp, ln)
    h = N.JoinHarness({"tz_table": tz_table(tz, start)})
    fid = {fp: h.add_file(fp, KINDS[file_kind(fp)], fp.split("/")[2]) for fp in sorted(lines)}
    got, fo = [], {}
    for now, chunks in bl:
        bch = [(KINDS[file_kind(fp)], ("\n".join(ls) + "\n").encode()) for fp, ls in chunks]
        cf = [fid[fp] for fp, _ in chunks]
        ev, _, _, buf = parse_batch(bch, tz, fo, cf)
        got += h.process(ev.tobytes(), buf, cf, now)
    assert len(want) > 300 and sum("|jvm90|" in l for _, l in want) > 50
    assert h.counters()["host_fallback"] > 0  # the host's own date conversion ran
    assert collections.Counter(want) == collections.Counter(got)
    assert want == got

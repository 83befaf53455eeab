"""The device join's boundary corpora (tests/join_cases.py) on the CPU: the case tables prove the
tiers they claim, the oracle agrees with the reference's own JavaScript on every case (recorded
answers, tests/golden/refjs/), and the C++ host join agrees with the oracle."""
import pytest

import join_cases as J
import refjs
from apmbackend_amd import _native
from apmbackend_amd.models.oracle import file_kind
from apmbackend_amd.ops.parse_ref import parse_batch, tz_table


def first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"entry {i}:\n  got  {g!r}\n  want {w!r}"
    if len(got) != len(want):
        return f"{len(got)} entries, want {len(want)}"
    return None


def test_constants_are_the_kernels_own():
    """The mirrored constants against the sources they name."""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc", "kernels")
    text = open(os.path.join(root, "devjoin.hip")).read() + open(os.path.join(root, "devjoin_types.h")).read()
    for name in ("GW_SMALL", "GWB_LDS", "TXW_LINES", "TXW_LDS", "KS_PARTS", "PBLK_N", "NEED_ITEMS", "NBLK_N",
                 "NEED_LID", "LBLK_N"):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+);" % name, text)
        assert m and int(m.group(1)) == getattr(J, name), name


def test_case_tables_list_every_size():
    assert J.GROUP_SIZES == [1, 2, J.GW_SMALL - 1, J.GW_SMALL, J.GW_SMALL + 1, 2 * J.GW_SMALL - 1, 2 * J.GW_SMALL,
                             2 * J.GW_SMALL + 1, J.GWB_LDS - 1, J.GWB_LDS, J.GWB_LDS + 1]
    assert J.OPEN_COUNTS == [J.KS_PARTS - 1, J.KS_PARTS, J.KS_PARTS + 1, J.KS_PARTS + J.PBLK_N - 1,
                             J.KS_PARTS + J.PBLK_N, J.KS_PARTS + J.PBLK_N + 1, J.KS_PARTS + 2 * J.PBLK_N,
                             J.KS_PARTS + 2 * J.PBLK_N + 1]
    assert J.PARKED_COUNTS == [1, 2, 3, J.NEED_ITEMS - 1, J.NEED_ITEMS, J.NEED_ITEMS + 1, J.NEED_ITEMS + J.NBLK_N - 1,
                               J.NEED_ITEMS + J.NBLK_N, J.NEED_ITEMS + J.NBLK_N + 1, J.NEED_ITEMS + 2 * J.NBLK_N + 1]
    assert J.LOGID_LENGTHS == [1, J.NEED_LID - 1, J.NEED_LID, J.NEED_LID + 1, J.NEED_LID + J.LBLK_N - 1,
                               J.NEED_LID + J.LBLK_N, J.NEED_LID + J.LBLK_N + 1, J.NEED_LID + 2 * J.LBLK_N,
                               J.NEED_LID + 2 * J.LBLK_N + 1]
    assert J.WRITE_TOTALS == list(range(J.TXW_LDS - 4, J.TXW_LDS + 5))
    assert (J.RECORD_TTL, J.ACCT_TTL, J.NEED_TTL) == (120000, 120000, 30000)


@pytest.mark.parametrize("name", J.CASE_NAMES)
def test_case_proves_its_tiers(name):
    case = J.get_case(name)
    tiers = J.prove(case)
    assert tiers and all(tiers.values()), (name, tiers)
    assert all(ls for _now, ch in case.batches for _fp, ls in ch)
    assert case.n_lines() <= (13000 if name == "group_sizes" else 4000)


@pytest.mark.parametrize("name", J.REFERENCE_CASES)
def test_oracle_matches_reference_js(name):
    """ParseOracle == the reference's stream_parse_transactions.js on the case, record for record."""
    case = J.get_case(name)
    ref = refjs.parse(case.batches)
    assert ref["errors"] == []
    want = [tuple(x) for x in ref["records"]]
    got = [(q, l) for _b, q, l in case.replay().records]
    diff = first_difference(got, want)
    assert diff is None, f"{name}: oracle differs from the reference at " + diff


def run_host(case):
    N = _native.load()
    h = N.JoinHarness({"tz_table": tz_table(J.UTC)})
    files = sorted({fp for _now, ch in case.batches for fp, _ls in ch})
    fid = {fp: h.add_file(fp, J.KINDS[file_kind(fp)], fp.split("/")[2]) for fp in files}
    got, fo = [], {}
    for now, chunks in case.batches:
        bch = [(J.KINDS[file_kind(fp)], ("\n".join(ls) + "\n").encode()) for fp, ls in chunks]
        cf = [fid[fp] for fp, _ in chunks]
        ev, _, _, buf = parse_batch(bch, J.UTC, fo, cf)
        got += h.process(ev.tobytes(), buf, cf, now)
    return got, h.counters()


@pytest.mark.parametrize("name", J.CASE_NAMES)
def test_host_join_matches_oracle(name):
    """csrc/runtime/join.cpp through JoinHarness (as tests/test_join_native.py::run_both) == the oracle."""
    case = J.get_case(name)
    R = case.replay()
    got, nc = run_host(case)
    diff = first_difference(got, [(q, l) for _b, q, l in R.records])
    assert diff is None, f"{name}: host join differs from the oracle at " + diff
    for k in ("need_expired", "expired_partials", "ejb_exit_unmatched", "invalid_acct"):
        assert nc[k] == R.counters[k], (name, k, nc[k], R.counters[k])
    if case.plain:
        assert nc["host_fallback"] == 0

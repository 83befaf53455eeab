"""The device join (K4/K5/K6, devjoin.hip + devjoin.cpp) on the boundary corpora of
tests/join_cases.py: every stream against PipelineOracle in order, the join's counters against the
oracle's, and the chain-block allocations against what the case computes from its own sizes
(join_cases.prove shows on the CPU that each case reaches the tiers it names)."""
import collections
import copy

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU containers
    pytest.skip("no GPU", allow_module_level=True)

import join_cases as J  # noqa: E402
from apmbackend_amd.models.oracle import PipelineOracle  # noqa: E402
from apmbackend_amd.models.pipeline import APMEngine  # noqa: E402
from test_engine_gpu import small_cfg  # noqa: E402

STREAMS = ("transactions", "audit_db", "st", "fs", "al")
_ORACLE = {}


def oracle_of(case):
    """PipelineOracle over the case (once per case): its streams and the output sizes per batch."""
    if case.name not in _ORACLE:
        P = PipelineOracle(copy.deepcopy(small_cfg("exact")), J.UTC)
        marks = []
        for b in case.batches:
            P.run_batches([b])
            marks.append({"transactions": len(P.tx_out), "audit_db": len(P.audit_db), "st": len(P.stats),
                          "fs": len(P.fs), "al": len(P.al)})
        want = {"transactions": P.tx_out, "audit_db": P.audit_db, "st": P.stats, "fs": P.fs, "al": P.al}
        R = case.replay()
        assert P.tx_out == R.stream("transactions") and P.audit_db == R.stream("db_insert")
        _ORACLE[case.name] = (want, marks, dict(P.parse.counters))
    return _ORACLE[case.name]


def run_engine(case, tmp_path=None):
    """The batches through APMEngine as test_engine_gpu._run_engine feeds them; with tmp_path, the
    state is saved after case.save_after batches and a fresh engine continues from it."""
    C = small_cfg("exact")
    assert C["gpu"].get("joinOnDevice", True)
    eng = APMEngine(C, keep_text=True)
    out = collections.defaultdict(list)
    for i, (now, chunks) in enumerate(case.batches):
        if tmp_path is not None and i == case.save_after:
            ck = str(tmp_path / "join.ckpt")
            assert eng.save_state(ck) > 0
            del eng
            eng = APMEngine(small_cfg("exact"), keep_text=True)
            eng.load_state(ck)
        eng.process_lines(chunks, now)
        for k in STREAMS:
            out[k] += eng.take(k)
    return eng, out


def assert_streams(case, out):
    want, marks, _c = oracle_of(case)
    for k in STREAMS:
        got, w = out[k], want[k]
        d = next((i for i, (a, b) in enumerate(zip(got, w)) if a != b), min(len(got), len(w)))
        if d < max(len(got), len(w)):
            at = next((b for b, m in enumerate(marks) if m[k] > d), len(marks))
            bad = sum(1 for a, b in zip(got, w) if a != b)
            pytest.fail(f"case {case.name}: {k} stream differs first at line {d} (batch {at}; {bad} lines differ, "
                        f"{len(got)} vs {len(w)}): {got[d][:200] if d < len(got) else None!r} != "
                        f"{w[d][:200] if d < len(w) else None!r}")


@pytest.mark.parametrize("name", J.CASE_NAMES)
def test_device_join_case(name):
    case = J.get_case(name)
    _want, _marks, oc = oracle_of(case)
    eng, out = run_engine(case)
    assert_streams(case, out)
    j = eng.metrics()["join"]
    for k in ("expired_partials", "need_expired", "ejb_exit_unmatched", "invalid_acct"):
        assert j[k] == oc[k], (name, k, j[k], oc[k])
    for k in ("partial_overflow", "need_overflow", "table_full", "pool_exhausted"):
        assert j[k] == 0, (name, k, j[k])
    for k, n in case.replay().blocks.items():
        assert j[k] == n, (name, k, j[k], n)
    if case.plain:
        assert j["host_fallback"] == 0


@pytest.mark.parametrize("name", J.SAVE_CASES)
def test_device_join_case_across_a_checkpoint(name, tmp_path):
    """save_state at the batch boundary with the most chain state live (open PartBlk chains, parked
    NeedBlk chains, LidBlk chains), load_state into a fresh engine, the same streams."""
    case = J.get_case(name)
    assert case.save_after is not None
    _eng, out = run_engine(case, tmp_path)
    assert_streams(case, out)

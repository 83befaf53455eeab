"""The tk stream through the whole engine: parse -> device join -> K7 -> K8 -> K18, against the
CPU oracle at every rollover; the other streams unchanged by it; the service's route to
gpu.topQueue; the engine's resources returned.  (Shapes of tests/test_slo_engine_gpu.py.)"""
import collections
import copy
import gc

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

from apmbackend_amd import _native  # noqa: E402
from apmbackend_amd.models.oracle import PipelineOracle  # noqa: E402
from apmbackend_amd.models.pipeline import ENGINE_OUT_KINDS, NATIVE_OUT_KINDS, APMEngine, engine_config  # noqa: E402
from apmbackend_amd.runtime.amqp_broker import Broker  # noqa: E402
from apmbackend_amd.runtime.service import IngestService  # noqa: E402

import topk_ref as R  # noqa: E402
from test_hist_engine_gpu import KINDS, UTC, run, small_cfg, synth_batches  # noqa: E402
from test_service import feed_in_steps, make_env, srv_of  # noqa: E402
from test_service_gpu import gpu_cfg  # noqa: E402

BOARD = {"k": 4, "by": ["per95", "average", "tpm"], "minTpm": 0.5}


def top_cfg(board=BOARD):
    C = small_cfg()
    C["gpu"]["leaderboard"] = copy.deepcopy(board)
    return C


def test_stream_is_opt_in():
    assert NATIVE_OUT_KINDS == ENGINE_OUT_KINDS + ("tk",)
    eng = APMEngine(top_cfg(), keep_text=True)   # the key in the config alone does not start it
    assert not (eng.ecfg["outputs"] >> NATIVE_OUT_KINDS.index("tk")) & 1
    assert eng.eng.leaderboard() == []
    with pytest.raises(ValueError):
        APMEngine(small_cfg(), outputs=("st", "tk"))
    # the native constructor checks what it is handed as well
    N = _native.load()
    ecfg = engine_config(top_cfg(), outputs=("st", "tk"))
    for bad in ({"tk_k": 0}, {"tk_k": 129}, {"tk_k": None}, {"tk_by": []}, {"tk_by": [0, 0]}, {"tk_by": [4]},
                {"tk_by": [-1]}, {"tk_by": [0, 1, 2, 3, 0]}, {"tk_min_tpm": -1.0}, {"tk_min_tpm": float("nan")},
                {"tk_min_tpm": float("inf")}):
        with pytest.raises(ValueError):
            N.Engine(dict(ecfg, **bad))


def test_full_pipeline_matches_the_cpu_engine_and_changes_nothing_else():
    _lines, bl = synth_batches(seed=1, duration=300)
    C = top_cfg()
    kinds = KINDS + ("tk",)
    eng, on = run(C, bl, kinds, kinds=kinds)
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)

    def by_rollover(rows):
        out = collections.OrderedDict()
        for r in rows:
            out.setdefault(r.split("|")[1], []).append(r)
        return out

    got_r, want_r = by_rollover(on["tk"]), by_rollover(P.tk)
    assert list(got_r) == list(want_r) and len(want_r) > 10 and len(P.tk) > 100
    for ts in want_r:   # every rollover on its own
        assert got_r[ts] == want_r[ts], ts
    last_ts = on["tk"][-1].split("|")[1]
    last = [r.split("|") for r in on["tk"] if r.split("|")[1] == last_ts]
    assert [(b, r) for b, r, *_ in eng.eng.leaderboard()] == [(f[2], int(f[3])) for f in last]
    _e, off = run(small_cfg(), bl, KINDS, kinds=KINDS + ("tk",))
    assert off["tk"] == [] and _e.eng.leaderboard() == []
    for k in ("st", "fs", "al", "audit_db", "transactions"):
        assert on[k] == off[k], k
    assert collections.Counter(on["db"]) == collections.Counter(off["db"]) and len(on["db"]) > 100
    assert on["st"] == P.stats
    # ... and the rows follow from the st rows alone
    by_ts = collections.OrderedDict()
    for r in on["st"]:
        by_ts.setdefault(r.split("|")[1], []).append(r)
    want = []
    for rows in by_ts.values():
        want += R.rows_from_st(rows, BOARD["k"], BOARD["by"], BOARD["minTpm"])
    assert on["tk"] == want


def test_with_st_and_fs_off_the_stream_uploads_its_own_order():
    _lines, bl = synth_batches(seed=5, duration=200)
    C = top_cfg({"k": 128, "by": ["tpm", "per75"]})
    _e, on = run(C, bl, ("tk",), kinds=("tk",))
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    assert on["tk"] == P.tk and len(P.tk) > 100


def test_service_routes_the_rows_to_the_queue(tmp_path):
    b = Broker(port=0).start()
    try:
        C, lines, mapping, sc = make_env(tmp_path, mode="amqp", duration=200)
        gpu_cfg(C)
        C["amqpConnectionString"] = b.url
        C["gpu"]["leaderboard"] = {"k": 5, "by": ["average"]}
        C["gpu"]["topQueue"] = "top_rows"
        svc = IngestService(C, engine="native", files=sorted(mapping.values()), rank=0, world=1, server_of_path=srv_of)
        assert svc.outputs[-1] == "tk"
        P = PipelineOracle(copy.deepcopy(C), UTC, server_fn=srv_of)
        feed_in_steps(svc, lines, mapping, sc, P)
        svc.shutdown()
        st = b.stats()
        assert len(P.tk) > 20 and 20 < st["top_rows"]["messages"] <= len(P.tk)
        assert st["db_insert"]["messages"] > 0 and "leaderboard" not in st
    finally:
        b.stop()


def test_resources_return_after_the_engine():
    COUNTS = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes", "events", "streams")
    gc.collect()
    N = _native.load()
    before = dict(N.live_resources())
    _lines, bl = synth_batches(seed=3, duration=150)
    kinds = KINDS + ("tk",)
    eng, out = run(top_cfg(), bl, kinds, kinds=kinds)
    assert len(out["tk"]) > 10
    during = dict(N.live_resources())
    assert during["device_bytes"] - before["device_bytes"] == eng.eng.device_bytes()
    plain, _o = run(small_cfg(), bl, KINDS)
    assert eng.eng.device_bytes() > plain.eng.device_bytes()   # the stream's memory is accounted for
    del eng, out, plain, _o
    gc.collect()
    after = dict(N.live_resources())
    assert {k: after[k] for k in COUNTS} == {k: before[k] for k in COUNTS}

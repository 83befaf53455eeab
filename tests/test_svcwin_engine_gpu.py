"""The sv stream through the whole engine: parse -> device join -> K7 -> K8 -> K19, against
PipelineOracle over several rollovers; with wp, sl and tk on as well; the other streams unchanged
by it; a checkpoint taken mid-run; the engine's resources returned.  (Shapes of
tests/test_winpct_engine_gpu.py.)"""
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
from apmbackend_amd.models.pipeline import DEVICE_OUT_KINDS, NATIVE_OUT_KINDS, APMEngine, engine_config  # noqa: E402
from apmbackend_amd.utils.synth import Generator, SynthConfig, batches, with_watermarks  # noqa: E402

import svcwin_ref as R  # noqa: E402
from test_hist_engine_gpu import KINDS, UTC, run, small_cfg  # noqa: E402

PCTS = [50, 75, 95, 99]
QS = [50000, 75000, 95000, 99000]


def svc_cfg(extra=False):
    C = small_cfg()
    C["gpu"]["serviceWindow"] = {"percentiles": list(PCTS)}
    if extra:
        C["gpu"]["windowPercentiles"] = [50, 99.9]
        C["gpu"]["latencyObjectives"] = {"default": [200, 1000]}
        C["gpu"]["leaderboard"] = {"k": 4, "by": ["per95", "tpm"]}
    return C


def synth3(seed=1, duration=200):
    """3 servers, 20 services: every service on every server."""
    cfg = SynthConfig(servers=3, duration_s=duration, tx_per_sec_per_server=4, seed=seed, ejb_services=12,
                      provider_services=8)
    lines = Generator(cfg).generate()
    return with_watermarks(batches(lines, cfg.start_ms, 5.0), UTC)


def test_stream_is_opt_in():
    assert DEVICE_OUT_KINDS == NATIVE_OUT_KINDS + ("sv",)
    eng = APMEngine(svc_cfg(), keep_text=True)   # the key in the config alone does not start it
    assert not (eng.ecfg["outputs"] >> DEVICE_OUT_KINDS.index("sv")) & 1
    assert eng.eng.svcwins() == []
    with pytest.raises(ValueError):
        APMEngine(small_cfg(), outputs=("st", "sv"))
    bad = small_cfg()
    bad["gpu"]["serviceWindow"] = {"percentiles": [99, 50]}
    with pytest.raises(ValueError):
        APMEngine(bad, outputs=("st", "sv"))
    # the native constructor checks the list it is handed as well
    N = _native.load()
    ecfg = engine_config(svc_cfg(), outputs=("st", "sv"))
    for lst in ([], [50000, 50000], [0], [100001], list(range(1, 10))):
        with pytest.raises(ValueError):
            N.Engine(dict(ecfg, svc_pcts=lst))


def test_full_pipeline_matches_oracle_and_changes_nothing_else():
    bl = synth3(seed=1)
    C = svc_cfg()
    kinds = KINDS + ("sv",)
    eng, on = run(C, bl, kinds, kinds=kinds)
    _e, off = run(small_cfg(), bl, KINDS, kinds=KINDS + ("sv",))
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    assert len(P.sv) > 100 and len({r.split("|")[2] for r in P.sv}) >= 15
    assert max(int(r.split("|")[3]) for r in P.sv) == 3
    assert on["sv"] == P.sv
    assert off["sv"] == [] and _e.eng.svcwins() == []
    for k in ("st", "fs", "al", "audit_db", "transactions"):
        assert on[k] == off[k], k
    assert collections.Counter(on["db"]) == collections.Counter(off["db"]) and len(on["db"]) > 100
    assert on["st"] == P.stats
    # servers and the row order follow from the st rows alone: per timestamp a service's st rows,
    # the services in the order of their first one
    cnt = collections.OrderedDict()
    for l in on["st"]:
        f = l.split("|")
        cnt[(f[1], f[3])] = cnt.get((f[1], f[3]), 0) + 1
    assert [int(r.split("|")[3]) for r in on["sv"]] == [cnt[tuple(r.split("|")[1:3])] for r in on["sv"]]
    keys = [tuple(r.split("|")[1:3]) for r in on["sv"]]
    assert keys == [k for k in cnt if k in set(keys)]
    # the read-back holds the last rollover's records
    last_ts = on["sv"][-1].split("|")[1]
    last = {r.split("|")[2]: r.split("|") for r in on["sv"] if r.split("|")[1] == last_ts}
    dev = {d[0]: d for d in eng.eng.svcwins()}
    for svc, f in last.items():
        assert dev[svc][1:5] == (int(f[3]), int(f[4]), int(f[5]), int(f[6])), svc
        assert [R.half(v) for v in dev[svc][5]] == [p.split(":")[1] for p in f[7].split(",")]


def test_with_the_other_window_streams_on_all_are_right():
    bl = synth3(seed=5, duration=150)
    C = svc_cfg(extra=True)
    kinds = KINDS + ("wp", "sl", "tk", "sv")
    _e, on = run(C, bl, kinds, kinds=kinds)
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    assert min(len(P.sv), len(P.wp), len(P.sl), len(P.tk)) > 50
    assert on["sv"] == P.sv and on["wp"] == P.wp and on["sl"] == P.sl and on["tk"] == P.tk and on["st"] == P.stats
    _e, off = run(small_cfg(), bl, KINDS)
    for k in ("st", "fs", "al"):
        assert on[k] == off[k], k


def test_checkpoint_resumes_the_stream(tmp_path):
    bl = synth3(seed=6, duration=200)
    C = svc_cfg()
    kinds = KINDS + ("sv",)
    _e, full = run(C, bl, kinds, kinds=kinds)
    cut = len(bl) // 2
    eng, head = run(C, bl[:cut], kinds, kinds=kinds)
    ck = str(tmp_path / "engine.ckpt")
    assert eng.save_state(ck) > 0
    del eng
    eng2 = APMEngine(C, outputs=kinds)
    eng2.load_state(ck)
    _e, tail = run(C, bl[cut:], kinds, eng=eng2, kinds=kinds)
    assert len(tail["sv"]) > 20 and len(head["sv"]) > 20
    assert head["sv"] + tail["sv"] == full["sv"]
    assert head["st"] + tail["st"] == full["st"]


def test_resources_return_after_the_engine():
    COUNTS = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes", "events", "streams")
    gc.collect()
    N = _native.load()
    before = dict(N.live_resources())
    bl = synth3(seed=3, duration=100)
    kinds = KINDS + ("sv",)
    eng, out = run(svc_cfg(), bl, kinds, kinds=kinds)
    assert len(out["sv"]) > 10
    during = dict(N.live_resources())
    assert during["device_bytes"] - before["device_bytes"] == eng.eng.device_bytes()
    plain, _o = run(small_cfg(), bl, KINDS)
    assert eng.eng.device_bytes() > plain.eng.device_bytes()   # the stream's memory is accounted for
    del eng, out, plain, _o
    gc.collect()
    after = dict(N.live_resources())
    assert {k: after[k] for k in COUNTS} == {k: before[k] for k in COUNTS}

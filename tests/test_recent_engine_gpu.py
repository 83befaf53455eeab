"""The rw stream through the whole engine: parse -> device join -> K7 -> K8 -> K20, against
PipelineOracle over several rollovers; with lh, wp, sl, tk and sv on as well; the other streams
unchanged by it; a checkpoint taken mid-run; the service's routes to gpu.recentQueue and to the
table; slot reuse and regrow of a used text slot; the engine's resources returned.  (Shapes of
tests/test_svcwin_engine_gpu.py and tests/test_text_streams_gpu.py.)"""
import collections
import copy
import gc
import os

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

from apmbackend_amd import _native  # noqa: E402
from apmbackend_amd.models.oracle import PipelineOracle  # noqa: E402
from apmbackend_amd.models.pipeline import DEVICE_OUT_KINDS, STREAM_OUT_KINDS, APMEngine, engine_config  # noqa: E402
from apmbackend_amd.runtime.amqp_broker import Broker  # noqa: E402
from apmbackend_amd.runtime.service import IngestService  # noqa: E402

import recent_ref as R  # noqa: E402
from test_hist_engine_gpu import KINDS, UTC, run, small_cfg  # noqa: E402
from test_service import feed_in_steps, make_env, srv_of  # noqa: E402
from test_service_gpu import gpu_cfg  # noqa: E402
from test_svcwin_engine_gpu import synth3  # noqa: E402
from test_text_streams_gpu import HEAVY_ROW, build_batches, streams_cfg  # noqa: E402

KEY = {"buckets": [1, 6], "percentiles": [50, 95, 99]}
EXTRA = ("lh", "wp", "sl", "tk", "sv")


def rw_cfg(extra=False):
    C = small_cfg()
    C["gpu"]["recentWindows"] = copy.deepcopy(KEY)
    if extra:
        C["gpu"]["latencyHistogram"] = True
        C["gpu"]["windowPercentiles"] = [50, 99.9]
        C["gpu"]["latencyObjectives"] = {"default": [200, 1000]}
        C["gpu"]["leaderboard"] = {"k": 4, "by": ["per95", "tpm"]}
        C["gpu"]["serviceWindow"] = {"percentiles": [50, 75, 95, 99]}
    return C


def test_stream_is_opt_in():
    assert STREAM_OUT_KINDS == DEVICE_OUT_KINDS + ("rw",)
    eng = APMEngine(rw_cfg(), keep_text=True)   # the key in the config alone does not start it
    assert not (eng.ecfg["outputs"] >> STREAM_OUT_KINDS.index("rw")) & 1
    assert eng.eng.recents() == []
    with pytest.raises(ValueError):
        APMEngine(small_cfg(), outputs=("st", "rw"))
    bad = small_cfg()
    bad["gpu"]["recentWindows"] = {"buckets": [6, 1], "percentiles": [50]}
    with pytest.raises(ValueError):
        APMEngine(bad, outputs=("st", "rw"))
    # the native constructor checks the lists it is handed as well
    N = _native.load()
    ecfg = engine_config(rw_cfg(), outputs=("st", "rw"))
    w = ecfg["window"]
    for lst in ([], [0], [6, 6], [6, 1], [1, 2, 3, 4, 5], [w + 1], [1, w + 1]):
        with pytest.raises(ValueError):
            N.Engine(dict(ecfg, rw_buckets=lst))
    for lst in ([], [50000, 50000], [0], [100001], list(range(1, 10))):
        with pytest.raises(ValueError):
            N.Engine(dict(ecfg, rw_pcts=lst))
    assert N.recent_group_max() == 512 and N.recent_group_win() == 32


def test_full_pipeline_matches_oracle_and_changes_nothing_else():
    bl = synth3(seed=1)
    C = rw_cfg()
    kinds = KINDS + ("rw",)
    eng, on = run(C, bl, kinds, kinds=kinds)
    _e, off = run(small_cfg(), bl, KINDS, kinds=KINDS + ("rw",))
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    assert len(P.rw) > 200 and {r.split("|")[4] for r in P.rw} == {"1", "6"}
    assert any(r.split("|")[5] == "0" for r in P.rw)   # a span without a sample inside a window with some
    assert on["rw"] == P.rw
    assert off["rw"] == [] and _e.eng.recents() == []
    for k in ("st", "fs", "al", "audit_db", "transactions"):
        assert on[k] == off[k], k
    assert collections.Counter(on["db"]) == collections.Counter(off["db"]) and len(on["db"]) > 100
    assert on["st"] == P.stats
    # rows stand in st order with the st rows' timestamps, one per span
    st_keys = [tuple(l.split("|")[1:4]) for l in on["st"]]
    rw_keys = [tuple(r.split("|")[1:4]) for r in on["rw"]]
    assert rw_keys[0::2] == rw_keys[1::2] and [r.split("|")[4] for r in on["rw"][:2]] == ["1", "6"]
    have = set(rw_keys)
    assert rw_keys[0::2] == [k for k in st_keys if k in have]
    # the read-back holds the last rollover's records, per series id
    last_ts = on["rw"][-1].split("|")[1]
    last = [r.split("|") for r in on["rw"] if r.split("|")[1] == last_ts]
    dev = [d for d in eng.eng.recents() if d is not None]
    assert len(dev) * 2 == len(last)
    got = sorted((m, nan, total, tuple(R.half(v) for v in s2)) for spans in dev for (m, nan, total, s2) in spans)
    want = sorted((int(f[5]), int(f[6]), int(f[7]), tuple(p.split(":")[1] for p in f[8].split(",") if p)) for f in last)
    assert got == want


def test_off_is_byte_identical_to_never_naming_it():
    """The key set and the stream off: every other stream is what a config without the key gives."""
    bl = synth3(seed=2, duration=150)
    kinds = KINDS + EXTRA
    C = rw_cfg(extra=True)
    _e, named = run(C, bl, kinds, kinds=kinds + ("rw",))
    C0 = copy.deepcopy(C)
    del C0["gpu"]["recentWindows"]
    _e, never = run(C0, bl, kinds, kinds=kinds)
    assert named["rw"] == []
    for k in kinds:
        if k == "db":
            assert collections.Counter(named[k]) == collections.Counter(never[k])
        else:
            assert named[k] == never[k], k
    assert min(len(never[k]) for k in EXTRA) > 20


def test_with_every_window_stream_on_each_equals_its_solo_run():
    bl = synth3(seed=5, duration=150)
    C = rw_cfg(extra=True)
    kinds = KINDS + EXTRA + ("rw",)
    _e, on = run(C, bl, kinds, kinds=kinds)
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    assert min(len(P.lh), len(P.wp), len(P.sl), len(P.tk), len(P.sv), len(P.rw)) > 50
    for k in EXTRA + ("rw",):
        _s, solo = run(C, bl, ("st", k), kinds=(k,))
        assert on[k] == solo[k] == getattr(P, k), k
    assert on["st"] == P.stats


def test_checkpoint_resumes_the_stream(tmp_path):
    bl = synth3(seed=6, duration=200)
    C = rw_cfg()
    kinds = KINDS + ("rw",)
    _e, full = run(C, bl, kinds, kinds=kinds)
    cut = len(bl) // 2
    eng, head = run(C, bl[:cut], kinds, kinds=kinds)
    ck = str(tmp_path / "engine.ckpt")
    assert eng.save_state(ck) > 0
    del eng
    eng2 = APMEngine(C, outputs=kinds)
    eng2.load_state(ck)
    _e, tail = run(C, bl[cut:], kinds, eng=eng2, kinds=kinds)
    assert len(tail["rw"]) > 20 and len(head["rw"]) > 20
    assert head["rw"] + tail["rw"] == full["rw"]
    assert head["st"] + tail["st"] == full["st"]


def test_a_reload_that_shortens_the_window_clips_the_spans():
    """windowSizeInIntervals 30 -> 3 by a hot reload (4 window buckets): the reload is accepted and
    names nothing that needs a restart; from then on the spans 6 and 9 read the whole window -- the
    second of them the entries the first one sorted already -- and still print the configured k.
    Rows against the oracle applying the same reload between the same batches, and the clipped
    spans against the series' wp row."""
    bl = synth3(seed=9, duration=200)
    C0 = small_cfg()
    C0["gpu"]["windowPercentiles"] = [50, 95, 99]
    C0["gpu"]["recentWindows"] = {"buckets": [1, 6, 9], "percentiles": [50, 95, 99]}
    C1 = copy.deepcopy(C0)
    C1["streamCalcStats"]["windowSizeInIntervals"] = 3
    cut = len(bl) // 2
    P = PipelineOracle(copy.deepcopy(C0), UTC)
    P.run_batches(bl[:cut])
    n_before = len(P.rw)
    P.reload(copy.deepcopy(C1))
    P.run_batches(bl[cut:])
    kinds = ("st", "wp", "rw")
    eng = APMEngine(copy.deepcopy(C0), outputs=kinds)
    out = collections.defaultdict(list)
    for i, (now, chunks) in enumerate(bl):
        if i == cut:
            assert eng.reload(copy.deepcopy(C1), gen=1) == []
        eng.process_lines(chunks, now)
        for k in kinds:
            out[k] += eng.take(k)
    info = eng.eng.reconfig_info()
    assert info["applied"] == 1 and info["window_changes"] == 1
    assert out["st"] == P.stats and out["wp"] == P.wp
    assert out["rw"] == P.rw and n_before > 100 and len(P.rw) - n_before > 300
    after = [r.split("|") for r in out["rw"][n_before:]]
    assert {f[4] for f in after} == {"1", "6", "9"}            # the configured values, not the clipped one
    wp = {tuple(f[1:4]): f for f in (r.split("|") for r in out["wp"])}
    whole = 0
    for f in after[-180:]:                                      # (the last rollovers: the window shrank before them)
        w = wp.get(tuple(f[1:4]))
        if f[4] != "1" and w is not None:
            assert [f[5], f[6], f[8]] == w[4:7], (f, w)
            whole += 1
    assert whole >= 60
    assert any(f[5] != g[5] for f, g in zip(after[0::3], after[1::3]))   # span 1 stays shorter than the window
    # the read-back after the reload: the two clipped spans hold the same record
    dev = [d for d in eng.eng.recents() if d is not None]
    assert dev and all(d[1] == d[2] for d in dev)


def test_service_routes_the_rows_to_the_queue(tmp_path):
    b = Broker(port=0).start()
    try:
        C, lines, mapping, sc = make_env(tmp_path, mode="amqp", duration=200)
        gpu_cfg(C)
        C["amqpConnectionString"] = b.url
        C["gpu"]["recentWindows"] = copy.deepcopy(KEY)
        C["gpu"]["recentQueue"] = "recent_rows"
        svc = IngestService(C, engine="native", files=sorted(mapping.values()), rank=0, world=1, server_of_path=srv_of)
        assert svc.outputs[-1] == "rw"
        P = PipelineOracle(copy.deepcopy(C), UTC, server_fn=srv_of)
        feed_in_steps(svc, lines, mapping, sc, P)
        svc.shutdown()
        st = b.stats()
        assert len(P.rw) > 20 and 20 < st["recent_rows"]["messages"] <= len(P.rw)
        assert st["db_insert"]["messages"] > 0 and "recent_window" not in st
    finally:
        b.stop()


def test_service_spools_the_table(tmp_path):
    files = {}
    for engine in ("native", "cpu-oracle"):
        d = tmp_path / engine
        d.mkdir()
        C, lines, mapping, sc = make_env(d, duration=200)
        gpu_cfg(C)
        C["gpu"]["recentWindows"] = copy.deepcopy(KEY)
        svc = IngestService(C, engine=engine, files=sorted(mapping.values()), rank=0, world=1, server_of_path=srv_of)
        assert "rw" in svc.outputs
        feed_in_steps(svc, lines, mapping, sc)
        svc.shutdown()
        files[engine] = {f: open(d / "copy" / f, "rb").read() for f in sorted(os.listdir(d / "copy"))}
    nat, cpu = files["native"], files["cpu-oracle"]
    assert nat["apm_recent_window.copy"] == cpu["apm_recent_window.copy"]
    assert nat["apm_recent_window.copy"].count(b"\n") > 20
    assert nat["apm_recent_window.columns"] == cpu["apm_recent_window.columns"]


# ---- the text slot (engine.h TextStream), as tests/test_text_streams_gpu.py has it for lh / wp / sl / sv

def test_slot_reuse_and_regrow():
    """Several rollovers, so both slots are taken twice while their output-lane tasks may be
    outstanding; a much longer service name first appears after both slots were used, so each
    slot's device output is regrown; about 70 series, two lanes each, cross the write block; one
    series holds more samples in its spans than the group pass takes."""
    bl = build_batches()
    C = streams_cfg()
    C["gpu"]["recentWindows"] = {"buckets": [1, 6], "percentiles": [50, 99.9]}
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    kinds = KINDS + ("lh", "wp", "sl", "sv", "rw")
    _e, out = run(C, bl, kinds, kinds=kinds)
    assert out["st"] == P.stats
    rows = [r.split("|") for r in P.rw]
    stamps = sorted({int(f[1]) for f in rows})
    assert len(stamps) >= 4
    long_stamps = sorted({int(f[1]) for f in rows if len(f[3]) >= 280})
    assert len(long_stamps) >= 2 and stamps.index(long_stamps[0]) >= 2
    assert max(sum(1 for f in rows if int(f[1]) == t) for t in stamps) > 128
    counts = [int(f[5]) for f in rows if f[3] == HEAVY_ROW]
    assert counts and max(counts) > _native.load(build_if_missing=False).recent_group_max()
    assert min(int(f[5]) for f in rows) <= 8
    assert out["rw"] == P.rw
    for k in ("lh", "wp", "sl", "sv"):
        assert out[k] == getattr(P, k), k


def test_resources_return_after_the_engine():
    COUNTS = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes", "events", "streams")
    gc.collect()
    N = _native.load()
    before = dict(N.live_resources())
    bl = synth3(seed=3, duration=100)
    kinds = KINDS + ("rw",)
    eng, out = run(rw_cfg(), bl, kinds, kinds=kinds)
    assert len(out["rw"]) > 10
    during = dict(N.live_resources())
    assert during["device_bytes"] - before["device_bytes"] == eng.eng.device_bytes()
    plain, _o = run(small_cfg(), bl, KINDS)
    assert eng.eng.device_bytes() > plain.eng.device_bytes()   # the stream's memory is accounted for
    keyed, _o2 = run(rw_cfg(), bl, KINDS)                       # the key set, the stream off: nothing allocated
    assert keyed.eng.device_bytes() == plain.eng.device_bytes()
    del eng, out, plain, _o, keyed, _o2
    gc.collect()
    after = dict(N.live_resources())
    assert {k: after[k] for k in COUNTS} == {k: before[k] for k in COUNTS}

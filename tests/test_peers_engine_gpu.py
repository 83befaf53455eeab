"""The po stream through the whole engine: parse -> device join -> K7 -> K8 -> K23, against
PipelineOracle over several rollovers, record for record, with one server whose calls of one
service are slowed mid-run (the synthetic load's planted anomaly: the generator stretches that
server's calls of the service thirtyfold from the cut on); the other streams unchanged by it;
nothing allocated or launched while it is off, with sv on and off; a checkpoint taken mid-run; two
ranks, each against an oracle over its own servers.  (Shapes of tests/test_traffic_engine_gpu.py.)"""
import collections
import copy
import gc
import threading

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

from apmbackend_amd import _native  # noqa: E402
from apmbackend_amd.models.oracle import PipelineOracle  # noqa: E402
from apmbackend_amd.models.pipeline import EVERY_OUT_KINDS, WHOLE_OUT_KINDS, APMEngine, engine_config  # noqa: E402
from apmbackend_amd.parallel.dist import shard_servers  # noqa: E402
from apmbackend_amd.parallel.fleet import FleetBaseline  # noqa: E402
from apmbackend_amd.utils.records import entry_from_csv  # noqa: E402
from apmbackend_amd.utils.synth import Anomaly, Generator, SynthConfig, batches, with_watermarks  # noqa: E402

from test_hist_engine_gpu import KINDS, START, UTC, run, server_of, small_cfg  # noqa: E402

# a window of 9 buckets that the run fills; six servers a service, so a group reaches minPeers
KEY = {"percentile": 95, "default": {"minValue": 20}, "services": {"S:getSvc0003": None},
       "high": 3, "low": 0.1, "z": 3, "minDelta": 10, "minPeers": 5, "minSamples": 10}
SLOW_SERVER, SLOW = "jvm02", "getSvc0001"


def po_cfg(key=KEY, sv=False):
    C = small_cfg()
    C["streamCalcStats"]["windowSizeInIntervals"] = 8
    C["gpu"]["peerOutliers"] = copy.deepcopy(key)
    if sv:
        C["gpu"]["serviceWindow"] = {"percentiles": [50, 95]}
    return C


def plain_cfg():
    C = small_cfg()
    C["streamCalcStats"]["windowSizeInIntervals"] = 8
    return C


def load(seed=1, duration=300, servers=6, frac=0.4, slow_server=SLOW_SERVER):
    """(lines, batches, cut): from frac * duration on, slow_server's calls of SLOW take thirty times as long."""
    cut = START + int(duration * 1000 * frac)
    an = [Anomaly(slow_server, SLOW, cut, START + int(duration * 1000) + 1, 30.0)]
    cfg = SynthConfig(servers=servers, duration_s=duration, tx_per_sec_per_server=3, seed=seed,
                      ejb_services=4, provider_services=3, anomalies=an)
    lines = Generator(cfg).generate()
    return lines, with_watermarks(batches(lines, cfg.start_ms, 5.0), UTC), cut


def test_stream_is_opt_in():
    assert WHOLE_OUT_KINDS == EVERY_OUT_KINDS + ("po",)
    eng = APMEngine(po_cfg(), keep_text=True)   # the key in the config alone does not start it
    assert not (eng.ecfg["outputs"] >> WHOLE_OUT_KINDS.index("po")) & 1
    assert eng.eng.peers() == [] and eng.metrics()["po_rows"] == 0
    with pytest.raises(ValueError):
        APMEngine(small_cfg(), outputs=("st", "po"))
    bad = po_cfg()
    bad["gpu"]["peerOutliers"]["minPeers"] = 2
    with pytest.raises(ValueError):
        APMEngine(bad, outputs=("st", "po"))
    # the native constructor checks what it is handed as well
    N = _native.load()
    ecfg = engine_config(po_cfg(), outputs=("st", "po"))
    for over in ({"po_classes": []}, {"po_classes": [[]]}, {"po_classes": [[], [5, 1]]}, {"po_classes": [[], [0]]},
                 {"po_classes": [[], [2 ** 31]]}, {"po_classes": [[5]]}, {"po_default": 7}, {"po_services": {"x": 9}},
                 {"po_pct": 0}, {"po_pct": 100001}, {"po_high": 1000}, {"po_high": 1000001}, {"po_low": 1000},
                 {"po_low": -1}, {"po_high": 0, "po_low": 0}, {"po_z": 100001}, {"po_z": -1}, {"po_min_delta": -1},
                 {"po_min_peers": 2}, {"po_min_samples": 0}):
        with pytest.raises(ValueError):
            N.Engine(dict(ecfg, **over))


def test_full_pipeline_matches_oracle_and_changes_nothing_else():
    _lines, bl, cut = load(seed=1, duration=300)
    C = po_cfg()
    kinds = KINDS + ("po",)
    eng, on = run(C, bl, kinds, kinds=kinds)
    off_eng, off = run(plain_cfg(), bl, KINDS, kinds=KINDS + ("po",))
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    rows = [r.split("|") for r in P.po]
    slow = [f for f in rows if f[3] == "S:" + SLOW]
    # the slowed server prints H rows while it lasts, none before, and no other server of the service prints
    assert len(slow) > 5 and all(f[2] == SLOW_SERVER and f[9] == "H" for f in slow)
    assert all(int(f[1]) >= cut - 10_000 for f in slow)
    assert all(int(f[6]) == 6 and 2 * int(f[5].split(":")[1]) >= 3 * int(f[7]) for f in slow)
    assert not any(f[3] == "S:getSvc0003" for f in rows)
    assert len(P.po) < len(P.stats) // 4
    # record for record
    assert len(on["po"]) == len(P.po)
    for got, want in zip(on["po"], P.po):
        assert got == want and entry_from_csv(got) == entry_from_csv(want)
    assert off["po"] == [] and off_eng.eng.peers() == [] and off_eng.metrics()["po_rows"] == 0
    assert eng.metrics()["po_rows"] == len(P.po)
    # with the stream on, every other stream's bytes are those of a run with it off
    for k in ("st", "fs", "al", "audit_db", "transactions"):
        assert on[k] == off[k], k
    assert collections.Counter(on["db"]) == collections.Counter(off["db"]) and len(on["db"]) > 100
    assert on["st"] == P.stats
    # rows stand in st order with the st rows' timestamps
    st_keys = [tuple(l.split("|")[1:4]) for l in on["st"]]
    po_keys = [tuple(r.split("|")[1:4]) for r in on["po"]]
    have = set(po_keys)
    assert len(have) == len(po_keys) and po_keys == [k for k in st_keys if k in have]
    # the read-back holds the last rollover's records per series id, for series that did not fire too
    last_ts = on["st"][-1].split("|")[1]
    last = sorted(int(f[5].split(":")[1]) for f in (r.split("|") for r in on["po"]) if f[1] == last_ts)
    dev = eng.eng.peers()
    assert any(d is None for d in dev)                       # S:getSvc0003: class 0
    recs = [d for d in dev if d is not None]
    assert sorted(d[1] for d in recs if d[5] != "N") == last and last
    assert any(d[5] == "N" for d in recs) and all(d[0] >= KEY["minSamples"] for d in recs)


@pytest.mark.parametrize("sv", [False, True])
def test_key_set_and_stream_off_allocates_and_launches_nothing(sv):
    """The key set and the stream off: the engine holds exactly the device blocks, bytes, pinned
    blocks, events and streams of an engine whose config never names the key (with the sv stream,
    whose service lists po shares, on or off), keeps no record and prints what that engine prints."""
    _lines, bl, _cut = load(seed=3, duration=150)
    gc.collect()
    N = _native.load()
    COUNTS = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes", "events", "streams")
    outs = KINDS + (("sv",) if sv else ())
    base = plain_cfg()
    if sv:
        base["gpu"]["serviceWindow"] = {"percentiles": [50, 95]}
    before = dict(N.live_resources())
    plain, out0 = run(base, bl, outs, kinds=outs)
    one = {k: N.live_resources()[k] - before[k] for k in COUNTS}
    keyed, out1 = run(po_cfg(sv=sv), bl, outs, kinds=outs + ("po",))
    two = {k: N.live_resources()[k] - before[k] for k in COUNTS}
    assert two == {k: 2 * one[k] for k in COUNTS}
    assert keyed.eng.device_bytes() == plain.eng.device_bytes()
    assert out1["po"] == [] and keyed.eng.peers() == [] and keyed.metrics()["po_rows"] == 0
    for k in outs:
        if k == "db":
            assert collections.Counter(out0[k]) == collections.Counter(out1[k])
        else:
            assert out0[k] == out1[k], k
    on, out2 = run(po_cfg(sv=sv), bl, outs + ("po",), kinds=outs + ("po",))
    assert len(out2["po"]) > 2 and on.eng.device_bytes() > plain.eng.device_bytes()   # the stream's memory is accounted for
    if sv:
        assert out2["sv"] == out0["sv"] and len(out0["sv"]) > 5
    del on, out2, plain, keyed, out0, out1
    gc.collect()
    after = dict(N.live_resources())
    assert {k: after[k] for k in COUNTS} == {k: before[k] for k in COUNTS}


def test_checkpoint_resumes_the_stream(tmp_path):
    _lines, bl, _cut = load(seed=6, duration=300, frac=0.2)   # (rows on both sides of the checkpoint)
    C = po_cfg()
    kinds = KINDS + ("po",)
    _e, full = run(C, bl, kinds, kinds=kinds)
    cut = len(bl) // 2
    eng, head = run(C, bl[:cut], kinds, kinds=kinds)
    ck = str(tmp_path / "engine.ckpt")
    assert eng.save_state(ck) > 0
    del eng
    eng2 = APMEngine(C, outputs=kinds)
    eng2.load_state(ck)
    _e, tail = run(C, bl[cut:], kinds, eng=eng2, kinds=kinds)
    assert len(tail["po"]) > 5 and len(head["po"]) > 2
    assert head["po"] + tail["po"] == full["po"]
    assert head["st"] + tail["st"] == full["st"]


def run_node(world, bl, servers):
    """`world` engines with the po stream on, one host thread each, joined by an in-process
    collective group with lock-step clocks (the harness of tests/test_hist_engine_gpu.py)."""
    group = _native.load().LocalCollGroup(world, 120000.0)
    shards = shard_servers(servers, world)
    engs, outs, errs = [], [], []
    for r in range(world):
        eng = APMEngine(po_cfg(), keep_text=True, outputs=("po",))
        for _now, chunks in bl:
            for fp, _ls in chunks:
                if server_of(fp) in shards[r]:
                    eng.add_file(fp)
        engs.append(eng)
        outs.append(collections.defaultdict(list))

    def rank_main(r):
        try:
            fleet = FleetBaseline(engs[r], world, r, max_services=64, local_group=group, servers=servers)
            for now, chunks in bl:
                engs[r].process_lines([(fp, ls) for fp, ls in chunks if server_of(fp) in shards[r]], now)
                for k in ("st", "po"):
                    outs[r][k] += engs[r].take(k)
            fleet.drain_alerts()
            for k in ("st", "po"):
                outs[r][k] += engs[r].take(k)
        except Exception as e:  # pragma: no cover - reported below
            errs.append((r, repr(e)))

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    assert not errs, errs
    assert all(not t.is_alive() for t in th)
    return engs, outs, shards


def test_two_ranks_judge_their_own_servers():
    """World 2, servers sharded: a rank sees only its own servers, so a service's peers are the
    series of that rank.  Each rank's rows are those of an oracle fed that rank's servers alone;
    together they are not the one-rank run's rows (other peers, other medians)."""
    lines, bl, _cut = load(seed=2, duration=200, servers=12, slow_server="jvm03")
    servers = sorted({server_of(fp) for fp in lines})
    P = PipelineOracle(po_cfg(), UTC)
    P.run_batches(bl)
    _e1, one, _s = run_node(1, bl, servers)
    _e2, two, shards = run_node(2, bl, servers)
    assert one[0]["po"] == P.po and len(P.po) > 5
    for r in range(2):
        assert len(shards[r]) == 6
        Pr = PipelineOracle(po_cfg(), UTC)
        Pr.run_batches([(now, [(fp, ls) for fp, ls in chunks if server_of(fp) in shards[r]]) for now, chunks in bl])
        assert two[r]["po"] == Pr.po
        assert {l.split("|")[2] for l in two[r]["po"]} <= set(shards[r])
        assert all(l.split("|")[6] == "6" for l in two[r]["po"])
    assert sum(len(two[r]["po"]) for r in range(2)) > 5
    assert collections.Counter(two[0]["po"] + two[1]["po"]) != collections.Counter(one[0]["po"])

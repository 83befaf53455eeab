"""The sb stream through the whole engine: parse -> device join -> K7 -> K8 -> K21, against
PipelineOracle over several rollovers, record for record; the other streams unchanged by it; nothing
allocated or launched while it is off; a checkpoint taken mid-run; two ranks against one.  (Shapes
of tests/test_recent_engine_gpu.py and tests/test_hist_engine_gpu.py.)"""
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
from apmbackend_amd.models.pipeline import FULL_OUT_KINDS, STREAM_OUT_KINDS, APMEngine, engine_config  # noqa: E402
from apmbackend_amd.parallel.dist import shard_servers  # noqa: E402
from apmbackend_amd.parallel.fleet import FleetBaseline  # noqa: E402
from apmbackend_amd.utils.records import entry_from_csv  # noqa: E402

from test_hist_engine_gpu import KINDS, UTC, run, server_of, small_cfg, synth_batches  # noqa: E402

# on the synthetic load about a third of the st rows breach, some by the second rule only
KEY = {"default": {"threshold": 300, "target": 95},
       "services": {"S:getSvc0002": {"threshold": 150, "target": 99}, "S:getSvc0003": None},
       "rules": [{"short": 1, "factor": 2}, {"short": 6, "factor": 1}],
       "minSamples": 5}


def sb_cfg(key=KEY):
    C = small_cfg()
    C["gpu"]["sloBurn"] = copy.deepcopy(key)
    return C


def test_stream_is_opt_in():
    assert FULL_OUT_KINDS == STREAM_OUT_KINDS + ("sb",)
    eng = APMEngine(sb_cfg(), keep_text=True)   # the key in the config alone does not start it
    assert not (eng.ecfg["outputs"] >> FULL_OUT_KINDS.index("sb")) & 1
    assert eng.eng.burns() == [] and eng.metrics()["sb_rows"] == 0
    with pytest.raises(ValueError):
        APMEngine(small_cfg(), outputs=("st", "sb"))
    bad = sb_cfg()
    bad["gpu"]["sloBurn"]["rules"] = [{"short": 6, "factor": 1}, {"short": 1, "factor": 1}]
    with pytest.raises(ValueError):
        APMEngine(bad, outputs=("st", "sb"))
    wide = sb_cfg()
    wide["gpu"]["sloBurn"]["rules"] = [{"short": 31, "factor": 1}]   # windowSizeInIntervals is 30
    with pytest.raises(ValueError):
        APMEngine(wide, outputs=("st", "sb"))
    # the native constructor checks the tables it is handed as well
    N = _native.load()
    ecfg = engine_config(sb_cfg(), outputs=("st", "sb"))
    w = ecfg["window"]
    for over in ({"sb_short": [], "sb_factor": []}, {"sb_short": [w + 1], "sb_factor": [1000]},
                 {"sb_classes": []}, {"sb_classes": [[]]}, {"sb_classes": [[], [5]]}, {"sb_classes": [[], [5, 0]]},
                 {"sb_classes": [[], [5, 100000]]}, {"sb_classes": [[], [-1, 99000]]}, {"sb_classes": [[5, 99000]]},
                 {"sb_default": 7}, {"sb_services": {"x": 9}}):
        with pytest.raises(ValueError):
            N.Engine(dict(ecfg, **over))
    for over in ({"sb_short": [6, 1], "sb_factor": [1, 1]}, {"sb_short": [1], "sb_factor": [0]},
                 {"sb_short": [1], "sb_factor": [1000001]}, {"sb_short": [1, 2], "sb_factor": [1]},
                 {"sb_short": [1, 2, 3, 4, 5], "sb_factor": [1] * 5}, {"sb_min_samples": 0}):
        with pytest.raises(ValueError):
            N.Engine(dict(ecfg, **over))
    assert N.burn_group_max() == N.slo_group_max() == 4096


def test_full_pipeline_matches_oracle_and_changes_nothing_else():
    _lines, bl = synth_batches(seed=1, duration=300)
    C = sb_cfg()
    kinds = KINDS + ("sb",)
    eng, on = run(C, bl, kinds, kinds=kinds)
    off_eng, off = run(small_cfg(), bl, KINDS, kinds=KINDS + ("sb",))
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    assert 50 < len(P.sb) < len(P.stats) - 50
    fired = collections.Counter(tuple(g.split(":")[4] for g in r.split("|")[9].split(",")) for r in P.sb)
    assert fired[("1", "1")] > 10 and fired[("0", "1")] > 10
    assert {r.split("|")[3] for r in P.sb} >= {"S:getSvc0002"} and not any(r.split("|")[3] == "S:getSvc0003" for r in P.sb)
    # record for record
    assert len(on["sb"]) == len(P.sb)
    for got, want in zip(on["sb"], P.sb):
        assert got == want and entry_from_csv(got) == entry_from_csv(want)
    assert off["sb"] == [] and off_eng.eng.burns() == [] and off_eng.metrics()["sb_rows"] == 0
    assert eng.metrics()["sb_rows"] == len(P.sb)
    # with the stream on, every other stream's bytes are those of a run with it off
    for k in ("st", "fs", "al", "audit_db", "transactions"):
        assert on[k] == off[k], k
    assert collections.Counter(on["db"]) == collections.Counter(off["db"]) and len(on["db"]) > 100
    assert on["st"] == P.stats
    # rows stand in st order with the st rows' timestamps
    st_keys = [tuple(l.split("|")[1:4]) for l in on["st"]]
    sb_keys = [tuple(r.split("|")[1:4]) for r in on["sb"]]
    have = set(sb_keys)
    assert len(have) == len(sb_keys) and sb_keys == [k for k in st_keys if k in have]
    # the read-back holds the last rollover's records per series id, for series that did not fire too
    last_ts = on["st"][-1].split("|")[1]
    last = sorted((int(f[6]), int(f[7]), int(f[8])) for f in (r.split("|") for r in on["sb"]) if f[1] == last_ts)
    dev = eng.eng.burns()
    assert any(d is None for d in dev)                       # S:getSvc0003: class 0
    recs = [d for d in dev if d is not None]
    assert sorted((m, bad, nan) for m, bad, nan, _r, mask in recs if mask) == last
    assert any(mask == 0 for *_x, mask in recs) and all(len(r) == 2 for _m, _b, _n, r, _k in recs)


def test_key_set_and_stream_off_allocates_and_launches_nothing():
    """The key set and the stream off: the engine holds exactly the device blocks, bytes, pinned
    blocks, events and streams of an engine whose config never names the key, keeps no record
    (burns() is empty: no value pass ran) and prints what that engine prints."""
    _lines, bl = synth_batches(seed=3, duration=100)
    gc.collect()
    N = _native.load()
    COUNTS = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes", "events", "streams")
    before = dict(N.live_resources())
    plain, out0 = run(small_cfg(), bl, KINDS)
    one = {k: N.live_resources()[k] - before[k] for k in COUNTS}
    keyed, out1 = run(sb_cfg(), bl, KINDS, kinds=KINDS + ("sb",))
    two = {k: N.live_resources()[k] - before[k] for k in COUNTS}
    assert two == {k: 2 * one[k] for k in COUNTS}
    assert keyed.eng.device_bytes() == plain.eng.device_bytes()
    assert out1["sb"] == [] and keyed.eng.burns() == [] and keyed.metrics()["sb_rows"] == 0
    for k in KINDS:
        if k == "db":
            assert collections.Counter(out0[k]) == collections.Counter(out1[k])
        else:
            assert out0[k] == out1[k], k
    on, out2 = run(sb_cfg(), bl, KINDS + ("sb",), kinds=KINDS + ("sb",))
    assert len(out2["sb"]) > 5 and on.eng.device_bytes() > plain.eng.device_bytes()   # the stream's memory is accounted for
    del on, out2, plain, keyed, out0, out1
    gc.collect()
    after = dict(N.live_resources())
    assert {k: after[k] for k in COUNTS} == {k: before[k] for k in COUNTS}


def test_checkpoint_resumes_the_stream(tmp_path):
    _lines, bl = synth_batches(seed=6, duration=300)
    C = sb_cfg()
    kinds = KINDS + ("sb",)
    _e, full = run(C, bl, kinds, kinds=kinds)
    cut = len(bl) // 2
    eng, head = run(C, bl[:cut], kinds, kinds=kinds)
    ck = str(tmp_path / "engine.ckpt")
    assert eng.save_state(ck) > 0
    del eng
    eng2 = APMEngine(C, outputs=kinds)
    eng2.load_state(ck)
    _e, tail = run(C, bl[cut:], kinds, eng=eng2, kinds=kinds)
    assert len(tail["sb"]) > 20 and len(head["sb"]) > 5
    assert head["sb"] + tail["sb"] == full["sb"]
    assert head["st"] + tail["st"] == full["st"]


def run_node(world, bl, servers):
    """`world` engines with the sb stream on, one host thread each, joined by an in-process
    collective group with lock-step clocks (the harness of tests/test_hist_engine_gpu.py)."""
    group = _native.load().LocalCollGroup(world, 120000.0)
    shards = shard_servers(servers, world)
    engs, outs, errs = [], [], []
    for r in range(world):
        eng = APMEngine(sb_cfg(), keep_text=True, outputs=("sb",))
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
                for k in ("st", "sb"):
                    outs[r][k] += engs[r].take(k)
            fleet.drain_alerts()
            for k in ("st", "sb"):
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


def test_two_ranks_give_the_union_of_one_ranks_rows():
    """World 2, servers sharded: a server's series never span ranks, so every rank's rows are
    complete and their union is the 1-rank run's (and the oracle's)."""
    lines, bl = synth_batches(seed=2, duration=200, servers=4)
    servers = sorted({server_of(fp) for fp in lines})
    P = PipelineOracle(sb_cfg(), UTC)
    P.run_batches(bl)
    _e1, one, _s = run_node(1, bl, servers)
    _e2, two, shards = run_node(2, bl, servers)
    assert one[0]["sb"] == P.sb and len(P.sb) > 50
    for r in range(2):
        assert {l.split("|")[2] for l in two[r]["sb"]} <= set(shards[r]) and len(two[r]["sb"]) > 10
        stamps = [int(l.split("|")[1]) for l in two[r]["sb"]]
        assert stamps == sorted(stamps)
    assert collections.Counter(two[0]["sb"] + two[1]["sb"]) == collections.Counter(one[0]["sb"])

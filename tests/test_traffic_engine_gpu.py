"""The tf stream through the whole engine: parse -> device join -> K7 -> K8 -> K22, against
PipelineOracle over several rollovers, record for record, with a service that stops mid-run and
one that floods (ten times its calls from a second synthetic load); the other streams unchanged
by it; nothing allocated or launched while it is off; a checkpoint taken mid-run; two ranks
against one; a reload past the window bound refused.  (Shapes of tests/test_burn_engine_gpu.py.)"""
import collections
import copy
import gc
import re
import threading

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

from apmbackend_amd import _native  # noqa: E402
from apmbackend_amd.models.oracle import PipelineOracle  # noqa: E402
from apmbackend_amd.models.pipeline import EVERY_OUT_KINDS, FULL_OUT_KINDS, APMEngine, engine_config  # noqa: E402
from apmbackend_amd.parallel.dist import shard_servers  # noqa: E402
from apmbackend_amd.parallel.fleet import FleetBaseline  # noqa: E402
from apmbackend_amd.utils.records import entry_from_csv  # noqa: E402

from apmbackend_amd.utils.synth import Generator, SynthConfig, batches, with_watermarks  # noqa: E402

from test_hist_engine_gpu import KINDS, START, UTC, run, server_of, small_cfg  # noqa: E402

# a window of 9 buckets, so that the buckets of a run fill it: 8 and 6 baseline buckets.  At about
# 7 calls per bucket and series the load's own jitter seldom reaches these ratios.
KEY = {"default": {"minRate": 3},
       "services": {"S:getSvc0003": None},
       "rules": [{"short": 1, "drop": 0.2, "surge": 3, "z": 3}, {"short": 3, "drop": 0.5, "surge": 2.5, "z": 3}],
       "minBuckets": 4}
STOPS = "getSvc0002"
FLOODS = "getSvc0000"
LOG_ID = re.compile(r"JVM\d\d-\d{8}")


def tf_cfg(key=KEY, base=None):
    C = base or small_cfg()
    C["streamCalcStats"]["windowSizeInIntervals"] = 8
    C["gpu"]["trafficWatch"] = copy.deepcopy(key)
    return C


def plain_cfg():
    C = small_cfg()
    C["streamCalcStats"]["windowSizeInIntervals"] = 8
    return C


def synth_lines(seed, duration, servers, rate):
    cfg = SynthConfig(servers=servers, duration_s=duration, tx_per_sec_per_server=rate, seed=seed,
                      ejb_services=4, provider_services=3)
    return Generator(cfg).generate(), cfg


def flood_lines(extra, name, from_ms):
    """From another synthetic load, every log line of the calls of service `name` that start at
    from_ms or later, under log ids of their own: {file: [(ts, seq, text)]}."""
    by_dir = collections.defaultdict(dict)
    for fp in extra:
        by_dir[fp.rsplit("/", 1)[0]][fp.rsplit("/", 1)[1]] = fp
    out = {}
    for files in by_dir.values():
        ids = set()
        for ts, _seq, text in extra[files["server.log"]]:
            m = LOG_ID.search(text)
            if m and ts >= from_ms and text.endswith("started for bean Delegation method: " + name):
                ids.add(m.group(0))
        for fn, fp in files.items():
            cur, keep = None, []
            for ts, seq, text in extra[fp]:
                m = LOG_ID.search(text)
                if m:
                    cur = m.group(0)
                elif fn != "soap_io.log":    # (a SOAP body's lines follow their header; other lines carry their id)
                    cur = None
                if cur in ids:
                    keep.append((ts, seq + 10 ** 9, text.replace(cur, cur[:6] + "9" + cur[7:])))
            out[fp] = keep
    return out


def load(seed=1, duration=300, servers=2, frac=0.6):
    """(lines, batches) of the synthetic load at 3 calls a second and server in which, from
    frac * duration on, STOPS receives no call any more (its lines are removed) and FLOODS
    receives those of a second load at ten times the rate as well."""
    lines, cfg = synth_lines(seed, duration, servers, 3)
    cut = START + int(duration * 1000 * frac)
    extra, _cfg = synth_lines(seed + 70, duration, servers, 30)
    more = flood_lines(extra, FLOODS, cut)
    merged = {fp: sorted([l for l in ls if not (l[0] >= cut and STOPS in l[2])] + more.get(fp, []))
              for fp, ls in lines.items()}
    return merged, with_watermarks(batches(merged, cfg.start_ms, 5.0), UTC)


def test_stream_is_opt_in():
    assert EVERY_OUT_KINDS == FULL_OUT_KINDS + ("tf",)
    eng = APMEngine(tf_cfg(), keep_text=True)   # the key in the config alone does not start it
    assert not (eng.ecfg["outputs"] >> EVERY_OUT_KINDS.index("tf")) & 1
    assert eng.eng.traffic() == [] and eng.metrics()["tf_rows"] == 0
    with pytest.raises(ValueError):
        APMEngine(small_cfg(), outputs=("st", "tf"))
    bad = tf_cfg()
    bad["gpu"]["trafficWatch"]["rules"] = [{"short": 6, "drop": 0.5}, {"short": 1, "drop": 0.5}]
    with pytest.raises(ValueError):
        APMEngine(bad, outputs=("st", "tf"))
    wide = tf_cfg()
    wide["gpu"]["trafficWatch"]["rules"] = [{"short": 9, "drop": 0.5}]   # windowSizeInIntervals is 8
    with pytest.raises(ValueError):
        APMEngine(wide, outputs=("st", "tf"))
    # the native constructor checks the tables it is handed as well
    N = _native.load()
    ecfg = engine_config(tf_cfg(), outputs=("st", "tf"))
    w = ecfg["window"]
    one = {"tf_drop": [500], "tf_surge": [0], "tf_z": [0]}
    for over in (dict(one, tf_short=[w + 1]), {"tf_short": [], "tf_drop": [], "tf_surge": [], "tf_z": []},
                 {"tf_classes": []}, {"tf_classes": [[]]}, {"tf_classes": [[], [5, 1]]}, {"tf_classes": [[], [0]]},
                 {"tf_classes": [[], [2 ** 31]]}, {"tf_classes": [[5]]}, {"tf_default": 7}, {"tf_services": {"x": 9}}):
        with pytest.raises(ValueError):
            N.Engine(dict(ecfg, **over))
    for over in (dict(one, tf_short=[0]), dict(one, tf_short=[65]), dict(one, tf_short=[1], tf_drop=[1000]),
                 dict(one, tf_short=[1], tf_drop=[0]), dict(one, tf_short=[1], tf_surge=[1000]),
                 dict(one, tf_short=[1], tf_surge=[1000001]), dict(one, tf_short=[1], tf_z=[100001]),
                 dict(one, tf_short=[1], tf_z=[-1]), dict(one, tf_short=[1, 2]), {"tf_min_buckets": 2}):
        with pytest.raises(ValueError):
            N.Engine(dict(ecfg, **over))


def test_full_pipeline_matches_oracle_and_changes_nothing_else():
    _lines, bl = load(seed=1, duration=300)
    C = tf_cfg()
    kinds = KINDS + ("tf",)
    eng, on = run(C, bl, kinds, kinds=kinds)
    off_eng, off = run(plain_cfg(), bl, KINDS, kinds=KINDS + ("tf",))
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    assert 20 < len(P.tf) < len(P.stats) - 50
    verdicts = collections.Counter(g.split(":")[5] for r in P.tf for g in r.split("|")[6].split(","))
    assert verdicts["D"] > 5 and verdicts["S"] > 5 and verdicts["N"] > 5
    groups = lambda name: [g.split(":") for r in P.tf if r.split("|")[3] == name for g in r.split("|")[6].split(",")]
    # the stopped service: a D row with nothing in the newest bucket
    assert any(g[2] == "0" and g[5] == "D" for g in groups("S:" + STOPS))
    assert not any(g[5] == "S" for g in groups("S:" + STOPS))
    # the flooded one: S rows whose R is more than five times k' times the median (2 R > 5 k med2)
    flooded = [g for g in groups("S:" + FLOODS) if g[5] == "S"]
    assert len(flooded) > 5 and not any(g[5] == "D" for g in groups("S:" + FLOODS))
    assert any(g[0] == "1" and 2 * int(g[2]) > 5 * 1 * int(g[3]) for g in flooded)
    assert any(g[0] == "3" and 2 * int(g[2]) > 5 * 3 * int(g[3]) for g in flooded)
    # before the cut the load's own jitter prints next to nothing at these rules (a row's timestamp
    # is the start of its newest bucket: the first rows of the cut carry cut - 10 s)
    cut_ts = START + 180_000
    assert sum(1 for r in P.tf if int(r.split("|")[1]) < cut_ts - 10_000) <= 5
    assert not any(r.split("|")[3] == "S:getSvc0003" for r in P.tf)
    # record for record
    assert len(on["tf"]) == len(P.tf)
    for got, want in zip(on["tf"], P.tf):
        assert got == want and entry_from_csv(got) == entry_from_csv(want)
    assert off["tf"] == [] and off_eng.eng.traffic() == [] and off_eng.metrics()["tf_rows"] == 0
    assert eng.metrics()["tf_rows"] == len(P.tf)
    # with the stream on, every other stream's bytes are those of a run with it off
    for k in ("st", "fs", "al", "audit_db", "transactions"):
        assert on[k] == off[k], k
    assert collections.Counter(on["db"]) == collections.Counter(off["db"]) and len(on["db"]) > 100
    assert on["st"] == P.stats
    # rows stand in st order with the st rows' timestamps
    st_keys = [tuple(l.split("|")[1:4]) for l in on["st"]]
    tf_keys = [tuple(r.split("|")[1:4]) for r in on["tf"]]
    have = set(tf_keys)
    assert len(have) == len(tf_keys) and tf_keys == [k for k in st_keys if k in have]
    # the read-back holds the last rollover's records per series id, for series that did not fire too
    last_ts = on["st"][-1].split("|")[1]
    last = sorted(int(f[4]) for f in (r.split("|") for r in on["tf"]) if f[1] == last_ts)
    dev = eng.eng.traffic()
    assert any(d is None for d in dev)                       # S:getSvc0003: class 0
    recs = [d for d in dev if d is not None]
    assert sorted(n for n, per in recs if any(p[4] != "N" for p in per)) == last
    assert any(all(p[4] == "N" for p in per) for _n, per in recs) and all(len(per) == 2 for _n, per in recs)
    # the sum of a series' counts is K8's n: R plus a baseline of B buckets never exceeds it
    assert all(per[0][1] <= n for n, per in recs)


def test_key_set_and_stream_off_allocates_and_launches_nothing():
    """The key set and the stream off: the engine holds exactly the device blocks, bytes, pinned
    blocks, events and streams of an engine whose config never names the key, keeps no record
    (traffic() is empty: no value pass ran) and prints what that engine prints."""
    _lines, bl = load(seed=3, duration=150)
    gc.collect()
    N = _native.load()
    COUNTS = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes", "events", "streams")
    before = dict(N.live_resources())
    plain, out0 = run(plain_cfg(), bl, KINDS)
    one = {k: N.live_resources()[k] - before[k] for k in COUNTS}
    keyed, out1 = run(tf_cfg(), bl, KINDS, kinds=KINDS + ("tf",))
    two = {k: N.live_resources()[k] - before[k] for k in COUNTS}
    assert two == {k: 2 * one[k] for k in COUNTS}
    assert keyed.eng.device_bytes() == plain.eng.device_bytes()
    assert out1["tf"] == [] and keyed.eng.traffic() == [] and keyed.metrics()["tf_rows"] == 0
    for k in KINDS:
        if k == "db":
            assert collections.Counter(out0[k]) == collections.Counter(out1[k])
        else:
            assert out0[k] == out1[k], k
    on, out2 = run(tf_cfg(), bl, KINDS + ("tf",), kinds=KINDS + ("tf",))
    assert len(out2["tf"]) > 5 and on.eng.device_bytes() > plain.eng.device_bytes()   # the stream's memory is accounted for
    del on, out2, plain, keyed, out0, out1
    gc.collect()
    after = dict(N.live_resources())
    assert {k: after[k] for k in COUNTS} == {k: before[k] for k in COUNTS}


def test_checkpoint_resumes_the_stream(tmp_path):
    _lines, bl = load(seed=6, duration=300, frac=0.3)   # (rows on both sides of the checkpoint)
    C = tf_cfg()
    kinds = KINDS + ("tf",)
    _e, full = run(C, bl, kinds, kinds=kinds)
    cut = len(bl) // 2
    eng, head = run(C, bl[:cut], kinds, kinds=kinds)
    ck = str(tmp_path / "engine.ckpt")
    assert eng.save_state(ck) > 0
    del eng
    eng2 = APMEngine(C, outputs=kinds)
    eng2.load_state(ck)
    _e, tail = run(C, bl[cut:], kinds, eng=eng2, kinds=kinds)
    assert len(tail["tf"]) > 5 and len(head["tf"]) > 2
    assert head["tf"] + tail["tf"] == full["tf"]
    assert head["st"] + tail["st"] == full["st"]


def run_node(world, bl, servers):
    """`world` engines with the tf stream on, one host thread each, joined by an in-process
    collective group with lock-step clocks (the harness of tests/test_hist_engine_gpu.py)."""
    group = _native.load().LocalCollGroup(world, 120000.0)
    shards = shard_servers(servers, world)
    engs, outs, errs = [], [], []
    for r in range(world):
        eng = APMEngine(tf_cfg(), keep_text=True, outputs=("tf",))
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
                for k in ("st", "tf"):
                    outs[r][k] += engs[r].take(k)
            fleet.drain_alerts()
            for k in ("st", "tf"):
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
    lines, bl = load(seed=2, duration=200, servers=4)
    servers = sorted({server_of(fp) for fp in lines})
    P = PipelineOracle(tf_cfg(), UTC)
    P.run_batches(bl)
    _e1, one, _s = run_node(1, bl, servers)
    _e2, two, shards = run_node(2, bl, servers)
    assert one[0]["tf"] == P.tf and len(P.tf) > 20
    for r in range(2):
        assert {l.split("|")[2] for l in two[r]["tf"]} <= set(shards[r]) and len(two[r]["tf"]) > 5
        stamps = [int(l.split("|")[1]) for l in two[r]["tf"]]
        assert stamps == sorted(stamps)
    assert collections.Counter(two[0]["tf"] + two[1]["tf"]) == collections.Counter(one[0]["tf"])


def test_a_reload_past_the_window_bound_is_refused():
    """The value pass takes windows up to traffic_max_win() buckets.  A reload that asks for more is
    refused when it is staged, whole, and the engine goes on with the window it has; an engine
    without the stream takes the same reload."""
    N = _native.load()
    _lines, bl = load(seed=4, duration=150)
    C = tf_cfg()
    eng = APMEngine(C, outputs=("st", "tf"))
    long = copy.deepcopy(C)
    long["streamCalcStats"]["windowSizeInIntervals"] = N.traffic_max_win()   # one bucket too many
    with pytest.raises(ValueError):
        eng.reload(long, gen=1)
    assert eng.ecfg["window"] == 8 and eng.eng.reconfig_info()["applied"] == 0
    _e, out = run(C, bl, ("st", "tf"), eng=eng, kinds=("st", "tf"))
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    assert out["st"] == P.stats and out["tf"] == P.tf and len(out["tf"]) > 5
    assert eng.eng.reconfig_info()["window_changes"] == 0
    with pytest.raises(ValueError):
        APMEngine(long, outputs=("st", "tf"))                                # the constructor's bound is the same

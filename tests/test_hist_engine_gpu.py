"""The lh stream through the whole engine: parse -> device join -> K7 -> K15, against
PipelineOracle; the other streams unchanged by it; a checkpoint taken mid-run.  (Shapes of
tests/test_engine_gpu.py.)"""
import collections
import copy
import threading

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

from apmbackend_amd.models.oracle import PipelineOracle  # noqa: E402
from apmbackend_amd import _native  # noqa: E402
from apmbackend_amd.models.pipeline import OUT_KINDS, APMEngine  # noqa: E402
from apmbackend_amd.parallel.dist import shard_servers  # noqa: E402
from apmbackend_amd.parallel.fleet import FleetBaseline  # noqa: E402
from apmbackend_amd.utils.config import default_config  # noqa: E402
from apmbackend_amd.utils.synth import Anomaly, Generator, SynthConfig, batches, with_watermarks  # noqa: E402
from apmbackend_amd.utils.timeparse import TzOffset  # noqa: E402

UTC = TzOffset("UTC")
START = 1578391200000
KINDS = ("transactions", "audit_db", "db", "st", "fs", "al")


def small_cfg(mode="exact"):
    C = default_config(replay=True)
    C["streamCalcZScore"]["defaults"] = [{"LAG": 6, "THRESHOLD": 3.0, "INFLUENCE": 0.5},
                                         {"LAG": 30, "THRESHOLD": 2.0, "INFLUENCE": 0.0}]
    C["streamCalcZScore"]["overrides"]["services"]["S:getSvc0002"] = {"6": {"THRESHOLD": 4.0, "INFLUENCE": 0.25}}
    C["streamProcessAlerts"]["rollingAlertWindowSizeInIntervals"] = 10
    C["streamProcessAlerts"]["requiredNumberBadIntervalsInAlertWindowToTrigger"] = 3
    C["streamProcessAlerts"]["perServiceAlertCooldownInMinutes"] = 2
    C["gpu"].update({"emulateOverrideAliasing": True, "zscoreMeanMode": mode, "timezone": "UTC",
                     "maxSeries": 4096, "batchBytes": 4 << 20, "maxLinesPerBatch": 1 << 16,
                     "bucketCellCapacity": 8, "bucketOverflowCapacity": 1 << 16})
    return C


def synth_batches(seed=1, duration=300, servers=2):
    an = [Anomaly("jvm00", "getSvc0001", START + 400_000, START + 1100_000, 30.0)]
    cfg = SynthConfig(servers=servers, duration_s=duration, tx_per_sec_per_server=3, seed=seed,
                      ejb_services=4, provider_services=3, anomalies=an)
    lines = Generator(cfg).generate()
    return lines, with_watermarks(batches(lines, cfg.start_ms, 5.0), UTC)


def run(C, bl, outputs, eng=None, kinds=KINDS):
    eng = eng or APMEngine(C, outputs=outputs)
    out = collections.defaultdict(list)
    for now, chunks in bl:
        eng.process_lines(chunks, now)
        for k in kinds:
            out[k] += eng.take(k)
    return eng, out


def test_keep_text_leaves_the_stream_off():
    assert OUT_KINDS[-1] == "lh"
    eng = APMEngine(small_cfg(), keep_text=True)
    assert not (eng.ecfg["outputs"] >> OUT_KINDS.index("lh")) & 1


def test_full_pipeline_matches_oracle_and_changes_nothing_else():
    _lines, bl = synth_batches(seed=1, duration=300)
    C = small_cfg()
    assert C["gpu"].get("joinOnDevice", True)
    _e, on = run(C, bl, KINDS + ("lh",), kinds=KINDS + ("lh",))
    _e, off = run(C, bl, KINDS)
    Co = copy.deepcopy(C)
    Co["gpu"]["latencyHistogram"] = True
    P = PipelineOracle(Co, UTC)
    P.run_batches(bl)
    assert len(P.lh) > 100
    assert on["lh"] == P.lh
    for k in ("st", "fs", "al", "audit_db", "transactions"):
        assert on[k] == off[k], k
    # released tx: the same records in the same endTs order; the order among equal endTs is not
    # pinned anywhere in the project (tests/test_engine_gpu.py compares multisets too)
    assert collections.Counter(on["db"]) == collections.Counter(off["db"]) and len(on["db"]) > 100
    ends = lambda rows: [int(l.split("|")[6]) for l in rows]
    assert ends(on["db"]) == ends(off["db"]) == sorted(ends(on["db"]))
    assert on["st"] == P.stats


def test_checkpoint_resumes_the_stream(tmp_path):
    _lines, bl = synth_batches(seed=6, duration=300)
    C = small_cfg()
    kinds = KINDS + ("lh",)
    _e, full = run(C, bl, kinds, kinds=kinds)
    cut = len(bl) // 2
    eng, head = run(C, bl[:cut], kinds, kinds=kinds)
    ck = str(tmp_path / "engine.ckpt")
    assert eng.save_state(ck) > 0
    del eng
    eng2 = APMEngine(C, outputs=kinds)
    eng2.load_state(ck)
    _e, tail = run(C, bl[cut:], kinds, eng=eng2, kinds=kinds)
    assert len(tail["lh"]) > 20
    assert head["lh"] + tail["lh"] == full["lh"]
    assert head["st"] + tail["st"] == full["st"]


# ------------------------------------------------------------------------------- two ranks

def server_of(fp):
    return fp.split("/")[2]


def run_node(world, bl, servers):
    """`world` engines with the lh stream on, one host thread each, joined by an in-process
    collective group with lock-step clocks (the harness of tests/test_node_gpu.py)."""
    group = _native.load().LocalCollGroup(world, 120000.0)
    shards = shard_servers(servers, world)
    engs, outs, errs = [], [], []
    for r in range(world):
        eng = APMEngine(small_cfg(), keep_text=True, outputs=("lh",))
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
                for k in ("st", "lh"):
                    outs[r][k] += engs[r].take(k)
            fleet.drain_alerts()
            for k in ("st", "lh"):
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


def test_two_ranks_report_every_bucket_once():
    """World 2, servers sharded.  Rank 1's servers are silent for 100 s in the middle, so that rank
    rolls over through the lock-step clock alone there, and again by its own tx afterwards.  The
    union of the ranks' lh rows is the 1-rank run's (and the oracle's) as a multiset, and no rank
    reports a (bucket, series) twice."""
    lines, bl = synth_batches(seed=2, duration=300, servers=4)
    servers = sorted({server_of(fp) for fp in lines})
    quiet = set(shard_servers(servers, 2)[1])
    bl = [(now, [(fp, ls) for fp, ls in chunks if not (20 <= i < 40 and server_of(fp) in quiet)])
          for i, (now, chunks) in enumerate(bl)]
    Co = small_cfg()
    Co["gpu"]["latencyHistogram"] = True
    P = PipelineOracle(Co, UTC)
    P.run_batches(bl)
    _e1, one, _s = run_node(1, bl, servers)
    engs, two, shards = run_node(2, bl, servers)
    assert one[0]["lh"] == P.lh and len(P.lh) > 200
    for r in range(2):
        rows = two[r]["lh"]
        keys = [tuple(l.split("|")[1:4]) for l in rows]
        assert len(set(keys)) == len(keys), f"rank {r} reported a (bucket, series) twice"
        assert {k[1] for k in keys} <= set(shards[r])
        stamps = [int(k[0]) for k in keys]
        assert stamps == sorted(stamps)
    assert collections.Counter(two[0]["lh"] + two[1]["lh"]) == collections.Counter(one[0]["lh"])
    # rank 1 did roll over on the other rank's clock while its own servers were silent
    assert engs[1].metrics()["lockstep_rollovers"] >= 8
    quiet_rows = [l for l in two[1]["lh"] if START + 110_000 <= int(l.split("|")[1]) < START + 190_000]
    assert quiet_rows == []

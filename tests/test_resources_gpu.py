"""Every device block, pinned block, event and stream an engine creates goes back when the
engine does: the process-wide live counts of the resource owners (csrc/runtime/hipres.h,
``_apm_native.live_resources()``) return exactly to their starting values.  Four short runs with
the shapes of tests/test_engine_gpu.py, each across a dozen interval edges so the lazily made
staging, format-ring, release and histogram buffers all exist."""
import collections
import gc
import threading

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover - CPU containers
    pytest.skip("no GPU", allow_module_level=True)

from apmbackend_amd import _native  # noqa: E402
from apmbackend_amd.models.pipeline import APMEngine  # noqa: E402
from apmbackend_amd.parallel.dist import shard_servers  # noqa: E402
from apmbackend_amd.parallel.fleet import FleetBaseline  # noqa: E402
from test_engine_gpu import small_cfg, synth_batches  # noqa: E402

KINDS = ("transactions", "audit_db", "db", "st", "fs", "al")
COUNTS = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes", "events", "streams")


def cfg(**gpu):
    C = small_cfg()
    C["gpu"].update({"joinTableSlots": 1024, "needArenaEntries": 1024, "joinChainBlocks": 1024, "txTextRingMB": 16})
    C["gpu"].update(gpu)
    return C


def live():
    return dict(_native.load().live_resources())


def feed(eng, bl, kinds):
    out = collections.defaultdict(list)
    for now, chunks in bl:
        eng.process_lines(chunks, now)
        for k in kinds:
            out[k] += eng.take(k)
    return out


def check_live(start, engines):
    """The owners' device bytes are the engines' own figure; pinned blocks and events exist."""
    now = live()
    assert now["device_bytes"] - start["device_bytes"] == sum(e.eng.device_bytes() for e in engines)
    assert now["device_blocks"] > start["device_blocks"]
    assert now["pinned_blocks"] > start["pinned_blocks"] and now["pinned_bytes"] > start["pinned_bytes"]
    assert now["events"] > start["events"] and now["streams"] > start["streams"]


@pytest.fixture
def start():
    gc.collect()
    before = live()
    yield before
    gc.collect()
    after = live()
    assert {k: after[k] for k in COUNTS} == {k: before[k] for k in COUNTS}


@pytest.fixture(scope="module")
def corpus():
    return synth_batches(seed=5, duration=120)  # 24 batches of 5 s: 12 interval edges


def test_device_join_all_outputs(start, corpus):
    _lines, bl = corpus
    eng = APMEngine(cfg(), outputs=KINDS + ("lh",))
    out = feed(eng, bl, KINDS + ("lh",))
    assert len(out["st"]) > 0 and len(out["fs"]) > 0 and len(out["db"]) > 0 and len(out["lh"]) > 0
    check_live(start, [eng])
    del eng


def test_host_join(start, corpus):
    _lines, bl = corpus
    eng = APMEngine(cfg(joinOnDevice=False), keep_text=True)
    out = feed(eng, bl, KINDS)
    assert len(out["st"]) > 0 and len(out["db"]) > 0
    check_live(start, [eng])
    del eng


def test_two_ranks_lockstep(start):
    """Two engines in one in-process group.  Lock-step clocks and the node-wide cooldown are both
    switched on explicitly: together they are the engine's node mode (fleet_setup), so the fleet
    buffers, the fb staging, the node-metrics reduction and the node candidate exchange all
    allocate."""
    lines, bl = synth_batches(seed=5, duration=120, servers=4)
    server_of = lambda fp: fp.split("/")[2]  # noqa: E731
    servers = sorted({server_of(fp) for fp in lines})
    world = 2
    group = _native.load().LocalCollGroup(world, 120000.0)
    shards = shard_servers(servers, world)
    engs, errs, fb = [], [], [0] * world
    for r in range(world):
        eng = APMEngine(cfg(nodeCooldown=True), keep_text=True)
        assert eng.ecfg["node_cooldown"] == 1
        for _now, chunks in bl:
            for fp, _ls in chunks:
                if server_of(fp) in shards[r]:
                    eng.add_file(fp)
        engs.append(eng)

    def rank_main(r):
        try:
            fleet = FleetBaseline(engs[r], world, r, max_services=64, lockstep=True, local_group=group,
                                  servers=servers)
            for now, chunks in bl:
                engs[r].process_lines([(fp, ls) for fp, ls in chunks if server_of(fp) in shards[r]], now)
                fb[r] += len(engs[r].take("fb"))
            fleet.drain_alerts()
            fb[r] += len(engs[r].take("fb"))
        except Exception as e:  # pragma: no cover - reported below
            errs.append((r, repr(e)))

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    assert not errs, errs
    assert all(not t.is_alive() for t in th)
    assert sum(fb) > 0  # the fb staging (device and pinned) was used
    for e in engs:
        assert e.eng.fleet_info()["nranks"] == world
        assert e.eng.node_metrics()[0] == world  # the node-metrics all-reduce ran (lock-step rounds)
        # one exchange (and one node round) per batch; the last two may still be open (device join)
        assert e.eng.fleet_rounds() >= len(bl) - 2
    check_live(start, engs)
    del engs, eng, group, th


def test_checkpoint_then_trim(start, corpus, tmp_path):
    _lines, bl = corpus
    eng = APMEngine(cfg(), keep_text=True)
    feed(eng, bl[:-4], KINDS)
    assert eng.checkpoint_async(str(tmp_path / "engine.rank0")) > 0
    assert eng.checkpoint_wait() > 0
    feed(eng, bl[-4:], KINDS)
    check_live(start, [eng])
    before, after = eng.eng.trim_device_memory()
    assert after <= before and after == eng.eng.device_bytes()
    check_live(start, [eng])
    del eng

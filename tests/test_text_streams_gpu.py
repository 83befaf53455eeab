"""The text slots the lh, wp, sl and sv streams share (engine.h TextStream), through the whole
engine in one run with all four on: a slot is taken again while its output-lane task may be
outstanding (several rollovers), and the device output of a slot that was used is regrown (a much
longer service name first appears between two rollovers).  About 70 series cross the 64-row write
block; one series holds more samples than every stream's group pass takes, so both value paths
run.  Every stream's rows must equal PipelineOracle's."""
import copy

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

from apmbackend_amd import _native  # noqa: E402
from apmbackend_amd.models.oracle import PipelineOracle  # noqa: E402
from apmbackend_amd.utils.synth import Generator, SynthConfig, batches, with_watermarks  # noqa: E402

from test_hist_engine_gpu import KINDS, START, UTC, run, small_cfg  # noqa: E402

STREAMS = ("lh", "wp", "sl", "sv")
HEAVY_EJB, HEAVY, HEAVY_ROW = "getHeavy", "Provider[cb-heavy]", "Provider:cb-heavy"   # (as logged, as printed)
LONG_EJB, LONG = "get" + "L" * 300, "Provider[cb-" + "l" * 280 + "]"
LONG_FROM = 4          # the bucket whose transactions bring the long names
BUCKETS = 9
# (position of the sample count in a row, position of the service)
FIELDS = {"lh": (4, 3), "wp": (4, 3), "sl": (4, 3), "sv": (4, 2)}


def streams_cfg():
    C = small_cfg()
    C["streamCalcStats"]["windowSizeInIntervals"] = 6
    C["streamCalcStats"]["bufferSizeInIntervals"] = 1
    C["gpu"]["latencyHistogram"] = True
    C["gpu"]["windowPercentiles"] = [50, 99.9]
    C["gpu"]["latencyObjectives"] = {"default": [200, 1000]}
    C["gpu"]["serviceWindow"] = {"percentiles": [50, 75, 95]}
    return C


def build_batches():
    """Bucket 0: every service once or more on both servers and ~4500 samples of HEAVY on jvm00;
    every later bucket a few transactions per server; from bucket LONG_FROM on the long names."""
    cfg = SynthConfig(servers=2, ejb_services=20, provider_services=14, seed=2021, sub_calls=(1, 2),
                      noise_lines_per_tx=1, audit_fraction=0.0, missing_logid_fraction=0.0, no_acct_fraction=0.0,
                      soap_late_fraction=0.0)
    g = Generator(cfg)
    ejbs, provs = list(g.ejb), list(g.prov)
    g.base.update({HEAVY_EJB: 400.0, HEAVY: 1.0, LONG_EJB: 300.0, LONG: 50.0})
    idx = [0]

    def tx(server, t, ejb, prov, n_sub):
        g.ejb, g.prov, cfg.sub_calls = ejb, prov, (n_sub, n_sub)
        idx[0] += 1
        g.transaction(server, START + t, idx[0])

    for si, server in enumerate(g.server_names):
        for j, e in enumerate(ejbs):   # every EJB service, every provider
            tx(server, 100 + 97 * j + 13 * si, [e], [provs[j % len(provs)]], 1)
    for j in range(75):
        tx("jvm00", 3000 + 40 * j, [HEAVY_EJB], ["cb-heavy"], 60)
    for b in range(1, BUCKETS):
        for si, server in enumerate(g.server_names):
            for j in range(6):
                tx(server, b * 10000 + 500 + 1300 * j + 50 * si, ejbs, provs, 2)
            if b >= LONG_FROM:
                tx(server, b * 10000 + 9000 + 50 * si, [LONG_EJB], [LONG[9:-1]], 1)
    for fp in g.lines:
        g.lines[fp].sort(key=lambda x: (x[0], x[1]))
    return with_watermarks(batches(g.lines, START, 5.0), UTC)


@pytest.fixture(scope="module")
def both():
    """(oracle, engine rows per kind) of the one run all four cases read."""
    bl = build_batches()
    C = streams_cfg()
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    kinds = KINDS + STREAMS
    _e, out = run(C, bl, kinds, kinds=kinds)
    assert out["st"] == P.stats
    return P, out


@pytest.mark.parametrize("stream", STREAMS)
def test_slot_reuse_and_regrow(both, stream):
    P, out = both
    N = _native.load(build_if_missing=False)
    group_max = {"lh": N.hist_group_max(), "wp": N.winpct_group_max(), "sl": N.slo_group_max(),
                 "sv": N.svcwin_group_max()}[stream]
    want = getattr(P, stream)
    cnt, svc = FIELDS[stream]
    rows = [r.split("|") for r in want]
    stamps = sorted({int(f[1]) for f in rows})
    # the input does what the test is about: four rollovers and more print rows, so both slots are
    # taken twice; the long names come after both slots were used and stay for two rollovers, so
    # each slot's output is regrown once; more series than a write block; both value paths
    assert len(stamps) >= 4
    long_stamps = sorted({int(f[1]) for f in rows if len(f[svc]) >= 280})
    assert len(long_stamps) >= 2 and stamps.index(long_stamps[0]) >= 2
    per_stamp = max(sum(1 for f in rows if int(f[1]) == t) for t in stamps)
    assert per_stamp > (64 if stream != "sv" else 30)   # (sv: one row per service)
    assert len({tuple(r.split("|")[2:4]) for r in P.stats}) > 64
    counts = [int(f[cnt]) for f in rows if f[svc] == HEAVY_ROW]
    assert counts and max(counts) > group_max and min(int(f[cnt]) for f in rows) <= 8
    assert out[stream] == want

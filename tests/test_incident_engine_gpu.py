"""The ic stream through the whole engine: parse -> device join -> K7 -> K8 -> K22 / K24 -> K25,
against the CPU engine record for record and against tests/incident_ref.py driven by the tf and ls
rows alone, over the synthetic replay of tests/test_shift_engine_gpu.py with one server's calls of
one service slowed for a stretch and then restored; the stream off; the errors; a checkpoint and a
restore; a capacity growth mid-run."""
import collections
import copy
import gc
import struct

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

from apmbackend_amd import _native  # noqa: E402
from apmbackend_amd.models.oracle import PipelineOracle  # noqa: E402
from apmbackend_amd.models.pipeline import TOTAL_OUT_KINDS, APMEngine, engine_config  # noqa: E402
from apmbackend_amd.utils.records import entry_from_csv  # noqa: E402
from apmbackend_amd.utils.synth import Anomaly, Generator, SynthConfig, batches, with_watermarks  # noqa: E402

import incident_ref as R  # noqa: E402
from test_hist_engine_gpu import KINDS, START, UTC, run, small_cfg  # noqa: E402
from test_shift_engine_gpu import KEY as LS_KEY, SLOW, SLOW_SERVER  # noqa: E402
from test_traffic_engine_gpu import KEY as TF_KEY  # noqa: E402

IC_KEY = {"sources": {"ls": {"openAfter": 2, "closeAfter": 3}, "tf": {"openAfter": 2, "closeAfter": 3}}, "remindEvery": 4}
ON = KINDS + ("tf", "ls", "ic")


def ic_cfg(key=IC_KEY, **gpu):
    C = small_cfg()
    C["streamCalcStats"]["windowSizeInIntervals"] = 12
    C["gpu"]["latencyShift"] = copy.deepcopy(LS_KEY)
    C["gpu"]["trafficWatch"] = copy.deepcopy(TF_KEY)
    if key is not None:
        C["gpu"]["incidents"] = copy.deepcopy(key)
    C["gpu"].update(gpu)
    return C


def load(seed=1, duration=360, servers=3, lo=0.4, hi=0.55):
    """SLOW_SERVER's calls of SLOW take thirty times as long from lo * duration to hi * duration: the
    stretch at which the reference alone opens an ls incident on the series and closes it again
    before the run ends (the counts are asserted below)."""
    an = [Anomaly(SLOW_SERVER, SLOW, START + int(duration * 1000 * lo), START + int(duration * 1000 * hi), 30.0)]
    cfg = SynthConfig(servers=servers, duration_s=duration, tx_per_sec_per_server=3, seed=seed,
                      ejb_services=4, provider_services=3, anomalies=an)
    return with_watermarks(batches(Generator(cfg).generate(), cfg.start_ms, 5.0), UTC)


_shared = {}


def replay():
    """The replay, the CPU engine's streams and the engine's, once for the tests that read them."""
    if not _shared:
        bl = load()
        C = ic_cfg()
        P = PipelineOracle(copy.deepcopy(C), UTC)
        P.run_batches(bl)
        eng, on = run(C, bl, ON, kinds=ON)
        _shared.update(bl=bl, P=P, eng=eng, on=on)
    return _shared["bl"], _shared["P"], _shared["eng"], _shared["on"]


def reference_rows(P):
    """incident_ref alone over the CPU engine's st, tf and ls rows: per rollover the series in st order,
    a source's code from the verdicts of its row (the lowest-numbered rule that is not N)."""
    def codes_of(rows):
        out = collections.defaultdict(dict)
        for r in rows:
            e = entry_from_csv(r)
            code = next((x[-1] for x in e.rules if x[-1] != "N"), "")
            out[int(e.timestamp)][(e.server, e.service)] = code
        return out
    tf, ls = codes_of(P.tf), codes_of(P.ls)
    by_ts = collections.OrderedDict()
    for r in P.stats:
        f = r.split("|")
        by_ts.setdefault(int(f[1]), []).append((f[2], f[3]))
    book = R.Book({k: (v["openAfter"], v["closeAfter"]) for k, v in IC_KEY["sources"].items()}, IC_KEY["remindEvery"])
    rows = []
    for ts, series in by_ts.items():
        rows += book.step_all(ts, [(k, k[0], k[1], {"tf": tf[ts].get(k, ""), "ls": ls[ts].get(k, "")}) for k in series])
    return rows, book


def test_full_pipeline_matches_the_cpu_engine_and_the_reference():
    bl, P, eng, on = replay()
    want, book = reference_rows(P)
    ev = collections.Counter((r.split("|")[4], r.split("|")[5]) for r in want)
    # the reference alone opens and closes: an empty comparison cannot pass
    assert ev[("ls", "O")] >= 1 and ev[("ls", "C")] >= 1 and sum(v for (s, e), v in ev.items() if e == "O") >= 2
    slow = [r.split("|") for r in want if r.split("|")[2] == SLOW_SERVER and r.split("|")[3] == "S:" + SLOW and r.split("|")[4] == "ls"]
    assert [f[5] for f in slow][0] == "O" and [f[5] for f in slow][-1] == "C" and "S" in [f[5] for f in slow]
    assert P.ic == want                                       # the CPU engine against the reference
    assert len(on["ic"]) == len(want)
    for got, w in zip(on["ic"], want):                        # the HIP engine, record for record
        assert got == w and entry_from_csv(got) == entry_from_csv(w)
    m = eng.metrics()
    assert m["ic_rows"] == len(want)
    assert [m["ic_open_sb"], m["ic_open_tf"], m["ic_open_po"], m["ic_open_ls"]] == \
        [0, book.open_count("tf"), 0, book.open_count("ls")]
    assert on["tf"] == P.tf and on["ls"] == P.ls and on["st"] == P.stats
    # the read-back: per series id None or the per-source states; sb and po are not configured
    names = {}
    for r in on["st"]:
        f = r.split("|")
        names.setdefault((f[2], f[3]), len(names))
    dev = eng.eng.incidents()
    assert len(dev) == len(names)
    open_dev = sorted((k, d[k][0], d[k][1], d[k][2]) for d in dev if d is not None for k in (1, 3) if d[k][0])
    open_ref = sorted((R.SOURCES.index(s), st["code0"], st["since"], st["age"]) for (_k, s), st in book.states.items()
                      if st["code0"])
    assert open_dev == open_ref
    assert all(d is None or (d[0] is None and d[2] is None) for d in dev)


def test_stream_off_allocates_nothing_and_changes_nothing():
    bl, _P, eng_on, on = replay()
    gc.collect()
    N = _native.load()
    COUNTS = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes", "events", "streams")
    off_kinds = KINDS + ("tf", "ls")
    before = dict(N.live_resources())
    plain, out0 = run(ic_cfg(None), bl, off_kinds, kinds=off_kinds + ("ic",))
    one = {k: N.live_resources()[k] - before[k] for k in COUNTS}
    keyed, out1 = run(ic_cfg(), bl, off_kinds, kinds=off_kinds + ("ic",))   # the key set, the stream off
    two = {k: N.live_resources()[k] - before[k] for k in COUNTS}
    assert two == {k: 2 * one[k] for k in COUNTS}
    assert keyed.eng.device_bytes() == plain.eng.device_bytes() < eng_on.eng.device_bytes()
    assert out1["ic"] == [] and keyed.eng.incidents() == [] and keyed.metrics()["ic_rows"] == 0
    assert not (keyed.ecfg["outputs"] >> TOTAL_OUT_KINDS.index("ic")) & 1
    for k in off_kinds:                                       # every other stream's bytes, on or off
        if k == "db":
            assert collections.Counter(out0[k]) == collections.Counter(out1[k]) == collections.Counter(on[k])
        else:
            assert out0[k] == out1[k] == on[k], k


def test_errors():
    with pytest.raises(ValueError):
        APMEngine(ic_cfg(None), outputs=("st", "tf", "ls", "ic"))          # "ic" without the key
    with pytest.raises(ValueError):
        APMEngine(ic_cfg(), outputs=("st", "ls", "ic"))                    # source tf is not in outputs
    bad = ic_cfg()
    del bad["gpu"]["trafficWatch"]                                         # source tf without its own stream's key
    with pytest.raises(ValueError):
        APMEngine(bad, outputs=("st", "ls", "ic"))
    assert not (APMEngine(ic_cfg(), keep_text=True).ecfg["outputs"] >> TOTAL_OUT_KINDS.index("ic")) & 1
    # the native constructor checks what it is handed as well
    N = _native.load()
    ecfg = engine_config(ic_cfg(), outputs=("st", "tf", "ls", "ic"))
    assert ecfg["ic_open_after"] == [0, 2, 0, 2] and ecfg["ic_close_after"] == [0, 3, 0, 3]
    for over in ({"ic_open_after": [0, 0, 0, 0], "ic_close_after": [0, 0, 0, 0]}, {"ic_open_after": [0, 256, 0, 2]},
                 {"ic_open_after": [0, 0, 0, 2]}, {"ic_close_after": [0, 3, 0, 0]}, {"ic_close_after": [0, 3, 0, 256]},
                 {"ic_open_after": [0, -1, 0, 2]}, {"ic_open_after": [0, 2, 2]}, {"ic_remind_every": 65536},
                 {"ic_remind_every": -1}, {"ic_open_after": [2, 2, 0, 2], "ic_close_after": [3, 3, 0, 3]},
                 {"outputs": ecfg["outputs"] & ~(1 << TOTAL_OUT_KINDS.index("tf"))}):
        with pytest.raises(ValueError):
            N.Engine(dict(ecfg, **over))


# checkpoint sections in file order (binio.h): those two runs of one replay write byte for byte alike
# (config, clock, parse carry, z-score state, tx pool, alert state, pending outputs, metrics, rings,
# extra), and the three that vary from run to run whatever the streams (see the test)
SEC_TOPOLOGY, SEC_SERIES, SEC_JOIN, SEC_BUCKETS = 2, 3, 5, 7
SEC_EXACT = (1, 4, 6, 8, 9, 10, 11, 12, 13, 14)


def ck_sections(b):
    assert b[:8] == b"APMCKPT\0" and b[-4:] == struct.pack("<I", 0xE0F)
    out, p = collections.OrderedDict(), 12
    while p < len(b) - 4:
        tag, ln = struct.unpack_from("<IQ", b, p)
        assert tag not in out
        out[tag] = b[p + 12:p + 12 + ln]
        p += 12 + ln
    assert p == len(b) - 4
    return out


def ck_strs(b, p):
    (n,) = struct.unpack_from("<Q", b, p)
    p += 8
    out = []
    for _ in range(n):
        (ln,) = struct.unpack_from("<Q", b, p)
        out.append(b[p + 8:p + 8 + ln])
        p += 8 + ln
    return out, p


def ck_topology(b):
    """(servers, [(path, server, kind)], services) of a TOPOLOGY section."""
    servers, p = ck_strs(b, 0)
    (nf,) = struct.unpack_from("<Q", b, p)
    p += 8
    files = []
    for _ in range(nf):
        (ln,) = struct.unpack_from("<Q", b, p)
        path = b[p + 8:p + 8 + ln]
        p += 8 + ln
        server, kind = struct.unpack_from("<iB", b, p)
        p += 5
        files.append((path, server, kind))
    services, p = ck_strs(b, p)
    assert p == len(b)
    return servers, files, services


def ck_series(b, servers, services):
    """[(server name, service name)] per series id of a SERIES section: the ids of the file's own tables
    replaced by the names they stand for."""
    (n,) = struct.unpack_from("<Q", b, 0)
    out = []
    for i in range(n):
        server, service, _key = struct.unpack_from("<iiQ", b, 8 + 16 * i)
        out.append((servers[server], services[service]))
    return out


def compare_checkpoints(tmp_path, bl):
    """A checkpoint taken with the stream on against one taken with it off: the same header and
    version, the same sections with the same lengths, every section that is deterministic byte for
    byte, and the others in the form that is: the topology's tables as sets and the series by the
    names their ids stand for, the buckets as the same bytes in another order.  A second run with the
    stream off calibrates this: whatever is byte-identical between the two runs with the stream off
    must be byte-identical with the stream on too."""
    off_kinds = KINDS + ("tf", "ls")
    files = {}
    for name, key, kinds in (("off", None, off_kinds), ("off2", None, off_kinds), ("on", IC_KEY, ON)):
        eng, _out = run(ic_cfg(key, joinOnDevice=False), bl, kinds, kinds=kinds)
        if name == "on":
            assert any(d is not None and d[3][0] for d in eng.eng.incidents())   # with an incident open
        path = str(tmp_path / (name + ".ckpt"))
        assert eng.save_state(path) > 0
        files[name] = open(path, "rb").read()
        del eng
    on, off, off2 = (ck_sections(files[k]) for k in ("on", "off", "off2"))
    assert files["on"][:12] == files["off"][:12] and len(files["on"]) == len(files["off"])
    assert [(t, len(v)) for t, v in on.items()] == [(t, len(v)) for t, v in off.items()]
    assert list(on) == list(range(1, 15))
    for t in on:
        if t in SEC_EXACT or off[t] == off2[t]:
            assert on[t] == off[t], t
    t_on, t_off = ck_topology(on[SEC_TOPOLOGY]), ck_topology(off[SEC_TOPOLOGY])
    assert t_on[0] == t_off[0] and t_on[1] == t_off[1] and sorted(t_on[2]) == sorted(t_off[2])
    assert ck_series(on[SEC_SERIES], t_on[0], t_on[2]) == ck_series(off[SEC_SERIES], t_off[0], t_off[2])
    assert sorted(on[SEC_BUCKETS]) == sorted(off[SEC_BUCKETS])


def test_checkpoint_restore_closes_everything(tmp_path):
    bl, _P, _eng, _on = replay()
    # the ls incident of the slowed series opens at the edge 160 s into the run and closes at 280 s; an
    # edge trails the newest bucket by the buffer, so three quarters into the batches it is open
    cut = len(bl) * 3 // 4
    C = ic_cfg()
    eng, head = run(C, bl[:cut], ON, kinds=ON)
    assert any(d is not None and d[3][0] for d in eng.eng.incidents())     # an ls incident is open here
    ck = str(tmp_path / "engine.ckpt")
    assert eng.save_state(ck) > 0
    off_kinds = KINDS + ("tf", "ls")
    eng0, _h = run(ic_cfg(None), bl[:cut], off_kinds, kinds=off_kinds)
    ck0 = str(tmp_path / "plain.ckpt")
    assert eng0.save_state(ck0) > 0
    # The state is not checkpointed: the file of a run with the stream on against one with it off.
    # Two checkpoints of one replay are not byte-identical even with the stream off: measured on an
    # MI355X, section by section, two such runs differed in TOPOLOGY and SERIES (the ids the services
    # got), BUCKETS (the same bytes in another order) and JOIN (the device join's section even in its
    # length) and in nothing else.  So the files are compared in a deterministic form, taken with
    # the host join, whose section has a fixed length.
    compare_checkpoints(tmp_path, bl[:cut])
    del eng, eng0
    _bl, P, _e, full = replay()
    plain = APMEngine(ic_cfg(None), outputs=off_kinds)
    plain.load_state(ck)                                                    # the stream-on file into a stream-off engine
    _e, tail_off = run(ic_cfg(None), bl[cut:], off_kinds, eng=plain, kinds=off_kinds)
    eng2 = APMEngine(C, outputs=ON)
    eng2.load_state(ck0)                                                    # ... and the stream-off file into a stream-on one
    for k in ("st", "fs", "tf", "ls"):
        assert head[k] + tail_off[k] == full[k], k
    assert all(d is None for d in eng2.eng.incidents())                     # every incident closed, every run 0
    st, rows, nxt = [], [], cut
    while not st:                                                           # one rollover
        eng2.process_lines(bl[nxt][1], bl[nxt][0])
        st += eng2.take("st")
        rows += eng2.take("ic")
        nxt += 1
    assert len({r.split("|")[1] for r in st}) == 1
    dev = eng2.eng.incidents()
    # openAfter is 2: after one step nothing is open, no run is above 1, and what was open before the
    # restart got no C row
    assert rows == [] and any(d is not None for d in dev)
    assert head["st"] + st == full["st"][:len(head["st"]) + len(st)]
    for d in dev:
        for k, x in enumerate(d or ()):
            assert (x is None) == (k in (0, 2))
            assert x is None or (x[0] == "" and x[3] + x[4] == 1)


def test_capacity_growth_keeps_open_incidents():
    """The state arrays are sized for maxSeries like the cooldown table and never move, so no growth
    of the engine can reach them; the buffers that do grow mid-run are others.  Here the spill lists
    grow (a small bucketOverflowCapacity): an incident is open at a point after a growth, and the
    rows come out as in the run without one."""
    bl, P, _eng, on = replay()
    eng = APMEngine(ic_cfg(bucketOverflowCapacity=64), outputs=ON)
    out = collections.defaultdict(list)
    cut = len(bl) * 3 // 4          # (the ls incident of the slowed series is open here)
    for i, (now, chunks) in enumerate(bl):
        eng.process_lines(chunks, now)
        for k in ON:
            out[k] += eng.take(k)
        if i == cut:
            assert eng.metrics()["spill_grows"] > 0
            assert any(d is not None and d[3][0] == "U" and d[3][2] > 0 for d in eng.eng.incidents())
    assert out["ic"] == on["ic"] == P.ic and out["st"] == on["st"]

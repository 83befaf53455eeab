"""The per-batch parse-stream chain with the device join on: chunk tables uploaded in one launch
(with the zero fills of the selection's counters), host events written to mapped pinned memory by
the selection's scatter, counts / watermark / selection totals exported in one launch.

Every case runs the HIP engine against the CPU oracle of the reference semantics and compares
every output stream with ==.  The corpora are hand-built from independent lines so a batch has an
exact number of kept events, of byte-deferred events (audit lines: the front list; SOAP request /
account lines and CommonTiming exits with a BAF account: the back list) and of host events; the
Python parse model confirms the counts the cases are named after before the GPU runs."""
import collections
import copy
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from apmbackend_amd.models.oracle import PipelineOracle, file_kind  # noqa: E402
from apmbackend_amd.models.pipeline import APMEngine  # noqa: E402
from apmbackend_amd.ops.parse_ref import parse_batch  # noqa: E402
from apmbackend_amd.utils.config import default_config  # noqa: E402
from apmbackend_amd.utils.timeparse import TzOffset  # noqa: E402

UTC = TzOffset("UTC")
KINDS = {"SOAP": 0, "SERVER": 1, "APP": 2}
START = 1578391200000
SERVER = "/net/jvm00/export/jvm1/log/server.log"
APP = "/net/jvm00/export/jvm1/log/app.log"
SOAP = "/net/jvm00/export/jvm1/log/soap_io.log"
STREAMS = ("transactions", "audit_db", "db", "st", "fs", "al")
PM_HOST_LID = "é"  # a non-ASCII logId sends the line to the host pre-pass


def _cfg(max_lines_per_batch=1 << 15, device_join=True):
    C = default_config(replay=True)
    C["streamCalcZScore"]["defaults"] = [{"LAG": 6, "THRESHOLD": 3.0, "INFLUENCE": 0.5}]
    C["gpu"].update({"zscoreMeanMode": "exact", "timezone": "UTC", "maxSeries": 1024, "batchBytes": 2 << 20,
                     "maxLinesPerBatch": max_lines_per_batch, "bucketCellCapacity": 8,
                     "bucketOverflowCapacity": 1 << 16, "joinOnDevice": device_join})
    return C


def _ts(ms):
    import datetime
    s, m = divmod(ms, 1000)
    return datetime.datetime.utcfromtimestamp(s).strftime("%Y-%m-%d %H:%M:%S") + f",{m:03d}"


class Lines:
    """Independent lines, one kept event each (or none: drop()), appended to the three logs of one
    JVM.  `i` numbers the requests so logIds and timestamps differ."""

    def __init__(self, t0=START, lid_suffix=""):
        self.f = collections.OrderedDict(((SERVER, []), (APP, []), (SOAP, [])))
        self.i = 0
        self.t = t0
        self.sfx = lid_suffix
        self.autr = 0  # the last map line's auditTrailId

    def _lid(self):
        self.i += 1
        self.t += 7
        return f"J0-{self.i:07d}{self.sfx}"

    # ---- decided from the Event alone
    def ejb_entry(self):
        self.f[SERVER].append(f"[{self._lid()}] {_ts(self.t)} INFO  [CommonTiming] The EJB call started for bean "
                              f"Delegation method: getSvc{self.i % 3:04d}")

    def ejb_exit(self):
        self.f[SERVER].append(f"[{self._lid()}] {_ts(self.t)} INFO  [CommonTiming] Total time taken for: "
                              f"getSvc{self.i % 3:04d} - {100 + self.i % 400} ms")

    def ct_start(self):
        self.f[APP].append(f"[{self._lid()}] {_ts(self.t)} INFO  CommonTiming::Start: Provider[cb-{self.i % 3}] begin")

    # ---- byte-deferred, back list
    def ct_stop_baf(self, pad=0):
        name = f"Provider[cb-{self.i % 3}{'x' * pad}]"
        self.f[APP].append(f"[{self._lid()}] {_ts(self.t)} [baf][x:y:{1000 + self.i}] INFO  CommonTiming::Stop: {name} "
                           f"- total time {5 + self.i % 300} ms")

    def soap_in(self):
        self.f[SOAP].append(f"=== jbossId={self._lid()} IO=I")

    def soap_acct(self):
        self._lid()
        self.f[SOAP].append(f"      <accountNumber>{4000000000000000 + self.i}</accountNumber>")

    # ---- byte-deferred, front list (audit lines)
    def audit_map(self, pad=0):
        self.f[APP].append(f"[{self._lid()}{'y' * pad}] {_ts(self.t)} [baf][x:{self.i}] INFO  auditTrailId=A{self.i:07d}")
        self.autr = self.i

    def audit_block(self):
        """Header, RequestTrace section, stopWatch list: audit lines (front list) in a row."""
        lid = self._lid()
        self.f[APP] += [f"Audit Trail id : A{self.autr:07d}",
                        f"[{lid}] {_ts(self.t)} INFO  com.acme.Audit: RequestTrace [stopWatchList=",
                        "  RulesEngine:[12 millis] ok", "]", "<stopWatchList>", "  <name>RulesEngine</name>",
                        f"  <startTime>{_ts(self.t).replace(' ', 'T').replace(',', '.')}Z</startTime>",
                        f"  <stopTime>{_ts(self.t + 12).replace(' ', 'T').replace(',', '.')}Z</stopTime>",
                        "</stopWatchList>"]

    def drop(self, fp=SERVER):
        self._lid()
        self.f[fp].append(f"[J0-{self.i:07d}] {_ts(self.t)} DEBUG [com.acme.svc.Handler{self.i % 9}] processed step {self.i}")

    def chunks(self):
        return [(fp, ls) for fp, ls in self.f.items() if ls]


def n_events(chunks, file_open=None):
    """Kept events of one batch by the Python parse model."""
    if not chunks:
        return 0
    bch = [(KINDS[file_kind(fp)], ("\n".join(ls) + "\n").encode()) for fp, ls in chunks]
    ev, _, _, _ = parse_batch(bch, UTC, {} if file_open is None else file_open, list(range(len(chunks))))
    return len(ev)


MIX = ("ejb_entry", "ct_stop_baf", "soap_in", "audit_map", "ejb_exit", "soap_acct", "ct_start")


def mixed_batch(k, t0=START, drops=True):
    """Exactly k kept events of every selection path in turn, dropped lines in between."""
    L = Lines(t0)
    for j in range(k):
        getattr(L, MIX[j % len(MIX)])()
        if drops and j % 3 == 0:
            L.drop((SERVER, APP, SOAP)[j % 3])
    if drops:
        L.drop()
    ch = L.chunks()
    assert n_events(ch) == k
    return ch


def run_both(C, bl, **kw):
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    eng = APMEngine(C, keep_text=True, **kw)
    out = collections.defaultdict(list)
    for now, chunks in bl:
        eng.process_lines(chunks, now)
        for k in STREAMS:
            out[k] += eng.take(k)
    eng.eng.flush()
    for k in STREAMS:
        out[k] += eng.take(k)
    return eng, out, P


def assert_streams(out, P):
    assert out["transactions"] == P.tx_out
    assert out["audit_db"] == P.audit_db
    assert out["st"] == P.stats
    assert out["fs"] == P.fs
    assert out["al"] == P.al
    assert sorted(out["db"]) == sorted(P.tx_db[:len(out["db"])]) or sorted(out["db"]) == sorted(P.tx_db)


def closing_batches(t0, n=4):
    """Later batches that move the clock on, so the stats of the batches under test roll over."""
    bl = []
    for j in range(n):
        L = Lines(t0 + (j + 1) * 20_000)
        L.ejb_entry()
        L.ejb_exit()
        bl.append((t0 + (j + 1) * 20_000 + 1000, L.chunks()))
    return bl


# wave (64), block (256) and scan-tile (4096) edges of the kept-event count
@pytest.mark.parametrize("k", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
def test_kept_event_count_edges(k):
    C = _cfg()
    bl = [(START + 60_000, mixed_batch(k))] + closing_batches(START + 60_000)
    eng, out, P = run_both(C, bl)
    assert_streams(out, P)
    m = eng.metrics()
    assert m["events"] == k + 2 * (len(bl) - 1)
    assert m["join"]["host_fallback"] == 0


def test_empty_and_all_dropped_batches():
    """0 kept events twice over -- no chunk at all, and lines that are all dropped -- between two
    ordinary batches: the counts, the selection totals and the host-event list of the previous
    batch must not leak into them."""
    C = _cfg()
    L = Lines(START + 5000, PM_HOST_LID)
    for _ in range(40):
        L.ejb_entry()
        L.ejb_exit()
    first = L.chunks()
    D = Lines(START + 20_000)
    for j in range(300):
        D.drop((SERVER, APP, SOAP)[j % 3])
    assert n_events(D.chunks()) == 0
    bl = [(START + 10_000, first), (START + 15_000, []), (START + 25_000, D.chunks()),
          (START + 40_000, mixed_batch(100, START + 30_000))] + closing_batches(START + 40_000)
    eng, out, P = run_both(C, bl)
    assert_streams(out, P)
    m = eng.metrics()
    assert m["events"] == 80 + 100 + 2 * 4
    assert m["join"]["host_events"] >= 80


def test_no_deferred_event_and_every_event_deferred():
    """A batch whose events are all decided from the Event alone, then one where every event
    needs its line's bytes, audit lines (front list) alternating with CommonTiming BAF exits and
    followed by SOAP lines (back list) inside the same waves."""
    C = _cfg()
    A = Lines(START + 1000)
    for _ in range(150):
        A.ejb_entry()
        A.ct_start()
        A.ejb_exit()
    B = Lines(START + 20_000)
    for j in range(200):
        B.audit_map()
        B.ct_stop_baf()
        if j % 4 == 0:
            B.audit_block()
        B.soap_in()
        B.soap_acct()
    bl = [(START + 10_000, A.chunks()), (START + 30_000, B.chunks())] + closing_batches(START + 30_000)
    assert n_events(bl[0][1]) == 450 and n_events(bl[1][1]) > 800
    eng, out, P = run_both(C, bl)
    assert_streams(out, P)
    assert len(P.audit_db) > 0 and len(P.tx_out) > 0


def test_deferred_lines_longer_than_the_lds_slot():
    """Byte-deferred lines over 256 bytes (they walk the batch instead of their staged copy): a
    CommonTiming BAF exit and an audit map line, among short ones."""
    C = _cfg()
    L = Lines(START + 1000)
    for j in range(130):
        L.ct_stop_baf(pad=300 if j % 5 == 0 else 0)
        L.audit_map(pad=280 if j % 7 == 0 else 0)
        L.soap_in()
    assert max(len(s) for s in L.f[APP]) > 256
    bl = [(START + 10_000, L.chunks())] + closing_batches(START + 10_000)
    eng, out, P = run_both(C, bl)
    assert_streams(out, P)
    assert len(P.tx_out) > 0


def _host_batch(n, t0):
    L = Lines(t0, PM_HOST_LID)
    for j in range(n):
        (L.ejb_entry if j % 2 == 0 else L.ejb_exit)()
    ch = L.chunks()
    assert n_events(ch) == n
    return ch


def test_first_batch_with_many_host_events():
    """More host-selected events in a fresh engine's first batch than the 256 a first speculative
    copy used to cover: all of them reach the host pre-pass."""
    C = _cfg()
    bl = [(START + 10_000, _host_batch(700, START + 1000))] + closing_batches(START + 10_000)
    eng, out, P = run_both(C, bl)
    assert_streams(out, P)
    assert eng.metrics()["join"]["host_events"] >= 700


def test_host_events_fill_the_configured_capacity():
    """maxLinesPerBatch 512 -> 1024 event slots, and a batch of exactly 1024 events that are all
    host events: the mapped host-event buffers are sized for the capacity."""
    C = _cfg(max_lines_per_batch=512)
    bl = [(START + 10_000, _host_batch(1024, START + 1000))] + closing_batches(START + 10_000)
    eng, out, P = run_both(C, bl)
    assert_streams(out, P)
    m = eng.metrics()
    assert m["events"] == 1024 + 8 and m["join"]["host_events"] >= 1024


def _split(chunks, parts):
    """Every file's lines cut into `parts` chunks, in file order (chunk_next / chunk_first chains)."""
    out = []
    for fp, ls in chunks:
        n = max(1, (len(ls) + parts - 1) // parts)
        out += [(fp, ls[i:i + n]) for i in range(0, len(ls), n)]
    return out


@pytest.mark.parametrize("shape", ["one", "chains", "max_chunks"])
def test_chunk_tables(shape):
    """One chunk; several chunks of each file in a batch (the SOAP chain's next / first links);
    as many chunks as the engine is configured for."""
    C = _cfg()
    kw = {}
    if shape == "one":
        L = Lines(START + 1000)
        for _ in range(90):
            L.ejb_entry()
            L.ejb_exit()
        b0 = L.chunks()
        b1 = _split(mixed_batch(300, START + 12_000), 1)
        assert len(b0) == 1
    elif shape == "chains":
        b0 = _split(mixed_batch(400, START + 1000), 5)
        b1 = _split(mixed_batch(300, START + 12_000), 3)
        assert len(b0) == 15
    else:
        kw["max_chunks"] = 12
        b0 = _split(mixed_batch(400, START + 1000), 4)
        b1 = _split(mixed_batch(90, START + 12_000), 2)
        assert len(b0) == 12
    bl = [(START + 10_000, b0), (START + 20_000, b1)] + closing_batches(START + 20_000)
    # (the oracle reads the files' lines in the same order whatever the chunking)
    eng, out, P = run_both(C, bl, **kw)
    assert_streams(out, P)
    assert len(P.tx_out) > 0


def test_prefetched_batches_use_both_slots():
    """Consecutive batches through the prefetch path (the next batch's parse launched before this
    batch's join), so both parse slots and their pinned blocks are in use; every other batch is
    much smaller than the one before it in the same slot and than its neighbour, with fewer host
    events and fewer chunks, so stale tail entries of either slot would show."""
    C = _cfg()
    sizes = [900, 40, 700, 3, 500, 0, 300, 1]
    bl = []
    for j, k in enumerate(sizes):
        t0 = START + 1000 + j * 10_000
        L = Lines(t0, PM_HOST_LID if j % 2 == 0 else "")
        for q in range(k):
            getattr(L, MIX[q % len(MIX)])()
        ch = L.chunks()
        bl.append((t0 + 9000, _split(ch, 3) if j % 2 == 0 else ch))
    bl += closing_batches(bl[-1][0])
    P = PipelineOracle(copy.deepcopy(C), UTC)
    P.run_batches(bl)
    eng = APMEngine(C, keep_text=True)
    N = eng.N
    bufs = []
    for now, chunks in bl:
        parts, table, off = [], [], 0
        for fp, ls in chunks:
            data = ("\n".join(ls) + "\n").encode()
            table.append((eng.add_file(fp), off, off + len(data)))
            parts.append(data)
            off += len(data)
        blob = b"".join(parts)
        p = N.alloc_pinned(len(blob) + 64)
        N.memcpy_to(p, blob, 0)
        bufs.append((p, len(blob), table, now))
    out = collections.defaultdict(list)
    try:
        for i, (p, n, table, now) in enumerate(bufs):
            if i + 1 < len(bufs):
                q, m, t2, _ = bufs[i + 1]
                eng.eng.process_batch_ptr(p, n, table, now, q, m, t2)
            else:
                eng.eng.process_batch_ptr(p, n, table, now)
            for k in STREAMS:
                out[k] += eng.take(k)
        eng.eng.flush()
        for k in STREAMS:
            out[k] += eng.take(k)
        m = eng.metrics()
    finally:
        del eng
        for p, *_ in bufs:
            N.free_pinned(p)
    assert_streams(out, P)
    assert m["events"] == sum(sizes) + 8


def test_host_join_path_is_unchanged():
    """gpu.joinOnDevice false: the chunk tables still go up in the one launch (three tables, no
    selection counters) and the counts come back in the export launch."""
    C = _cfg(device_join=False)
    bl = [(START + 10_000, mixed_batch(500, START + 1000)), (START + 20_000, mixed_batch(60, START + 12_000))]
    bl += closing_batches(START + 20_000)
    eng, out, P = run_both(C, bl)
    assert out["transactions"] == P.tx_out
    assert out["audit_db"] == P.audit_db
    assert out["st"] == P.stats and out["fs"] == P.fs and out["al"] == P.al
    assert eng.metrics()["events"] == 560 + 8

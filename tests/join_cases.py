"""Hand-built transaction corpora that bracket the tier constants of the device join (K4/K5/K6,
csrc/kernels/devjoin.hip + csrc/runtime/devjoin.cpp).

A case is a name, a list of batches ``[(now_ms, [(path, [lines])])]`` and the facts it claims about
itself (`facts`).  The lines have the exact shapes ``utils.synth.Generator.transaction`` emits; the
clock of every batch is chosen by the case (both ``APMEngine.process_lines`` and the oracles take it
as an argument), and the TTLs are the defaults (record 120 s, account 120 s, need 30 s).

``prove(case)`` shows from CPU models only that the case reaches the tiers it names:
``ops.parse_ref.parse_batch`` gives the ops per key per batch, a replay of the oracle's caches
(``replay``) the open-partial and parked counts and the chain blocks the device must allocate, and
the oracle's emitted lines the byte totals of the 64-line write blocks.

Nothing here needs a GPU at import time (tests/test_join_cases.py runs on any machine).
"""
import collections
import random

from apmbackend_amd.models.oracle import ParseOracle, file_kind
from apmbackend_amd.ops import parse_ref
from apmbackend_amd.utils.synth import LOG_DIR, fmt_iso, fmt_ts
from apmbackend_amd.utils.timeparse import TzOffset

UTC = TzOffset("UTC")
KINDS = {"SOAP": 0, "SERVER": 1, "APP": 2}
START = 1578391200000           # 2020-01-07 10:00:00 UTC, as utils.synth.SynthConfig.start_ms
RECORD_TTL, ACCT_TTL, NEED_TTL = 120000, 120000, 30000

# devjoin.hip (kernel-local constants, mirrored: nothing binds them)
GW_SMALL = 16       # k_group_walk: members sorted in registers, more go to k_group_walk_big
GWB_LDS = 4096      # k_group_walk_big: block_sort_asc in LDS up to here, in global memory above
TXW_LINES = 64      # k_write: output lines per block
TXW_LDS = 8192      # k_write: a block is staged in LDS iff p1 - (p0 & ~3) <= TXW_LDS
EMITTER_STAGED = 2  # Emitter::put: outputs staged per op, the third goes to the overflow list
# devjoin_types.h
KS_PARTS = 5        # KeyState: inline open partials
PBLK_N = 15         # PartBlk: open partials per chain block
NEED_ITEMS = 7      # NeedEnt: inline parked records
NBLK_N = 5          # NeedBlk: parked records per chain block
NEED_LID = 80       # NeedEnt: inline logId bytes
LBLK_N = 240        # LidBlk: logId bytes per chain block

GROUP_SIZES = [1, 2, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097]
OPEN_COUNTS = [4, 5, 6, 19, 20, 21, 35, 36]
PARKED_COUNTS = [1, 2, 3, 6, 7, 8, 11, 12, 13, 18]
DRAIN_WAYS = ["soap", "baf", "ttl"]
LOGID_LENGTHS = [1, 79, 80, 81, 319, 320, 321, 560, 561]
WRITE_TOTALS = list(range(TXW_LDS - 4, TXW_LDS + 5))   # 8188 .. 8196

_PAD = "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789abcdefghijklmnopqrstuvwxyz"


# ------------------------------------------------------------------------------- line helpers

def path(server, kind):
    return LOG_DIR.format(server=server, file=kind)


def soap_in(lid):
    return f"=== jbossId={lid} IO=I"


def soap_out(lid):
    return f"=== jbossId={lid} IO=O"


def soap_acct(acct):
    return f"      <accountNumber>{acct}</accountNumber>"


def soap_key_value(acct):
    return ["      <key>AccountNumber</key>", f"      <value>{acct}</value>"]


def soap_block(lid, acct, risk=False):
    """IO=I, the account (plain or the riskStrategy key / value pair), IO=O."""
    body = soap_key_value(acct) if risk else [soap_acct(acct)]
    return [soap_in(lid)] + body + [soap_out(lid)]


def ejb_entry(lid, t, name):
    return f"[{lid}] {fmt_ts(t)} INFO  [CommonTiming] The EJB call started for bean Delegation method: {name}"


def ejb_exit(lid, t, name, elapsed):
    return f"[{lid}] {fmt_ts(t)} INFO  [CommonTiming] Total time taken for: {name} - {elapsed} ms"


def _baf(acct):
    return "" if acct is None else f"[baf][x:y:{acct}] "


def ct_start(lid, t, svc, baf=None):
    return f"[{lid}] {fmt_ts(t)} {_baf(baf)}INFO  CommonTiming::Start: {svc} begin"


def ct_stop(lid, t, svc, elapsed, baf=None):
    return f"[{lid}] {fmt_ts(t)} {_baf(baf)}INFO  CommonTiming::Stop: {svc} - total time {elapsed} ms"


def audit_map(lid, t, acct, autr):
    return f"[{lid}] {fmt_ts(t)} [baf][x:{acct}] INFO  auditTrailId={autr}"


def audit_block(lid, t, autr, subs, rules=(None, None, 7)):
    """subs: [(service, start_ms, end_ms, elapsed)]; the RulesEngine entry (start, end, elapsed) goes
    to the db queue (no Provider[ in its name)."""
    r0, r1, rel = rules
    r0 = t if r0 is None else r0
    r1 = r0 + rel if r1 is None else r1
    out = [f"Audit Trail id : {autr}", f"[{lid}] {fmt_ts(t)} INFO  com.acme.Audit: RequestTrace [stopWatchList="]
    out += [f"  {svc}:[{el} millis] ok" for svc, _s, _e, el in subs]
    out += [f"  RulesEngine:[{rel} millis] ok", "]", "<stopWatchList>"]
    for svc, s, e, _el in subs:
        out += [f"  <name>{svc}</name>", f"  <startTime>{fmt_iso(s)}</startTime>", f"  <stopTime>{fmt_iso(e)}</stopTime>"]
    out += ["  <name>RulesEngine</name>", f"  <startTime>{fmt_iso(r0)}</startTime>",
            f"  <stopTime>{fmt_iso(r1)}</stopTime>", "</stopWatchList>"]
    return out


def prov(name):
    return f"Provider[{name}]"


def padded(head, n):
    """A logId of exactly n bytes that starts with `head` (cut when n is shorter)."""
    return (head + _PAD * (n // len(_PAD) + 1))[:n]


# ------------------------------------------------------------------------------- case type

class Batch:
    """One batch under construction: lines appended per (server, file); the chunks come out grouped
    by server in name order (the engine's canonical layout: servers in the order it first saw them,
    and every case names jvm00 first), files in `order` within a server."""

    def __init__(self, now, order=("soap_io.log", "app.log", "server.log")):
        self.now, self.order = now, order
        self.files = collections.OrderedDict()

    def add(self, server, kind, *lines):
        dst = self.files.setdefault((server, kind), [])
        for ln in lines:
            dst.extend(ln if isinstance(ln, list) else [ln])

    def done(self):
        servers = sorted({s for s, _k in self.files})
        chunks = []
        for s in servers:
            for k in self.order:
                if self.files.get((s, k)):
                    chunks.append((path(s, k), self.files[(s, k)]))
        return (self.now, chunks)


class Case:
    def __init__(self, name, batches, facts, save_after=None, plain=True):
        self.name, self.batches, self.facts = name, [b.done() if isinstance(b, Batch) else b for b in batches], facts
        self.save_after = save_after    # checkpoint after this many batches: the most chain state live
        self.plain = plain              # no audit and no non-ASCII lines: the host join never falls back
        nows = [now for now, _c in self.batches]
        assert nows == sorted(nows)

    def n_lines(self):
        return sum(len(ls) for _now, ch in self.batches for _fp, ls in ch)

    def replay(self):
        if not hasattr(self, "_replay"):
            self._replay = replay(self.batches)
        return self._replay


# ------------------------------------------------------------------------------- CPU models

class Replay:
    """The oracle over a case, with what the device join must do for it: records per batch, the
    oracle's counters, the largest number of open partials / parked records per logId, and the
    chain blocks allocated (a map growing from n to n + 1 entries takes a new block when n is at
    least the inline count and a whole number of blocks above it; a new needNumRecordCache entry
    takes ceil((len(logId) - NEED_LID) / LBLK_N) LidBlks)."""

    def __init__(self):
        self.records = []          # [(batch, queue, line)]
        self.max_open = collections.Counter()
        self.max_parked = collections.Counter()
        self.most_parked_drained = 0
        self.blocks = {"chain_partial_blocks": 0, "chain_need_blocks": 0, "chain_logid_blocks": 0}
        self.counters = None

    def batch_lines(self, b, queue=None):
        return [l for bb, q, l in self.records if bb == b and (queue is None or q == queue)]

    def stream(self, queue):
        return [l for _b, q, l in self.records if q == queue]


def _grew(prev, n, inline, per_block):
    return n == prev + 1 and prev >= inline and (prev - inline) % per_block == 0


def replay(batches):
    R = Replay()
    cur = [0]
    po = ParseOracle(lambda q, l: R.records.append((cur[0], q, l)), tz=UTC)
    open_n, need_n = {}, {}
    for b, (now, chunks) in enumerate(batches):
        cur[0] = b
        po.begin_batch(now)
        for fp, lines in chunks:
            for ln in lines:
                out0 = len(R.records)
                po.read_line(fp, ln)
                seen = {}
                for lid, (m, _t) in po.record_cache.data.items():
                    n = len(m)
                    seen[lid] = n
                    if _grew(open_n.get(lid, 0), n, KS_PARTS, PBLK_N):
                        R.blocks["chain_partial_blocks"] += 1
                    R.max_open[lid] = max(R.max_open[lid], n)
                open_n = seen
                seen = {}
                for lid, (m, _t) in po.need_cache.data.items():
                    n = len(m)
                    seen[lid] = n
                    if lid not in need_n:
                        R.blocks["chain_logid_blocks"] += max(0, -(-(len(lid.encode()) - NEED_LID) // LBLK_N))
                    prev = need_n.get(lid, 0)
                    if _grew(prev, n, NEED_ITEMS, NBLK_N):
                        R.blocks["chain_need_blocks"] += 1
                    if n == 0 and prev > 0:
                        R.most_parked_drained = max(R.most_parked_drained, len(R.records) - out0)
                    R.max_parked[lid] = max(R.max_parked[lid], n)
                need_n = seen
    R.counters = dict(po.counters)
    return R


def ops_per_key(batch):
    """{(server, logId bytes): ops} of one batch from the parse model: the timing events carry the
    hash of their logId; an account line counts for the logId of the SOAP block it stands in."""
    now, chunks = batch
    bch = [(KINDS[file_kind(fp)], ("\n".join(ls) + "\n").encode()) for fp, ls in chunks]
    ev, _n, _wm, buf = parse_ref.parse_batch(bch, UTC, {}, list(range(len(chunks))))
    ops = collections.Counter()
    ctx = {}
    for e in ev:
        ci = int(e["chunk"])
        server = chunks[ci][0].split("/")[2]
        kind, mask = int(e["kind"]), int(e["mask"])
        line = buf[int(e["off"]):int(e["off"]) + int(e["len"])]
        if parse_ref.LK_EJB_ENTRY <= kind <= parse_ref.LK_CT_EXIT:
            lid = line.split()[0].strip(b"[]")
            assert int(e["key"]) == parse_ref.hash_bytes(lid)
            ops[(server, lid)] += 1
        elif kind == parse_ref.LK_SOAP:
            if mask & parse_ref.PM_SOAP_IN:
                ctx[ci] = [line.split()[1].split(b"=")[1], False]
            elif mask & parse_ref.PM_SOAP_OUT:
                ctx.pop(ci, None)
            elif ci in ctx:
                if mask & parse_ref.PM_SOAP_KEY:
                    ctx[ci][1] = True
                elif mask & parse_ref.PM_SOAP_ACCT or (mask & parse_ref.PM_SOAP_VALUE and ctx[ci][1]):
                    ops[(server, ctx.pop(ci)[0])] += 1
    return ops


def write_block_totals(lines):
    """Byte totals (line feeds included) of the aligned 64-line blocks of one batch's output."""
    return [sum(len(l.encode()) + 1 for l in lines[j:j + TXW_LINES]) for j in range(0, len(lines), TXW_LINES)]


def block_is_staged(total, p0):
    """k_write's test for a block of `total` bytes that starts at ring offset p0."""
    return total + (p0 & 3) <= TXW_LDS


# ------------------------------------------------------------------------------- the cases

SRV = "jvm00"


def _flush(now, lid_tag):
    """A batch that only moves the clock: one EJB exit without a logId (a direct record)."""
    b = Batch(now)
    b.add(SRV, "server.log", ejb_exit("", now + 1, f"flush{lid_tag}", 3))
    return b


def group_lines(n, lid, t0, acct):
    """{file: [lines]} of a key with exactly n ops.  From three ops on: Start / Stop pairs of three
    services in turn (the same service again with another start), the first half in app.log (no
    account yet: they park, a later Stop of the service replaces the parked value), the account in
    soap_io.log, the second half in server.log (joined at once; every fifth pair is an EJB pair),
    and a Start left open when n is even."""
    out = {"app.log": [], "soap_io.log": [], "server.log": []}
    if n == 1:
        out["app.log"].append(ct_stop(lid, t0, prov("cb-g0"), 11))     # salvaged: an EXIT op of this key
        return out
    if n == 2:
        out["app.log"] += [ct_start(lid, t0, prov("cb-g0")), ct_stop(lid, t0 + 4, prov("cb-g0"), 4)]
        return out
    out["soap_io.log"] += soap_block(lid, acct)
    pairs, extra = (n - 1) // 2, (n - 1) % 2
    for j in range(pairs):
        s, e = t0 + 3 * j, t0 + 3 * j + 2 + j % 2
        if j < pairs // 2:
            out["app.log"] += [ct_start(lid, s, prov(f"cb-g{j % 3}")), ct_stop(lid, e, prov(f"cb-g{j % 3}"), e - s)]
        elif j % 5 == 4:
            out["server.log"] += [ejb_entry(lid, s, f"getG{j % 3}"), ejb_exit(lid, e, f"getG{j % 3}", e - s)]
        else:
            out["server.log"] += [ct_start(lid, s, prov(f"cb-g{j % 3}")), ct_stop(lid, e, prov(f"cb-g{j % 3}"), e - s)]
    if extra:
        out["server.log"].append(ct_start(lid, t0 + 3 * pairs, prov("cb-open")))
    return out


def _interleave(per_key, rng):
    """One file's lines: every key's lines in their own order, the keys mixed."""
    iters = [list(v) for v in per_key if v]
    at = [0] * len(iters)
    out = []
    live = list(range(len(iters)))
    while live:
        k = rng.choice(live)
        out.append(iters[k][at[k]])
        at[k] += 1
        if at[k] == len(iters[k]):
            live.remove(k)
    return out


def _group_case(name, sizes, seed):
    rng = random.Random(seed)
    b = Batch(START, order=("app.log", "soap_io.log", "server.log"))
    keys = {}
    per_file = collections.defaultdict(list)
    soap = []
    for i, n in enumerate(sizes):
        lid = f"GS-{n:04d}-{i}"
        keys[lid] = n
        kl = group_lines(n, lid, START + 10 + i, 300000000000000 + n)
        for f in ("app.log", "server.log"):
            per_file[f].append(kl[f])
        soap.append(kl["soap_io.log"])
    for f in ("app.log", "server.log"):
        b.add(SRV, f, _interleave(per_file[f], rng))
    order = list(range(len(soap)))
    rng.shuffle(order)
    for k in order:  # (a SOAP block stays whole: the account belongs to the IO=I before it)
        b.add(SRV, "soap_io.log", soap[k])
    return Case(name, [b, _flush(START + NEED_TTL + 1, "G")], {"ops": keys})


def case_group_sizes():
    return _group_case("group_sizes", GROUP_SIZES, 41)


def case_open_partials():
    b1, b2, b3 = Batch(START), Batch(START + 5000), Batch(START + 9000)
    rng = random.Random(7)
    keys = {}
    for i, c in enumerate(OPEN_COUNTS):
        lid = f"OP-{c:02d}"
        keys[lid] = c
        t0 = START + 100 * i
        b1.add(SRV, "soap_io.log", soap_block(lid, 400000000000000 + c, risk=bool(i % 2)))
        for k in range(c):
            b1.add(SRV, "app.log", ct_start(lid, t0 + k, prov(f"cb-o{k:02d}")))
        # Map.set on an open service: the start is replaced, the count stays
        for k in sorted({1 % c, c - 1}):
            b1.add(SRV, "app.log", ct_start(lid, t0 + 50 + k, prov(f"cb-o{k:02d}")))
        # closes after the batch boundary: first, middle, last, then the rest mixed, down to none
        rest = [k for k in range(c) if k not in (0, c // 2, c - 1)]
        rng.shuffle(rest)
        for j, k in enumerate([0, c // 2, c - 1] + rest):
            b2.add(SRV, "app.log", ct_stop(lid, START + 5000 + 100 * i + j, prov(f"cb-o{k:02d}"), 5000 + j))
    # the emptied key grows a first chain block again and gives it back
    lid = f"OP-{OPEN_COUNTS[-1]:02d}"
    for k in range(KS_PARTS + 1):
        b3.add(SRV, "app.log", ct_start(lid, START + 9000 + k, prov(f"cb-o{k:02d}")))
    for k in range(KS_PARTS + 1):
        b3.add(SRV, "app.log", ct_stop(lid, START + 9100 + k, prov(f"cb-o{k:02d}"), 100))
    return Case("open_partials", [b1, b2, b3], {"open": keys}, save_after=1)


def case_parked_records():
    N = START
    b1, b2 = Batch(N), Batch(N + 10000)
    keys = {}
    for w, way in enumerate(DRAIN_WAYS):
        for i, c in enumerate(PARKED_COUNTS):
            lid = f"PK-{way}-{c:02d}"
            keys[lid] = c
            t0 = N + 1000 * w + 50 * i
            for j, k in enumerate(list(range(c)) + sorted({0, c - 1})):  # the first and the last service park twice
                again = 20 if j >= c else 0
                b1.add(SRV, "app.log", ct_start(lid, t0 + k + again, prov(f"cb-p{k:02d}")))
                b1.add(SRV, "app.log", ct_stop(lid, t0 + k + 30, prov(f"cb-p{k:02d}"), 30 - again))
            t1 = N + 10000 + 1000 * w + 50 * i
            if way == "soap":
                b2.add(SRV, "soap_io.log", soap_block(lid, 500000000000000 + c))
            elif way == "baf" and c % 2 == 0:
                # matched Stop with a valid BAF account: drains, then parks itself on the drained entry
                # (still live: it keeps the expiry of batch 1)
                b2.add(SRV, "app.log", ct_start(lid, t1, prov("cb-late")))
                b2.add(SRV, "app.log", ct_stop(lid, t1 + 9, prov("cb-late"), 9, baf=600000000000000 + c))
            elif way == "baf":
                # salvaged Stop (no open partial) with a valid BAF account: drains as well
                b2.add(SRV, "app.log", ct_stop(lid, t1 + 9, prov("cb-late"), 9, baf=600000000000000 + c))
    return Case("parked_records", [b1, b2, _flush(N + NEED_TTL + 1, "P"), _flush(N + 45000, "Q")],
                {"parked": keys}, save_after=1)


def logid_of(way, n):
    return padded(way if n == 1 else f"{way}{n}-", n)


def case_logid_lengths():
    N = START
    b1, b2 = Batch(N), Batch(N + 10000)
    keys = {}
    for w, way in enumerate("AE"):  # A: an account in a later batch, E: expiry
        for i, n in enumerate(LOGID_LENGTHS):
            lid = logid_of(way, n)
            assert len(lid) == n and lid not in keys
            keys[lid] = n
            t0 = N + 500 * w + 20 * i
            for k in range(2):
                b1.add(SRV, "app.log", ct_start(lid, t0 + k, prov(f"cb-l{k}")))
                b1.add(SRV, "app.log", ct_stop(lid, t0 + 10 + k, prov(f"cb-l{k}"), 10))
            if way == "A":
                b2.add(SRV, "soap_io.log", soap_block(lid, 700000000000000 + n))
    return Case("logid_lengths", [b1, b2, _flush(N + NEED_TTL + 1, "L"), _flush(N + 45000, "M")],
                {"logids": keys}, save_after=1)


def case_ttl_edges():
    N = START
    M = N + 200000
    B = collections.OrderedDict((t, Batch(t)) for t in (
        N, N + 20000, N + 30000, N + 30001, N + 60000, N + 120000, N + 120001, N + 150000,
        M, M + 1000, M + 2000, M + 40000))
    svc = prov("cb-t0")

    def pair(t, lid, s=svc, el=5, file="app.log"):
        B[t].add(SRV, file, ct_start(lid, t + 1, s), ct_stop(lid, t + 1 + el, s, el))

    def acct(t, lid, a):
        B[t].add(SRV, "soap_io.log", soap_block(lid, a))

    # the account cache: set at N, an exit at N + 120000 is joined, at N + 120001 it parks
    acct(N, "TT-AJ", 811111111111111); acct(N, "TT-AP", 822222222222222)
    pair(N + 120000, "TT-AJ"); pair(N + 120001, "TT-AP")
    # the record cache: opened at N, the exit at N + 120000 matches (its account arrives just before,
    # soap_io.log leads the batch), at N + 120001 the partial is gone: a Stop is salvaged without a
    # logId, an EJB exit is counted unmatched
    B[N].add(SRV, "app.log", ct_start("TT-PM", N + 2, svc), ct_start("TT-PD", N + 3, svc))
    B[N].add(SRV, "server.log", ejb_entry("TT-PE", N + 4, "getT0"))
    acct(N + 120000, "TT-PM", 833333333333333)
    B[N + 120000].add(SRV, "app.log", ct_stop("TT-PM", N + 120002, svc, 120000))
    B[N + 120001].add(SRV, "app.log", ct_stop("TT-PD", N + 120003, svc, 120000))
    B[N + 120001].add(SRV, "server.log", ejb_exit("TT-PE", N + 120004, "getT0", 120000))
    # the need cache: parked at N, an account at N + 30000 drains it, at N + 30001 it has expired
    pair(N, "TT-ND"); pair(N, "TT-NX")
    acct(N + 30000, "TT-ND", 844444444444444); acct(N + 30001, "TT-NX", 855555555555555)
    # an account set again is refreshed: set at N and N + 60000, joined at N + 150000
    acct(N, "TT-AR", 866666666666666); acct(N + 60000, "TT-AR", 866666666666667)
    pair(N + 150000, "TT-AR")
    # a record entry touched again is not: opened at N, another service at N + 60000, both gone at
    # N + 120001
    B[N].add(SRV, "app.log", ct_start("TT-RR", N + 5, svc))
    B[N + 60000].add(SRV, "app.log", ct_start("TT-RR", N + 60005, prov("cb-t1")))
    B[N + 120001].add(SRV, "app.log", ct_stop("TT-RR", N + 120005, prov("cb-t1"), 60000))
    # nor is a need entry: parked at N, another service at N + 20000, both expire at N + 30001
    pair(N, "TT-NR"); pair(N + 20000, "TT-NR", prov("cb-t1"))
    # one sweep (M + 40000) over need entries of three batches: creation order, whatever the keys,
    # the line numbers or a later touch say
    pair(M, "TT-Cz"); pair(M, "TT-Ca")
    pair(M + 1000, "TT-Cm")
    pair(M + 2000, "TT-Cb", file="server.log"); pair(M + 2000, "TT-Cz", prov("cb-t2"), file="server.log")
    for t in (N + 30000, N + 30001, M, M + 40000):
        B[t].add(SRV, "server.log", ejb_exit("", t + 9, "flushT", 3))
    return Case("ttl_edges", list(B.values()), {
        "joined": ["TT-AJ", "TT-PM", "TT-AR"], "expired_partials": 4, "ejb_exit_unmatched": 1,
        "sweep_order": ["TT-Cz", "TT-Cz", "TT-Ca", "TT-Cm", "TT-Cb"]})


def case_keys():
    N = START
    b1, b2, b3 = Batch(N), Batch(N + 5000), _flush(N + 5000 + NEED_TTL + 1, "K")
    svc = prov("cb-k0")
    # one logId on two servers, each with its own account and partials.  (The reference keys its
    # caches by logId alone while the join keys them by logId and server: each server's use is
    # complete -- account set, partial closed, nothing parked -- before the other's begins, where
    # both readings agree.)
    for s, a in (("jvm00", 911111111111111), ("jvm01", 922222222222222)):
        b1.add(s, "soap_io.log", soap_block("KY-DUP", a))
        b1.add(s, "app.log", ct_start("KY-DUP", N + 1, svc), ct_stop("KY-DUP", N + 8, svc, 7))
    b2.add("jvm01", "app.log", ct_start("KY-DUP", N + 5001, svc), ct_stop("KY-DUP", N + 5009, svc, 8))
    # one logId in two files of one server: opened in app.log, closed in server.log
    b1.add(SRV, "soap_io.log", soap_block("KY-SH", 933333333333333, risk=True))
    b1.add(SRV, "app.log", ct_start("KY-SH", N + 20, svc))
    b1.add(SRV, "server.log", ct_stop("KY-SH", N + 29, svc, 9))
    # the empty logId: an entry is dropped, an EJB exit and a Stop are output directly
    b1.add(SRV, "server.log", ejb_entry("", N + 30, "getK0"), ejb_exit("", N + 35, "getK0", 5))
    b1.add(SRV, "app.log", ct_start("", N + 31, svc), ct_stop("", N + 36, svc, 5),
           ct_stop("", N + 37, svc, 6, baf=944444444444444))
    # IO=I without '=': the logId is undefined
    b1.add(SRV, "soap_io.log", "=== jbossId IO=I", soap_acct(955555555555555), "=== jbossId IO=O")
    b1.add(SRV, "app.log", ct_start("undefined", N + 40, svc), ct_stop("undefined", N + 44, svc, 4))
    # accounts of 15, 16 and 17 digits and with leading zeros
    accts = ["123456789012345", "1234567890123456", "9999999999999999", "12345678901234567", "000012345678901",
             "0000000000000000"]
    for i, a in enumerate(accts):
        lid = f"KY-AC{i}"
        b1.add(SRV, "soap_io.log", soap_block(lid, a, risk=i % 2 == 1))
        b1.add(SRV, "app.log", ct_start(lid, N + 50 + i, svc), ct_stop(lid, N + 60 + i, svc, 10))
    # BAF accounts: on a salvaged Stop (saved for the logId: the pair after it is joined) and on a
    # matched Stop
    b2.add(SRV, "app.log", ct_stop("KY-BS", N + 5020, svc, 20, baf=966666666666666),
           ct_start("KY-BS", N + 5021, svc), ct_stop("KY-BS", N + 5025, svc, 4))
    b2.add(SRV, "app.log", ct_start("KY-BV", N + 5040, svc), ct_stop("KY-BV", N + 5044, svc, 4, baf="0000977777"))
    # an audit trail: the map line's BAF account is saved for the logId, the block's Provider
    # entries are joined with it, its RulesEngine entry goes to the db queue; a second trail without
    # an account parks (db flag kept) and expires
    for lid, a, autr, t in (("KY-AU1", "988888888888888", "AUTR0001", N + 5100), ("KY-AU2", "", "AUTR0002", N + 5200)):
        b2.add(SRV, "app.log", audit_map(lid, t, a, autr))
        b2.add(SRV, "app.log", audit_block(lid, t + 50, autr, [(prov("cb-k1"), t + 1, t + 21, 20),
                                                               (prov("cb-k2"), t + 22, t + 40, 18)]))
    return Case("keys", [b1, b2, b3], {"invalid_acct": 0}, plain=False)


def case_keys_invalid():
    """Accounts that are not all digits: counted, never saved.  (A case of its own: the reference
    throws on them through a misspelt variable in its error message and leaves the line half done,
    which the oracle and the join do not copy -- so this case has no recorded reference answer.)"""
    N = START
    b1, b2 = Batch(N), _flush(N + NEED_TTL + 1, "I")
    svc = prov("cb-k0")
    for i, a in enumerate(["12345678X", " 12 34 ", "-5"]):
        lid = f"KI-AC{i}"
        b1.add(SRV, "soap_io.log", soap_block(lid, a, risk=i == 1))
        b1.add(SRV, "app.log", ct_start(lid, N + 50 + i, svc), ct_stop(lid, N + 60 + i, svc, 10))
    # on a matched Stop (the record parks with the text as its alternative account), on a salvaged one
    b1.add(SRV, "app.log", ct_start("KI-BI", N + 30, svc), ct_stop("KI-BI", N + 34, svc, 4, baf="97X"))
    b1.add(SRV, "app.log", ct_stop("KI-BS", N + 40, svc, 4, baf="98X"))
    return Case("keys_invalid", [b1, b2], {"invalid_acct": 5})


_W = {}


def _write_case(lens_b):
    """Batch 0 parks five records, batch 1 (at their expiry) emits them first, then 59 short filler
    transactions, then one 64-line group per total: 63 joined records of one logId and one of a
    second logId whose length (lens_b[g]) sets the group's byte total."""
    N = START
    b0, b1 = Batch(N), Batch(N + NEED_TTL + 1)
    for k in range(5):
        b0.add(SRV, "app.log", ct_start("WB-X", N + k, prov(f"cb-w{k}")), ct_stop("WB-X", N + 9 + k, prov(f"cb-w{k}"), 9))
    T = N + NEED_TTL + 1
    b1.add(SRV, "soap_io.log", soap_block("WB-F", 100000000000001))
    for k in range(TXW_LINES - 5):
        b1.add(SRV, "app.log", ct_start("WB-F", T + k, prov("cb-w0")), ct_stop("WB-F", T + k + 1, prov("cb-w0"), 1))
    for g, nb in enumerate(lens_b):
        la, lb = padded(f"WB-{g}a-", 54), padded(f"WB-{g}b-", nb)
        t0 = T + 1000 * (g + 1)
        b1.add(SRV, "soap_io.log", soap_block(la, 100000000000010 + g), soap_block(lb, 100000000000020 + g))
        for k in range(TXW_LINES - 1):
            b1.add(SRV, "app.log", ct_start(la, t0 + k, prov("cb-w1")), ct_stop(la, t0 + k + 2, prov("cb-w1"), 2))
        b1.add(SRV, "app.log", ct_start(lb, t0 + 100, prov("cb-w1")), ct_stop(lb, t0 + 102, prov("cb-w1"), 2))
    return Case("write_blocks", [b0, b1], {"totals": WRITE_TOTALS})


def case_write_blocks():
    if "case" not in _W:
        base = 120
        first = _write_case([base] * len(WRITE_TOTALS))
        got = write_block_totals(first.replay().batch_lines(1))
        assert len(got) == 1 + len(WRITE_TOTALS)
        # a line's length is its logId's length plus a constant: move the one line per group
        lens_b = [base + want - have for want, have in zip(WRITE_TOTALS, got[1:])]
        assert min(lens_b) > 10
        _W["case"] = _write_case(lens_b)
    return _W["case"]


_CASES = collections.OrderedDict([
    ("group_sizes", case_group_sizes), ("open_partials", case_open_partials),
    ("parked_records", case_parked_records), ("logid_lengths", case_logid_lengths),
    ("ttl_edges", case_ttl_edges), ("keys", case_keys), ("keys_invalid", case_keys_invalid),
    ("write_blocks", case_write_blocks)])
CASE_NAMES = list(_CASES)
REFERENCE_CASES = [n for n in CASE_NAMES if n != "keys_invalid"]   # (see case_keys_invalid)
SAVE_CASES = ["open_partials", "parked_records", "logid_lengths"]
_BUILT = {}


def get_case(name):
    if name not in _BUILT:
        _BUILT[name] = _CASES[name]()
    return _BUILT[name]


# ------------------------------------------------------------------------------- tier proofs

def _brackets(values, edge):
    """edge - 1, edge and edge + 1 are all among `values`."""
    return {edge - 1, edge, edge + 1} <= set(values)


def prove(case):
    """Asserts, from the CPU models alone, that `case` reaches the tiers it claims.  Returns the
    tiers by name."""
    R = case.replay()
    f = case.facts
    tiers = {}
    assert case.n_lines() > 0 and R.records, case.name
    if "ops" in f:
        ops = ops_per_key(case.batches[0])
        for lid, n in f["ops"].items():
            assert ops[(SRV, lid.encode())] == n, (lid, ops[(SRV, lid.encode())])
        assert sorted(ops.values()) == sorted(f["ops"].values())
        ns = list(f["ops"].values())
        tiers["k_group_walk (registers)"] = [n for n in ns if n <= GW_SMALL]
        tiers["k_group_walk_big, LDS sort"] = [n for n in ns if GW_SMALL < n <= GWB_LDS]
        tiers["k_group_walk_big, global sort"] = [n for n in ns if n > GWB_LDS]
        assert all(tiers.values())
        if case.name == "group_sizes":
            assert _brackets(ns, GW_SMALL) and _brackets(ns, GWB_LDS) and _brackets(ns, 2 * GW_SMALL)
            assert {1, 2} <= set(ns)
        # order-sensitive: parked records were replaced and drained three at a time
        assert R.most_parked_drained > EMITTER_STAGED
    if "open" in f:
        for lid, c in f["open"].items():
            assert R.max_open[lid] == c, (lid, R.max_open[lid])
        cs = list(f["open"].values())
        assert _brackets(cs, KS_PARTS) and _brackets(cs, KS_PARTS + PBLK_N)
        assert {KS_PARTS + 2 * PBLK_N, KS_PARTS + 2 * PBLK_N + 1} <= set(cs)
        tiers["inline partials"] = [c for c in cs if c <= KS_PARTS]
        tiers["PartBlk chain"] = [c for c in cs if c > KS_PARTS]
        # closed form: a key that reaches c open partials took ceil((c - KS_PARTS) / PBLK_N) blocks,
        # and the last key takes its first block once more in batch 3
        want = sum(-(-(c - KS_PARTS) // PBLK_N) for c in cs if c > KS_PARTS) + 1
        assert R.blocks["chain_partial_blocks"] == want, (R.blocks, want)
        assert R.counters["expired_partials"] == 0
    if "parked" in f:
        for lid, c in f["parked"].items():
            assert R.max_parked[lid] == c, (lid, R.max_parked[lid])
        cs = PARKED_COUNTS
        assert sorted(set(f["parked"].values())) == cs
        assert _brackets(cs, EMITTER_STAGED) and _brackets(cs, NEED_ITEMS) and _brackets(cs, NEED_ITEMS + NBLK_N)
        assert max(cs) > NEED_ITEMS + 2 * NBLK_N
        tiers["inline parked records"] = [c for c in cs if c <= NEED_ITEMS]
        tiers["NeedBlk chain"] = [c for c in cs if c > NEED_ITEMS]
        want = len(DRAIN_WAYS) * sum(-(-(c - NEED_ITEMS) // NBLK_N) for c in cs if c > NEED_ITEMS)
        assert R.blocks["chain_need_blocks"] == want, (R.blocks, want)
        assert R.most_parked_drained == max(cs) > EMITTER_STAGED
        # the ttl keys and the records re-parked by a matched BAF Stop expire with batch 1's clock
        n_ttl = sum(cs) + sum(1 for c in cs if c % 2 == 0)
        assert R.counters["need_expired"] == n_ttl == len(R.batch_lines(2)) - 1, (R.counters, n_ttl)
        assert len(R.batch_lines(3)) == 1
    if "logids" in f:
        ns = LOGID_LENGTHS
        assert sorted(set(f["logids"].values())) == ns
        assert _brackets(ns, NEED_LID) and _brackets(ns, NEED_LID + LBLK_N) and {NEED_LID + 2 * LBLK_N, NEED_LID + 2 * LBLK_N + 1} <= set(ns)
        tiers["inline logId"] = [n for n in ns if n <= NEED_LID]
        tiers["LidBlk chain"] = [n for n in ns if n > NEED_LID]
        want = 2 * sum(-(-(n - NEED_LID) // LBLK_N) for n in ns if n > NEED_LID)
        assert R.blocks["chain_logid_blocks"] == want, (R.blocks, want)
        for b in (1, 2):  # every length is printed from the need entry by an account and by expiry
            assert sorted(len(l.split("|")[3]) for l in R.batch_lines(b) if l.split("|")[3]) == sorted(ns * 2)
    if "sweep_order" in f:
        last = [l.split("|")[3] for l in R.batch_lines(len(case.batches) - 1)]
        assert last[:len(f["sweep_order"])] == f["sweep_order"], last
        tx = R.stream("transactions")
        for lid in f["joined"]:
            assert any(l.split("|")[3] == lid and l.split("|")[4] not in ("", "NaN", "undefined") for l in tx), lid
        assert R.counters["expired_partials"] == f["expired_partials"]
        assert R.counters["ejb_exit_unmatched"] == f["ejb_exit_unmatched"]
        by = {l.split("|")[3]: l.split("|")[4] for l in tx if l.split("|")[3]}
        assert by["TT-AP"] == "NaN" and by["TT-NX"] == "NaN" and by["TT-ND"] == "844444444444444"
        tiers["strict expiry"] = ["exp == now live", "exp + 1 expired"]
    if "invalid_acct" in f:
        assert R.counters["invalid_acct"] == f["invalid_acct"]
        assert R.stream("db_insert") or case.name != "keys"
        tiers["keys"] = ["two servers", "two files", "empty logId", "undefined logId", "accounts", "audit"]
    if "totals" in f:
        got = write_block_totals(R.batch_lines(1))
        assert got[1:] == f["totals"], got
        assert len(R.batch_lines(1)) == TXW_LINES * (1 + len(f["totals"]))
        assert [l.split("|")[3] for l in R.batch_lines(1)[:5]] == ["WB-X"] * 5   # expiry outputs first
        for r in range(4):  # whatever the start offset modulo 4, a staged group has an unstaged neighbour
            st = [block_is_staged(t, r) for t in f["totals"]]
            assert st[0] and not st[-1] and any(a and not b for a, b in zip(st, st[1:])), (r, st)
        tiers["k_write staged / direct"] = f["totals"]
    return tiers

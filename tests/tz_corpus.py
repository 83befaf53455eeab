"""Synthetic traffic across a time-zone transition, for tests/test_tz_table.py (host join) and
tests/test_parse_tz_gpu.py (whole pipeline): the generator's three log kinds with every stamp
written in the zone's local time, plus one app.log of audit trails whose <startTime> / <stopTime>
come with an offset, with 'Z' and without a zone, some on lines the device hands to the host
(non-ASCII names and elapsed values)."""
import dataclasses
import random

from apmbackend_amd.utils.synth import Generator, SynthConfig, batches, fmt_ts, with_watermarks

AUDIT_LOG = "/net/jvm90/export/jvm1/log/app.log"


def _iso(ms, form, tz):
    """form 0: UTC with 'Z'; 1: -06:00; 2: local time of the zone, no offset."""
    if form == 0:
        return fmt_ts(ms, 0).replace(" ", "T").replace(",", ".") + "Z"
    if form == 1:
        return fmt_ts(ms, -6 * 3600000).replace(" ", "T").replace(",", ".") + "-06:00"
    return fmt_ts(ms, tz=tz).replace(" ", "T").replace(",", ".")


def audit_lines(tz, start_ms, seconds, seed):
    """[(ts, seq, line)] of audit trails: a map line, then (now or a few requests later) the
    block with its elapsed section and stop-watch list."""
    rng = random.Random(seed)
    out, pending = [], []
    t, r = start_ms, 0
    while True:
        t += rng.randint(50, 600)
        if t >= start_ms + seconds * 1000:
            break
        r += 1
        lid = f"T{seed}{r:05d}" + ("é" if r % 29 == 0 else "")
        autr = f"A{r:05d}"
        acct = ("12345", "999", "007")[r % 3]
        out.append((t, len(out), f"[{lid}] {fmt_ts(t, tz=tz)} [baf][x:{acct}] INFO  auditTrailId={autr}"))
        svcs = [("Provider[cb-a]", "Provider[cb-b]", "RulesEngine", "Lookup", "Provider[cb-é]")[rng.randrange(5)]
                for _ in range(rng.randint(1, 4))]
        pending.append((autr, lid, svcs, t))
        while pending and (rng.random() < 0.5 or len(pending) > 4):
            a, l, sv, t0 = pending.pop(rng.randrange(len(pending)))
            block = [f"Audit Trail id : {a}",
                     f"[{l}] {fmt_ts(t, tz=tz)} INFO  com.acme.Audit: RequestTrace [stopWatchList="]
            for s in sv:
                block.append(f"  {s}:[{rng.choice([str(rng.randint(0, 900)), '12é'])} millis] ok")
            block += ["]", "<stopWatchList>"]
            for s in sv:
                block += [f"  <name>{s}</name>", f"  <startTime>{_iso(t0 + 1, rng.randrange(3), tz)}</startTime>",
                          f"  <stopTime>{_iso(t0 + rng.randint(2, 300), rng.randrange(3), tz)}</stopTime>"]
            block.append("</stopWatchList>")
            out += [(t, len(out) + i, ln) for i, ln in enumerate(block)]
    return out


def transition_corpus(tz, start_ms, seconds, seed, batch_s=5.0):
    """(lines per file, [(now, [(path, lines)])]) of 2 servers' traffic plus the audit log, from
    start_ms on, stamped in ``tz``; ``now`` is the engine's watermark clock in that zone."""
    cfg = SynthConfig(servers=2, duration_s=seconds, tx_per_sec_per_server=3, seed=seed, start_ms=start_ms,
                      ejb_services=4, provider_services=3, audit_fraction=0.2, tz=tz)
    lines = Generator(cfg).generate()
    lines[AUDIT_LOG] = audit_lines(tz, start_ms, seconds, seed)
    bl = batches(lines, start_ms, batch_s)
    # a few seconds of traffic two hours on (past the repeated hour, so its stamps are later for
    # every reader): the stats stage rolls over once more and releases all the tx from before,
    # which it otherwise holds back for ever where the log's clock has stepped back an hour
    late = dataclasses.replace(cfg, start_ms=start_ms + seconds * 1000 + 2 * 3600000, duration_s=3, seed=seed + 1)
    more = Generator(late).generate()
    bl += batches(more, late.start_ms, batch_s)
    for fp, ls in more.items():
        lines[fp] = lines.get(fp, []) + ls
    return lines, with_watermarks(bl, tz)

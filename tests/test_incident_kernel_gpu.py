"""K25's kernels alone (incident.hip: k_incident_step, k_text_len<IcRow>, k_incident_write) through
the incident_kernels test hook, against tests/incident_ref.py: plain int32 verdict arrays with
stride 4, a capacity of 160 slots of which 130 are series -- two full waves and a two-lane tail --
and 40 rollovers of seeded hot, clear and absent patterns.  After every rollover the state, the
event bytes, the open counters and the text are compared; slots 130 .. 159 keep the pattern written
before the first launch.  (After the manner of tests/test_topk_kernel_gpu.py.)

Names: a server name comes from a file name and a service name from one log token; the name table
stores lengths as int32 and sets no bound of its own, so the longest length a file system lets a
name component have, 255 bytes, stands for "the longest"."""
import random
import struct

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

from apmbackend_amd import _native  # noqa: E402

import incident_ref as R  # noqa: E402

CAP, N_SERIES, ROLLOVERS = 160, 130, 40
T0 = 1578391200000
OPEN = {"sb": 2, "tf": 3, "po": 6, "ls": 2}
CLOSE = {"sb": 6, "tf": 4, "po": 3, "ls": 5}
REMIND = 4
# verdict words: sb any set bit; tf / ls two bits a rule (1 = D / U, 2 = S / D); po 1 = H, 2 = L
WORDS = {"sb": (1, 2, 5, 15), "tf": (1, 2, 4, 8, 0x24, 0x90), "po": (1, 2), "ls": (1, 2, 4, 8, 0x18, 0x60)}
GUARD = bytes(range(1, 65))           # the pattern of an untouched state slot (four states)
GUARD_EV = b"\xa5\x5a\xc3\x3c"


def patterns(rng):
    """hot[src][s]: per rollover the verdict word (0 = clear); act[s]: per rollover the st flag.  The
    first series carry the named boundary cases, the others are seeded."""
    hot = {src: [[0] * ROLLOVERS for _ in range(CAP)] for src in R.SOURCES}
    act = [[1] * ROLLOVERS for _ in range(CAP)]
    for src in R.SOURCES:
        oa, ca = OPEN[src], CLOSE[src]
        w = WORDS[src]
        h = hot[src]
        for t in range(oa):
            h[0][t] = w[0]                       # opens exactly at openAfter ...
        for t in range(oa - 1):
            h[1][t] = w[0]                       # ... one rollover short of it: never opens
        for t in range(oa):
            h[2][t] = w[0]                       # open, then clear for closeAfter: closes exactly there
        for t in range(oa):
            h[3][t] = w[0]
        for t in range(oa + ca - 1, ROLLOVERS):
            h[3][t] = w[0]                       # clear one rollover short of closeAfter, then hot again: stays open
        for t in range(30):
            h[4][t] = w[0] if t < oa + 2 else w[1]   # the code flips inside an open incident
        for t in range(ROLLOVERS):
            h[5][t] = w[0]                       # open to the end: reminder steps every REMIND rollovers
        for t in range(ROLLOVERS):
            h[6][t] = w[0]                       # opens, then the series goes absent: closes by absence
            if t >= oa + 1:
                act[6][t] = 0
        for s in range(7, CAP):
            on = False
            for t in range(ROLLOVERS):
                if rng.random() < 0.25:
                    on = rng.random() < 0.5
                h[s][t] = rng.choice(w) if on else 0
    for s in range(7, CAP):
        if s % 9 == 0:
            for t in range(ROLLOVERS):
                if rng.random() < 0.2:
                    act[s][t] = 0
    return hot, act


def names_table(rng, long_at):
    """(names bytes, [(server off, len, service off, len)] per slot, [(server, service)]): 1-byte names
    for the first series, 255-byte ones at `long_at`, seeded lengths elsewhere."""
    blob, table, text = b"", [], []
    for s in range(CAP):
        if s < 3:
            a, b = chr(ord("a") + s), chr(ord("x") + s % 3)
        elif s in long_at:
            a = "".join(rng.choice("abcdefghij0123456789") for _ in range(255))
            b = "".join(rng.choice("KLMNOPQRS:_-") for _ in range(255))
        else:
            a = f"jvm{s:03d}" + "q" * rng.randrange(0, 9)
            b = f"S:svc{s % 11}" + "z" * rng.randrange(0, 17)
        table.append((len(blob), len(a), len(blob) + len(a), len(b)))
        blob += a.encode() + b.encode()
        text.append((a, b))
    return blob, table, text


def unpack_state(raw, s, k):
    since, age, code0, hr, cr, pad = struct.unpack_from("<qIBBBB", raw, (s * 4 + k) * 16)
    return {"code0": chr(code0) if code0 else "", "since": since, "age": age, "hot_run": hr, "clear_run": cr}, pad


def run_case(sources, seed):
    N = _native.load(build_if_missing=False)
    rng = random.Random(seed)
    hot, act = patterns(rng)
    blob, table, text = names_table(rng, long_at={3, 64, 129})
    perm = list(range(N_SERIES))
    rng.shuffle(perm)
    book = R.Book({src: (OPEN[src], CLOSE[src]) for src in sources}, REMIND)
    state = bytes(CAP * 64)[:N_SERIES * 64] + GUARD * (CAP - N_SERIES)
    ev = bytes(N_SERIES * 4) + GUARD_EV * (CAP - N_SERIES)
    oa = [OPEN[src] if src in sources else 0 for src in R.SOURCES]
    ca = [CLOSE[src] if src in sources else 0 for src in R.SOURCES]
    seen = set()
    for t in range(ROLLOVERS):
        ts = T0 + 10000 * t
        words = [[hot[src][s][t] for s in range(CAP)] if src in sources else None for src in R.SOURCES]
        active = bytes(act[s][t] for s in range(CAP))
        state, ev, opens, out = N.incident_kernels(state, ev, words, active, N_SERIES, oa, ca, REMIND, ts, perm, table, blob)
        series = []
        for s in perm:
            codes = {src: R.code_of(src, hot[src][s][t]) for src in sources} if act[s][t] else {}
            series.append((s, text[s][0], text[s][1], codes))
        want_rows = book.step_all(ts, series)
        # the text, byte for byte
        assert out.decode("utf-8") == "".join(r + "\n" for r in want_rows), t
        # the state and the event bytes of every series, the counters
        events = {}
        for r in want_rows:
            f = r.split("|")
            events[(f[2], f[3], f[4])] = f[5]
            seen.add((f[4], f[5]))
        for s in range(N_SERIES):
            for k, src in enumerate(R.SOURCES):
                got, pad = unpack_state(state, s, k)
                if src in sources:
                    assert got == book.states[(s, src)] and pad == 0, (t, s, src)
                    got_ev = chr(ev[s * 4 + k]) if ev[s * 4 + k] else ""
                    assert got_ev == events.get((text[s][0], text[s][1], src), ""), (t, s, src)
                else:
                    assert got == R.new_state() and ev[s * 4 + k] == 0
        assert list(opens) == [book.open_count(src) if src in sources else 0 for src in R.SOURCES], t
        # series ids at or above n_series are not touched
        assert state[N_SERIES * 64:] == GUARD * (CAP - N_SERIES) and ev[N_SERIES * 4:] == GUARD_EV * (CAP - N_SERIES)
    return book, seen


def test_all_sources_against_the_reference():
    book, seen = run_case(R.SOURCES, seed=25)
    for src in R.SOURCES:
        oa, ca = OPEN[src], CLOSE[src]
        st = book.states
        assert st[(1, src)]["code0"] == "" and st[(1, src)]["age"] == 0        # one short of openAfter: never opened
        assert st[(2, src)]["code0"] == "" and st[(2, src)]["age"] == ca       # closed exactly at closeAfter
        assert st[(3, src)]["code0"] != ""                                     # one short of closeAfter: still open
        assert st[(5, src)]["code0"] != "" and st[(5, src)]["age"] == ROLLOVERS - oa
        assert st[(6, src)]["code0"] == ""                                     # closed by absence
        assert {(src, "O"), (src, "S"), (src, "C")} <= seen


def test_one_source_only():
    book, seen = run_case(("tf",), seed=26)
    assert {e for _s, e in seen} == {"O", "S", "C"} and {s for s, _e in seen} == {"tf"}

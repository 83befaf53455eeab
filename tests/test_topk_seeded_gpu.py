"""K18 tk rows (topk.hip) on seeded engine state: one engine, one rollover (tests/seeded.py).  The
engine's rows must equal the CPU oracle's and a reference that shares no code with either
(tests/topk_ref.py, from the st rows), byte for byte, and leaderboard() the reference's series."""
import copy
import random

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import seeded as S  # noqa: E402
import topk_ref as R  # noqa: E402

NAN = S.ELAPSED_NAN
OTHER = "jvm01"
K = 14
BY = ["per95", "tpm", "average", "per75"]
MIN_TPM = 2.0          # 31 buckets of 10 s: tpm = n / 5.1666..., so series of up to 10 samples are cut


class TopSeeded(S.Seeded):
    """Seeded with the tk stream on, on both sides."""

    def __init__(self, C, *a, board, **kw):
        self.tk = []
        C = copy.deepcopy(C)
        C["gpu"]["leaderboard"] = copy.deepcopy(board)
        super().__init__(C, *a, **kw)

    def _seed_oracle(self):
        from apmbackend_amd.utils.config import leaderboard
        super()._seed_oracle()
        self.so.emit_top = self.tk.append
        self.so.board = leaderboard(self.C)

    def _seed_engine(self):
        from apmbackend_amd.models import pipeline
        real = pipeline.APMEngine
        pipeline.APMEngine = lambda C, outputs=(): real(C, outputs=tuple(outputs) + ("tk",))
        try:
            super()._seed_engine()
        finally:
            pipeline.APMEngine = real


def case_table(C):
    labels = S.window_labels(C)
    rng = random.Random(1818)
    order, buckets, names, sizes = S.sized_cases(C, [0, 1, 5, 10, 11, 12, 33, 70, 200, 513], ("spread",), seed=18)

    def add(name, vals, server=S.SERVER, how="spread"):
        b = S.layout(list(vals), labels, how, where=len(order))
        k = (server, "S:" + name)
        assert k not in buckets
        buckets[k] = S.with_decoys(b, labels, len(order))
        order.append(k); names.append(name); sizes.append(len(vals))
        return k

    twin = [2000000] * 8 + S._values(rng, 40, lo=0, hi=900000)         # the largest per95 of the table, twice
    pair = S._values(rng, 25, lo=0, hi=3000)
    add("twin", twin)
    add("only_nan", [NAN] * 15)                                         # tpm 2.90: on the tpm board alone
    add("only_nan_small", [NAN] * 3)                                    # ... and under the floor
    add("nan_mixed", [NAN, 800000, NAN, 5, 7] + S._values(rng, 20, lo=0, hi=1000))
    add("pair", pair)
    add("under_floor_big_values", [999999] * 10)                        # tpm 1.94 < 2.0: cut everywhere
    add("at_floor", [123] * 11)                                         # tpm 2.13
    order.append(S.key("inactive")); names.append("inactive"); sizes.append(0)
    order.append(S.TRIGGER); names.append("trigger"); sizes.append(0)
    add("twin", twin, server=OTHER)                                     # identical windows on a second server
    add("pair", pair, server=OTHER)
    add("tail", S._values(rng, 60, lo=0, hi=5000), server=OTHER)
    return order, buckets, names


def test_one_rollover():
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=8)
    order, buckets, names = case_table(C)
    board = {"k": K, "by": BY, "minTpm": MIN_TPM}
    sd = TopSeeded(C, order, buckets, board=board)
    sd.step()
    got = sd.eng.take("tk")
    st = sd.eng.take("st")
    assert st == sd.st and len(st) == len(order) - 2      # (the inactive id and the trigger print nothing)
    want = R.rows_from_st(st, K, BY, MIN_TPM)
    assert sd.tk == want, "oracle and reference differ: " + str(S.first_difference(sd.tk, want, lambda i: ""))
    diff = S.first_difference(got, want, lambda i: want[i] if i < len(want) else "")
    assert diff is None, "tk rows: " + diff
    # each row's tail is its st row's tail
    st_by = {tuple(r.split("|")[2:4]): r for r in st}
    for r in got:
        f = r.split("|")
        assert f[4:] == st_by[(f[4], f[5])].split("|")[2:]
    rows = {name: [r.split("|") for r in got if r.split("|")[2] == name] for name in BY}
    for name in BY:
        assert [int(f[3]) for f in rows[name]] == list(range(1, len(rows[name]) + 1))
    # the table does what it was built for: ties across two servers keep the st order, the NaN
    # series are on the tpm board alone, the floor cuts, one board has fewer candidates than k
    assert [(f[4], f[5]) for f in rows["per95"][:2]] == [(S.SERVER, "S:twin"), (OTHER, "S:twin")]
    assert rows["per95"][0][6:] == rows["per95"][1][6:]
    pos = {(f[4], f[5]): int(f[3]) for f in rows["average"]}
    assert pos[(S.SERVER, "S:pair")] + 1 == pos[(OTHER, "S:pair")]
    assert len(rows["tpm"]) == K and len(rows["average"]) < K and len(rows["average"]) == len(rows["per95"])
    named = lambda name: {f[5] for f in rows[name]}
    assert "S:only_nan" in named("tpm") and "S:only_nan" not in named("average")
    for name in BY:
        assert not named(name) & {"S:under_floor_big_values", "S:only_nan_small", "S:n10_spread", "S:n0_spread"}
    assert "S:at_floor" in named("average") and "S:n11_spread" in named("average")
    assert any(f[7] in ("NaN", "undefined") for f in rows["tpm"])
    # the read-back: the same series, in rank order, with the raw doubles of the rows
    lb = sd.eng.eng.leaderboard()
    assert [(b, r, s) for b, r, s, *_ in lb] == [(f[2], int(f[3]), sd.ids[(f[4], f[5])]) for f in map(lambda r: r.split("|"), want)]
    for (b, r, s, tpm, avg, p75, p95), row in zip(lb, want):
        f = row.split("|")
        for x, text in zip((tpm, avg, p75, p95), f[6:]):
            assert S.same_double(x, R.st_number(text))
    # the st / fs rows are what an engine without the stream prints; off means no tk text
    plain = S.Seeded(sd.C, order, buckets, reference=False)
    plain.step()
    assert plain.eng.take("st") == st
    assert sd.eng.take("fs") == plain.eng.take("fs")
    assert plain.eng.take("tk") == [] and plain.eng.eng.leaderboard() == []


def test_no_candidate_prints_nothing_and_k_one():
    C = S.seeded_cfg(window=31, buffer=6, cell_cap=8)
    order, buckets, names = case_table(C)
    sd = TopSeeded(C, order, buckets, board={"k": 1, "by": ["average", "tpm"], "minTpm": 1e9})
    sd.step()
    assert sd.eng.take("tk") == [] == sd.tk and sd.eng.eng.leaderboard() == []
    assert sd.eng.take("st") == sd.st
    sd = TopSeeded(C, order, buckets, board={"k": 1, "by": ["average", "tpm"]})
    sd.step()
    got = sd.eng.take("tk")
    assert got == sd.tk == R.rows_from_st(sd.eng.take("st"), 1, ["average", "tpm"]) and len(got) == 2

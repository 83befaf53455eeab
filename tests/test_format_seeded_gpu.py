"""K12 line assembly (format.hip: length pass, scan, write pass) on whole st / fs lines from a
seeded engine, byte for byte against the oracle's rows -- in COPY mode against what the Python
COPY encoder makes of the oracle's wire rows.  The case table (seeded.format_cases, checked on
the CPU by tests/test_seeded_cases.py) covers series and LAG counts around the 64-line block,
inactive series at every position, all line-start and name alignments, the four LDS stages and
the direct path, every alignment of the fs stream's start, COPY escapes and the widest row.  Two
rollovers per engine: the second one's stage follows from the first one's bytes."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import seeded as S  # noqa: E402

CASES = {c.label: c for c in S.format_cases()}


def _describe(c, lines_per_series):
    def f(i):
        pos = i // lines_per_series
        return f"(line {i}, block {i // S.FMT_WAVE_LINES} of the lines present, about series {pos})"
    return f


@pytest.mark.parametrize("label", list(CASES))
def test_seeded_lines_match_oracle_bytes(label):
    c = CASES[label]
    sd = S.Seeded(c.cfg(), c.order, c.buckets, c.histories, reference=False)
    nat = sd.eng.eng
    if c.copy:
        nat.set_fs_copy(True)
    for r in range(2):
        want_st, want_fs = c.expected(r)
        sd.step()
        nat.flush()
        got_st, got_fs = sd.eng.take_bytes("st"), sd.eng.take_bytes("fs")
        for kind, got, want, per in (("st", got_st, want_st, 1), ("fs", got_fs, want_fs, c.n_lags)):
            if got != want:
                diff = S.first_difference(got.split(b"\n"), want.split(b"\n"), _describe(c, per))
                raise AssertionError(f"{label} rollover {r} (stage {c.stage(r)}), {kind}: {len(got)} bytes, "
                                     f"want {len(want)}; " + str(diff))
    assert len(want_st) > 0 and len(want_fs) > 0  # (the second rollover prints the trigger at least)
    # the printer's inexact flag: raised for the values inside its documented domain, no others
    assert sd.eng.metrics()["format_fallbacks"] == c.flag_count()

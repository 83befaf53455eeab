"""The fleet `fb` rows (format.hip k_fleet_len / k_fleet_rows) from chosen moments, byte for byte
against rows built in Python from Fraction moments (format_cases.FleetCase).  Every input prints
the same whether the variance is evaluated exactly, in plain fp64 or with a fused
product-subtract (checked on the CPU by tests/test_seeded_cases.py), so a difference here is the
formatter's: row order, the wave prefix, the stage copy, a digit."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import format_cases as F  # noqa: E402
import seeded as S  # noqa: E402
from apmbackend_amd import _native  # noqa: E402

CASES = {c.label: c for c in F.fleet_cases()}


@pytest.mark.parametrize("copy", (False, True), ids=("wire", "copy"))
@pytest.mark.parametrize("label", list(CASES))
def test_fleet_rows_match_fraction_reference(label, copy):
    N = _native.load(build_if_missing=False)
    c = CASES[label]
    want = c.expected(copy)
    got = N.gpu_fleet_rows(c.flat(), c.names, c.lag_values, c.slot_lo, c.n_slots, copy, F.EDGE_TS)
    assert len(want) > 0
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        diff = S.first_difference(g, w, lambda i: f"(wave {i // F.FLEET_RPW} of the rows present)")
        raise AssertionError(f"{label}: {len(got)} bytes, want {len(want)}; row " + str(diff))


def test_fleet_rows_of_an_empty_slice():
    N = _native.load(build_if_missing=False)
    c = CASES["rows16"]
    assert N.gpu_fleet_rows(c.flat(), c.names, c.lag_values, 3, 0, False, F.EDGE_TS) == b""

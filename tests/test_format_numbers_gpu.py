"""K12's number printer (textout.h fixed / js_fixed) at every branch boundary, against Decimal on
the exact binary value.  One launch per (mode, f) prints the whole table (format_cases.number_table)."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import format_cases as F  # noqa: E402
from apmbackend_amd import _native  # noqa: E402


@pytest.fixture(scope="module")
def native():
    return _native.load(build_if_missing=False)


@pytest.mark.parametrize("f", (1, 2))
@pytest.mark.parametrize("mode", F.MODES)
def test_gpu_number_printer_matches_decimal_reference(native, mode, f):
    xs = F.number_table()
    got = native.gpu_to_fixed(xs, f, mode)
    assert len(got) == len(xs)
    flagged = [i for i, g in enumerate(got) if g == "<fallback>"]
    outside = [(xs[i], xs[i].hex()) for i in flagged if not F.may_flag(xs[i], f, mode)]
    print(f"{mode} f={f}: {len(xs)} values, {len(flagged)} flagged, {len(outside)} flagged outside the documented domain")
    assert not outside, outside[:10]
    flagged = set(flagged)
    bad = []
    for i, (x, g) in enumerate(zip(xs, got)):
        if i not in flagged:
            w = F.ref_number(x, f, mode)
            if g != w:
                bad.append((x, x.hex(), g, w))
    assert not bad, f"{len(bad)} differ, first: {bad[:10]}"


def test_gpu_number_printer_default_mode_is_nf(native):
    xs = [0.25, -0.04, 2147483647.0, float("nan")]
    assert native.gpu_to_fixed(xs, 1) == native.gpu_to_fixed(xs, 1, "nf") == ["0.3", "-0.0", "2147483647.0", "undefined"]

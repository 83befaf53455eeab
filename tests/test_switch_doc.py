"""docs/SWITCHES.md lists exactly the APM_* environment switches the native code reads."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apmbackend_amd", "csrc")
DOC = os.path.join(ROOT, "docs", "SWITCHES.md")


def _switches_read():
    names = set()
    for d, _, files in os.walk(CSRC):
        for f in files:
            with open(os.path.join(d, f), encoding="utf-8", errors="replace") as fh:
                names.update(re.findall(r'getenv\(\s*"(APM_[A-Z0-9_]+)"', fh.read()))
    return names


def _switches_documented():
    names = []
    with open(DOC, encoding="utf-8") as fh:
        for line in fh:
            m = re.match(r"\|\s*`(APM_[A-Z0-9_]+)`\s*\|", line)
            if m:
                names.append(m.group(1))
    return names


def test_switch_doc_matches_native_getenv():
    read, doc = _switches_read(), _switches_documented()
    assert read, "no getenv(\"APM_...\") found under csrc: the scan is broken"
    assert len(doc) == len(set(doc)), "a switch is listed twice"
    assert set(doc) == read, (f"undocumented: {sorted(read - set(doc))}; "
                              f"documented but not read: {sorted(set(doc) - read)}")


def test_every_documented_switch_has_default_purpose_and_user():
    with open(DOC, encoding="utf-8") as fh:
        rows = [ln for ln in fh if re.match(r"\|\s*`APM_", ln)]
    for ln in rows:
        cells = [c.strip() for c in ln.strip().strip("|").split("|")]
        assert len(cells) == 4 and all(cells), ln

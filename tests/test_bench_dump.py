"""bench.py --dump-outputs: the record -> array encoding (CPU) and one small run on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _h(tok: bytes) -> float:
    import hashlib
    return float(int.from_bytes(hashlib.blake2b(tok, digest_size=6).digest(), "big"))


def test_dump_outputs_encodes_sorted_records(tmp_path):
    fs = (b"fs|1578391500000|jvm001|S:b|360|1.20|5.0:undefined:NaN:3.0:0|1.0:2.0:3.0:4.0:1.0|9.5:8.0:7.0:6.0:-1.0\n"
          b"fs|1578391500000|jvm000|a|360|12.00|5.0:1.5:2.0:3.0:1|1.0:2.0:3.0:4.0:0.0|9.5:8.0:7.0:6.0:0.0\n")
    d = str(tmp_path / "d")
    w = bench.dump_outputs(d, {"fs": fs, "al": b"", "db": b"tx|jvm000|a|L_1|7|1|2|1_0|Y\n"})
    assert w == {"fs.npy": [2, 22], "db.npy": [1, 9], "rows.npy": [3]}
    assert sorted(os.listdir(d)) == ["db.npy", "fs.npy", "rows.npy"]  # no file for the empty stream
    assert np.load(os.path.join(d, "rows.npy")).tolist() == [0.0, 1.0, 2.0]  # al, db, fs
    a = np.load(os.path.join(d, "fs.npy"))
    assert a.dtype == np.float64 and np.isfinite(a).all()
    # sorted as bytes: jvm000 first; its service has no ':' so the row is one field short (0-padded)
    assert a[0].tolist() == [_h(b"fs"), 1578391500000.0, _h(b"jvm000"), _h(b"a"), 360.0, 12.0, 5.0, 1.5, 2.0, 3.0, 1.0,
                             1.0, 2.0, 3.0, 4.0, 0.0, 9.5, 8.0, 7.0, 6.0, 0.0, 0.0]
    assert a[1].tolist() == [_h(b"fs"), 1578391500000.0, _h(b"jvm001"), _h(b"S"), _h(b"b"), 360.0, 1.2, 5.0,
                             _h(b"undefined"), _h(b"NaN"), 3.0, 0.0, 1.0, 2.0, 3.0, 4.0, 1.0, 9.5, 8.0, 7.0, 6.0, -1.0]
    db = np.load(os.path.join(d, "db.npy"))
    assert db[0].tolist() == [_h(b"tx"), _h(b"jvm000"), _h(b"a"), _h(b"L_1"), 7.0, 1.0, 2.0, _h(b"1_0"), _h(b"Y")]
    assert _h(b"undefined") < 2.0 ** 48 and float(int(_h(b"undefined"))) == _h(b"undefined")


def test_dump_outputs_budget_keeps_a_fixed_sample(tmp_path):
    db = b"".join(b"tx|jvm%03d|svc|L%d|1|2|3|%d|Y\n" % (i % 7, i, i) for i in range(1000))
    s = {"db": db, "al": b"al|1|2|jvm000|svc|cause|fs&1&jvm000&svc\n"}
    full = bench.dump_outputs(str(tmp_path / "full"), s)
    assert full["db.npy"] == [1000, 9]
    budget = 20000
    w1 = bench.dump_outputs(str(tmp_path / "a"), s, budget=budget)
    w2 = bench.dump_outputs(str(tmp_path / "b"), s, budget=budget)
    assert w1 == w2 and w1["al.npy"] == full["al.npy"] and 200 < w1["db.npy"][0] < 1000
    a, b = np.load(tmp_path / "a" / "db.npy"), np.load(tmp_path / "b" / "db.npy")
    assert np.array_equal(a, b)
    assert a.nbytes + np.load(tmp_path / "a" / "al.npy").nbytes <= budget
    whole = np.load(tmp_path / "full" / "db.npy")
    pos = [int(np.flatnonzero((whole == r).all(axis=1))[0]) for r in a]
    assert pos == sorted(set(pos))  # rows of the whole array, in its order
    assert np.load(tmp_path / "a" / "rows.npy").tolist() == [1.0, 1000.0]  # the counts are of all records


@pytest.mark.gpu
def test_bench_dump_outputs_small_shard_is_repeatable(tmp_path):
    """Two runs with the same arguments write the same arrays; --steps sets the timed steps."""
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
            "--servers", "2", "--ejb", "60", "--providers", "40", "--pre-batches", "33", "--gen-threads", "4"]
    procs = [subprocess.Popen(base + ["--dump-outputs", str(tmp_path / n)], cwd=ROOT, text=True,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              env=dict(os.environ, PYTHONUNBUFFERED="1")) for n in ("a", "b")]
    outs = []
    for p in procs:
        so, se = p.communicate(timeout=200)
        assert p.returncode == 0, (so[-2000:], se[-4000:])
        rows = [l for l in so.splitlines() if l.startswith("{") and '"metric"' in l]
        assert len(rows) == 1, so[-3000:]
        outs.append(json.loads(rows[0]))
    r = outs[0]
    assert r["steps"] == 3 and len(r["step_ms"]) == 3 and r["ms_per_step"] > 0
    assert r["lines_total"] == outs[1]["lines_total"] > 0
    assert r["dump_outputs"]["files"] == outs[1]["dump_outputs"]["files"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == sorted(r["dump_outputs"]["files"])
    assert {"db.npy", "fs.npy", "fb.npy", "rows.npy"} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64 and np.isfinite(a).all()
        assert a.shape == b.shape and np.array_equal(a, b), n
        total += os.path.getsize(tmp_path / "a" / n)
    assert total <= 64 << 20
    fs = np.load(tmp_path / "a" / "fs.npy")
    # one interval edge in the last step: one fs row per series and LAG, all of the same interval
    assert fs.shape[0] == r["series_per_gpu"] * 2 and len(set(fs[:, 1].tolist())) == 1

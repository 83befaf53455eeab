"""Driver for profiling the K18 tk kernels (topk.hip) next to K8 on the headline shard.

Feeds the shard tests/test_scale_gpu.py uses (8 JVMs x 10k services, 80k series): 33 ten-second
batches of pre-history so the K8 window is full, then 20 more (one rollover each) with the tk
stream on (k = 20, boards per95 / average / tpm).  Run it under the kernel trace, in a run of its
own, and compare k_topk_tile and k_topk_final with k_window_stats_h2 from the same trace:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/topk_prof.py
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from apmbackend_amd import _native  # noqa: E402
from apmbackend_amd.models.pipeline import APMEngine  # noqa: E402
from apmbackend_amd.utils.config import default_config  # noqa: E402

START = 1578391200000
STEP_MS = 10_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pre", type=int, default=33)
    ap.add_argument("--rollovers", type=int, default=20)
    ap.add_argument("--no-tk", action="store_true")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--by", default="per95,average,tpm")
    ap.add_argument("--min-tpm", type=float, default=0.0)
    a = ap.parse_args()
    N = _native.load(build_if_missing=False)
    gen = N.SynthGen({"servers": 8, "ejb_services": 6000, "provider_services": 4000, "tx_per_sec_per_server": 250.0,
                      "seed": 3, "anomaly_services": 16, "anomaly_factor": 25.0,
                      "anomaly_start_ms": START + 2 * STEP_MS})
    C = default_config(replay=True)
    C["gpu"].update({"timezone": "UTC", "maxSeries": 1 << 17, "batchBytes": 48 << 20, "maxLinesPerBatch": 1 << 20,
                     "zscoreMeanMode": "rolling", "ringDtype": "float64", "bucketCellCapacity": 16})
    outs = ("st", "fs", "al")
    if not a.no_tk:
        C["gpu"]["leaderboard"] = {"k": a.k, "by": a.by.split(","), "minTpm": a.min_tpm}
        outs += ("tk",)
    eng = APMEngine(C, outputs=outs)
    for path, kind, server in gen.files():
        eng.add_file(path, {0: "SOAP", 1: "SERVER", 2: "APP"}[kind], server)
    rows = {k: 0 for k in outs}
    nbytes = {k: 0 for k in outs}
    t0 = time.time()
    for b in range(a.pre + a.rollovers):
        data, chunks = gen.generate(START + (b + 1) * STEP_MS, 16)
        eng.eng.process_batch(data, chunks, -1.0)
        for k in outs:
            blob = eng.take_bytes(k)
            if b >= a.pre:
                rows[k] += blob.count(b"\n")
                nbytes[k] += len(blob)
    m = eng.metrics()
    per = max(a.rollovers, 1)
    print(f"series {m['series']} rollovers {m['rollovers']} wall {time.time() - t0:.1f} s; last {a.rollovers} rollovers: "
          + "; ".join(f"{k} rows {rows[k]} bytes {nbytes[k]} ({nbytes[k] // per} each)" for k in outs if k in ("st", "tk")))


if __name__ == "__main__":
    main()

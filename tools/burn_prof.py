"""Driver for profiling the K21 sb kernels (burn.hip) next to K8, K17 and K12 on the headline shard.

Feeds the shard tests/test_scale_gpu.py uses (8 JVMs x 10k services, 80k series): 33 ten-second
batches of pre-history so the K8 window is full, then 20 more (one rollover each) with the sb
stream on: the default objective {threshold, target}, the rules [1 bucket at 14.4, 6 buckets at 6]
and minSamples 1.  The sl stream is on as well (one threshold, the same value), so k_slo_group
stands in the same trace.  Run it under the kernel trace, in a run of its own, and compare
k_burn_* with k_window_stats_h2, k_slo_group and k_format_write:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/burn_prof.py
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
    ap.add_argument("--no-sb", action="store_true")
    ap.add_argument("--no-sl", action="store_true")
    ap.add_argument("--threshold", type=int, default=2000)
    ap.add_argument("--target", default="99")
    ap.add_argument("--min-samples", type=int, default=1)
    a = ap.parse_args()
    N = _native.load(build_if_missing=False)
    gen = N.SynthGen({"servers": 8, "ejb_services": 6000, "provider_services": 4000, "tx_per_sec_per_server": 250.0,
                      "seed": 3, "anomaly_services": 16, "anomaly_factor": 25.0,
                      "anomaly_start_ms": START + 2 * STEP_MS})
    C = default_config(replay=True)
    C["gpu"].update({"timezone": "UTC", "maxSeries": 1 << 17, "batchBytes": 48 << 20, "maxLinesPerBatch": 1 << 20,
                     "zscoreMeanMode": "rolling", "ringDtype": "float64", "bucketCellCapacity": 16})
    outs = ("st", "fs", "al")
    if not a.no_sl:
        C["gpu"]["latencyObjectives"] = {"default": [a.threshold]}
        outs += ("sl",)
    if not a.no_sb:
        C["gpu"]["sloBurn"] = {"default": {"threshold": a.threshold, "target": a.target},
                               "rules": [{"short": 1, "factor": 14.4}, {"short": 6, "factor": 6}],
                               "minSamples": a.min_samples}
        outs += ("sb",)
    eng = APMEngine(C, outputs=outs)
    for path, kind, server in gen.files():
        eng.add_file(path, {0: "SOAP", 1: "SERVER", 2: "APP"}[kind], server)
    rows = nbytes = st_rows = 0
    t0 = time.time()
    for b in range(a.pre + a.rollovers):
        data, chunks = gen.generate(START + (b + 1) * STEP_MS, 16)
        eng.eng.process_batch(data, chunks, -1.0)
        for k in outs:
            blob = eng.take_bytes(k)
            if k == "sb" and b >= a.pre:
                rows += blob.count(b"\n")
                nbytes += len(blob)
            if k == "st" and b >= a.pre:
                st_rows += blob.count(b"\n")
    m = eng.metrics()
    print(f"series {m['series']} rollovers {m['rollovers']} sb rows {rows} sb bytes {nbytes} "
          f"(last {a.rollovers} rollovers: {rows // max(a.rollovers, 1)} rows, {nbytes // max(a.rollovers, 1)} bytes each; "
          f"sb_rows metric {m['sb_rows']}) st rows {st_rows} wall {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()

"""Driver for profiling the K22 tf kernels (traffic.hip) next to K8, K21 and K12 on the headline shard.

Feeds the shard tests/test_scale_gpu.py uses (8 JVMs x 10k services, 80k series): 33 ten-second
batches of pre-history so the K8 window is full, then 20 more (one rollover each) with the tf
stream on: the default minRate, the rules [1 bucket: drop 0.1, z 4] and [6 buckets: drop 0.5,
surge 3, z 3] and minBuckets 8.  The sb stream is on as well (tools/burn_prof.py's settings), so
k_burn_group stands in the same trace.  Run it under the kernel trace, in a run of its own, and
compare k_traffic_* with k_window_stats_h2, k_burn_group and k_format_write:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/traffic_prof.py
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
    ap.add_argument("--no-tf", action="store_true")
    ap.add_argument("--no-sb", action="store_true")
    ap.add_argument("--min-rate", type=int, default=1)
    ap.add_argument("--min-buckets", type=int, default=8)
    a = ap.parse_args()
    N = _native.load(build_if_missing=False)
    gen = N.SynthGen({"servers": 8, "ejb_services": 6000, "provider_services": 4000, "tx_per_sec_per_server": 250.0,
                      "seed": 3, "anomaly_services": 16, "anomaly_factor": 25.0,
                      "anomaly_start_ms": START + 2 * STEP_MS})
    C = default_config(replay=True)
    C["gpu"].update({"timezone": "UTC", "maxSeries": 1 << 17, "batchBytes": 48 << 20, "maxLinesPerBatch": 1 << 20,
                     "zscoreMeanMode": "rolling", "ringDtype": "float64", "bucketCellCapacity": 16})
    outs = ("st", "fs", "al")
    if not a.no_sb:
        C["gpu"]["sloBurn"] = {"default": {"threshold": 2000, "target": "99"},
                               "rules": [{"short": 1, "factor": 14.4}, {"short": 6, "factor": 6}], "minSamples": 1}
        outs += ("sb",)
    if not a.no_tf:
        C["gpu"]["trafficWatch"] = {"default": {"minRate": a.min_rate},
                                    "rules": [{"short": 1, "drop": 0.1, "z": 4},
                                              {"short": 6, "drop": 0.5, "surge": 3, "z": 3}],
                                    "minBuckets": a.min_buckets}
        outs += ("tf",)
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
            if k == "tf" and b >= a.pre:
                rows += blob.count(b"\n")
                nbytes += len(blob)
            if k == "st" and b >= a.pre:
                st_rows += blob.count(b"\n")
    m = eng.metrics()
    print(f"series {m['series']} rollovers {m['rollovers']} tf rows {rows} tf bytes {nbytes} "
          f"(last {a.rollovers} rollovers: {rows // max(a.rollovers, 1)} rows, {nbytes // max(a.rollovers, 1)} bytes each; "
          f"tf_rows metric {m['tf_rows']}) st rows {st_rows} wall {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()

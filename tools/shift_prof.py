"""Driver for profiling the K24 ls kernels (shift.hip) next to K8, K16 and K20 on the headline shard.

Feeds the shard tests/test_scale_gpu.py uses (8 JVMs x 10k services, 80k series): 33 ten-second
batches of pre-history so the K8 window is full, then 20 more (one rollover each) with the ls
stream on: the default minDelta, the rules [1 bucket: p95 up 3], [6 buckets: p95 up 3, z 4] and
[6 buckets: p25 down 2], minRecent 20 and minBaseline 100.  The wp and rw streams are on as well, so
k_winpct_group and k_recent_group stand in the same trace.  Run it under the kernel trace, in a
run of its own, and compare k_shift_group with k_window_stats_h2, k_winpct_group and k_recent_group:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/shift_prof.py
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
    ap.add_argument("--no-ls", action="store_true")
    ap.add_argument("--no-wp", action="store_true")
    ap.add_argument("--no-rw", action="store_true")
    ap.add_argument("--min-delta", type=int, default=50)
    ap.add_argument("--min-recent", type=int, default=20)
    ap.add_argument("--min-baseline", type=int, default=100)
    a = ap.parse_args()
    N = _native.load(build_if_missing=False)
    gen = N.SynthGen({"servers": 8, "ejb_services": 6000, "provider_services": 4000, "tx_per_sec_per_server": 250.0,
                      "seed": 3, "anomaly_services": 16, "anomaly_factor": 25.0,
                      "anomaly_start_ms": START + 2 * STEP_MS})
    C = default_config(replay=True)
    C["gpu"].update({"timezone": "UTC", "maxSeries": 1 << 17, "batchBytes": 48 << 20, "maxLinesPerBatch": 1 << 20,
                     "zscoreMeanMode": "rolling", "ringDtype": "float64", "bucketCellCapacity": 16})
    outs = ("st", "fs", "al")
    if not a.no_wp:
        C["gpu"]["windowPercentiles"] = [50, 95]
        outs += ("wp",)
    if not a.no_rw:
        C["gpu"]["recentWindows"] = {"buckets": [1, 6], "percentiles": [50, 95]}
        outs += ("rw",)
    if not a.no_ls:
        C["gpu"]["latencyShift"] = {"default": {"minDelta": a.min_delta},
                                    "rules": [{"short": 1, "percentile": 95, "up": 3},
                                              {"short": 6, "percentile": 95, "up": 3, "z": 4},
                                              {"short": 6, "percentile": 25, "down": 2}],
                                    "minRecent": a.min_recent, "minBaseline": a.min_baseline}
        outs += ("ls",)
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
            if k == "ls" and b >= a.pre:
                rows += blob.count(b"\n")
                nbytes += len(blob)
            if k == "st" and b >= a.pre:
                st_rows += blob.count(b"\n")
    m = eng.metrics()
    print(f"series {m['series']} rollovers {m['rollovers']} ls rows {rows} ls bytes {nbytes} "
          f"(last {a.rollovers} rollovers: {rows // max(a.rollovers, 1)} rows, {nbytes // max(a.rollovers, 1)} bytes each; "
          f"ls_rows metric {m['ls_rows']}) st rows {st_rows} wall {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()

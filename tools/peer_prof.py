"""Driver for profiling the K23 po kernels (peers.hip) next to K8, K16's value pass and K19 on the headline shard.

Feeds the shard tests/test_scale_gpu.py uses (8 JVMs x 10k services, 80k series, so 10 000 groups of
8 peers): 33 ten-second batches of pre-history so the K8 window is full, then 20 more (one rollover
each) with the po stream on: percentile 95, the default minValue, high 2, low 0.25, z 3, minDelta
10, minPeers 5.  The sv stream is on as well, so k_svcwin_group stands in the same trace, and
k_winpct_group there is the po stream's own stage A.  Run it under the kernel trace, in a run of
its own, and compare k_peer_group with k_window_stats_h2, k_winpct_group and k_svcwin_group:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/peer_prof.py
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
    ap.add_argument("--no-po", action="store_true")
    ap.add_argument("--no-sv", action="store_true")
    ap.add_argument("--min-value", type=int, default=20)
    ap.add_argument("--min-samples", type=int, default=20)
    a = ap.parse_args()
    N = _native.load(build_if_missing=False)
    gen = N.SynthGen({"servers": 8, "ejb_services": 6000, "provider_services": 4000, "tx_per_sec_per_server": 250.0,
                      "seed": 3, "anomaly_services": 16, "anomaly_factor": 25.0,
                      "anomaly_start_ms": START + 2 * STEP_MS})
    C = default_config(replay=True)
    C["gpu"].update({"timezone": "UTC", "maxSeries": 1 << 17, "batchBytes": 48 << 20, "maxLinesPerBatch": 1 << 20,
                     "zscoreMeanMode": "rolling", "ringDtype": "float64", "bucketCellCapacity": 16})
    outs = ("st", "fs", "al")
    if not a.no_sv:
        C["gpu"]["serviceWindow"] = {"percentiles": [50, 95]}
        outs += ("sv",)
    if not a.no_po:
        C["gpu"]["peerOutliers"] = {"percentile": 95, "default": {"minValue": a.min_value}, "high": 2, "low": 0.25, "z": 3,
                                    "minDelta": 10, "minPeers": 5, "minSamples": a.min_samples}
        outs += ("po",)
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
            if k == "po" and b >= a.pre:
                rows += blob.count(b"\n")
                nbytes += len(blob)
            if k == "st" and b >= a.pre:
                st_rows += blob.count(b"\n")
    m = eng.metrics()
    print(f"series {m['series']} rollovers {m['rollovers']} po rows {rows} po bytes {nbytes} "
          f"(last {a.rollovers} rollovers: {rows // max(a.rollovers, 1)} rows, {nbytes // max(a.rollovers, 1)} bytes each; "
          f"po_rows metric {m['po_rows']}) st rows {st_rows} wall {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()

"""Driver for profiling the K25 ic kernels (incident.hip) next to K21's k_burn_group on the headline shard.

Feeds the shard tests/test_scale_gpu.py uses (8 JVMs x 10k services, 80k series): 33 ten-second
batches of pre-history so the K8 window is full, then 20 more (one rollover each) with the sb, tf,
po and ls streams on and all four as sources of the ic stream.  Run it under the kernel trace, in a
run of its own, and compare k_incident_step, k_text_len<IcRow> and k_incident_write with
k_burn_group:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/incident_prof.py
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
    ap.add_argument("--no-ic", action="store_true")
    ap.add_argument("--remind-every", type=int, default=6)
    a = ap.parse_args()
    N = _native.load(build_if_missing=False)
    gen = N.SynthGen({"servers": 8, "ejb_services": 6000, "provider_services": 4000, "tx_per_sec_per_server": 250.0,
                      "seed": 3, "anomaly_services": 16, "anomaly_factor": 25.0,
                      "anomaly_start_ms": START + 2 * STEP_MS})
    C = default_config(replay=True)
    C["gpu"].update({"timezone": "UTC", "maxSeries": 1 << 17, "batchBytes": 48 << 20, "maxLinesPerBatch": 1 << 20,
                     "zscoreMeanMode": "rolling", "ringDtype": "float64", "bucketCellCapacity": 16})
    C["gpu"]["sloBurn"] = {"default": {"threshold": 400, "target": 99}, "rules": [{"short": 1, "factor": 14.4},
                                                                                    {"short": 6, "factor": 6}],
                           "minSamples": 5}
    C["gpu"]["trafficWatch"] = {"default": {"minRate": 1}, "rules": [{"short": 1, "drop": 0.2, "surge": 3, "z": 3}],
                                "minBuckets": 4}
    C["gpu"]["peerOutliers"] = {"percentile": 95, "default": {"minValue": 20}, "high": 2, "low": 0.25, "z": 3,
                                "minDelta": 10, "minPeers": 5, "minSamples": 5}
    C["gpu"]["latencyShift"] = {"default": {"minDelta": 50}, "rules": [{"short": 6, "percentile": 95, "up": 3, "z": 4}],
                                "minRecent": 5, "minBaseline": 20}
    outs = ("st", "fs", "al", "sb", "tf", "po", "ls")
    if not a.no_ic:
        C["gpu"]["incidents"] = {"sources": {k: {"openAfter": 2, "closeAfter": 3} for k in ("sb", "tf", "po", "ls")},
                                 "remindEvery": a.remind_every}
        outs += ("ic",)
    eng = APMEngine(C, outputs=outs)
    for path, kind, server in gen.files():
        eng.add_file(path, {0: "SOAP", 1: "SERVER", 2: "APP"}[kind], server)
    rows = nbytes = 0
    t0 = time.time()
    for b in range(a.pre + a.rollovers):
        data, chunks = gen.generate(START + (b + 1) * STEP_MS, 16)
        eng.eng.process_batch(data, chunks, -1.0)
        for k in outs:
            blob = eng.take_bytes(k)
            if k == "ic" and b >= a.pre:
                rows += blob.count(b"\n")
                nbytes += len(blob)
    m = eng.metrics()
    print(f"series {m['series']} rollovers {m['rollovers']} ic rows {rows} ic bytes {nbytes} (last {a.rollovers} rollovers; "
          f"ic_rows metric {m['ic_rows']}, open sb {m['ic_open_sb']} tf {m['ic_open_tf']} po {m['ic_open_po']} "
          f"ls {m['ic_open_ls']}) wall {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Sample subsets of a GRM store (pcoa_create_grm_subset) on device-resident .bed rows (not a test, not bench.py).

Per size N x V of tools/grm_probe.py, in one process: the synthetic PLINK rows of that probe are appended to a GRM engine, and
the probe reports
  append           pcoa_accumulate_plink_bed of the device rows, in calls of 2^20 rows, to pcoa_sync (wall clock): what feeding
                   the reduced cohort again would cost at best, the rows being on the device already
  subset -100      one pcoa_create_grm_subset with 100 samples removed, spread evenly over the cohort
  subset 1/2       one with every second sample removed
                   both as the HIP-event time of the gather launches (pcoa_get_grm_subset_stats; median of three calls after
                   one warm call) and as the wall clock of the whole call, which also creates the engine and its segments
  product          one pcoa_grm_matvec_device on the source engine (median of five after one warm call)
and, for each subset, the share of V x (src pitch + dst pitch) bytes at the 6.29 TB/s measured copy ceiling that the gather
reaches, and its ratio to the append.

Usage: python tools/grm_subset_probe.py [--sizes 2504x1000000,20000x262144,100000x131072] [--out profiles/NAME.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from grm_probe import COPY_CEILING, DEFAULT_SIZES, planted_bed, timed  # noqa: E402


def subset_times(eng, keep, repeats=3):
    """(median HIP-event seconds of the gather, median wall seconds of the call, bytes per call)"""
    ev, wall, nbytes = [], [], 0
    for k in range(repeats + 1):
        s0 = eng.grm_subset_stats()
        t0 = time.perf_counter()
        sub = eng.grm_subset(keep)
        w = time.perf_counter() - t0
        s1 = eng.grm_subset_stats()
        sub.close()
        if k > 0:      # (the first call loads the code object)
            ev.append(s1["grm_subset_seconds"] - s0["grm_subset_seconds"])
            wall.append(w)
            nbytes = s1["grm_subset_bytes"] - s0["grm_subset_bytes"]
    return statistics.median(ev), statistics.median(wall), nbytes


def run_size(P, n, v, seed):
    import numpy as np
    import torch
    rows = planted_bed(n, v, seed)
    call = 1 << 20
    x = torch.randn(n, dtype=torch.float64, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(seed + 1))
    out = {"n": n, "v": v, "bed_bytes": int(rows.numel())}
    with P.PcoaEngine(n, grm=True) as eng:
        eng.reserve(min(v, call), 2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r0 in range(0, v, call):
            eng.accumulate_plink_bed(rows[r0:r0 + call])
        eng.sync()
        out["append_s"] = time.perf_counter() - t0
        out["store_bytes"] = eng.grm_info()[2]
        out["product_ms"] = 1e3 * timed(lambda: eng.grm_matvec_device(x))
        idx = np.arange(n)
        lists = {"minus_100": np.delete(idx, (np.arange(100) * n) // 100 + n // 200), "every_second": idx[::2]}
        for name, keep in lists.items():
            ev, wall, nbytes = subset_times(eng, keep)
            ideal = nbytes / COPY_CEILING
            out[name] = {"n_keep": int(keep.size), "gather_ms": 1e3 * ev, "call_wall_ms": 1e3 * wall, "bytes": int(nbytes),
                         "at_copy_ceiling_ms": 1e3 * ideal, "share_of_copy_ceiling": ideal / ev, "gather_over_append": ev / out["append_s"],
                         "gather_over_product": ev / (1e-3 * out["product_ms"])}
        out["device"] = eng.device_info()[0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=DEFAULT_SIZES, help="comma-separated NxV")
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    P = importlib.import_module("spark-examples_amd")
    doc = {"tool": "tools/grm_subset_probe.py", "library": P._lib.load().pcoa_version().decode(), "source_hash": P._lib.source_hash(),
           "copy_ceiling_bytes_per_s": COPY_CEILING, "sizes": []}
    for n, v in [tuple(int(t) for t in s.split("x")) for s in args.sizes.split(",")]:
        doc["sizes"].append(run_size(P, n, v, args.seed))
        print(json.dumps(doc["sizes"][-1]), flush=True)
        if args.out:      # after every size: a later size that fails leaves the earlier ones on file
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""The relatedness cut-off on K (pcoa_grm_pairs) on device-resident .bed rows (not a test, not bench.py).

Per size N x V of tools/grm_probe.py, in one process: the synthetic PLINK rows of that probe are appended to a GRM engine, the
cutoff is taken from the engine's own K (the 99.99th percentile above the diagonal of its leading 2,048 x 2,048 block, so that
about one pair in 10,000 is reported), and the probe reports
  pairs            one pcoa_grm_pairs over the bands it is given (band_rows 1,024, capacity 2^20): wall clock of the call, and
                   from pcoa_get_grm_pairs_stats the HIP-event time of all its launches, the share of the count / scan / write
                   kernels in it, the bytes they read and their rate against the 6.29 TB/s measured copy ceiling
  blocks           the same bands [r0, r0 + 1,024) x [r0, N) read with pcoa_grm_block into device memory, one call a band: the
                   dense product alone, which is what a caller had before the screen existed (wall clock; HIP-event time)
and their ratio.  pcoa_grm_pairs always walks the whole triangle, so above --triangle-max samples the probe screens a subset
engine over the leading --bands-above x 1,024 samples instead: a few bands, not the triangle of N, and not bands of N's full
width; the record says so.

--resources writes the VGPR / scratch / occupancy lines hipcc prints for grm_pairs.hip.

Usage: python tools/grm_pairs_probe.py [--sizes 2504x1000000,20000x262144,100000x131072] [--out profiles/NAME.json]
                                       [--resources profiles/NAME.txt]
"""
import argparse
import importlib
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from grm_probe import COPY_CEILING, DEFAULT_SIZES, planted_bed  # noqa: E402

BAND = 1024


def delta(after, before):
    return dict((k, after[k] - before[k]) for k in after)


def pairs_once(eng, cutoff, divisor):
    s0 = eng.grm_pairs_stats()
    t0 = time.perf_counter()
    _, found = eng.grm_pairs(cutoff, divisor, band_rows=BAND, capacity=1 << 20)
    wall = time.perf_counter() - t0
    d = delta(eng.grm_pairs_stats(), s0)
    return {"wall_s": wall, "event_s": d["grm_pairs_seconds"], "screen_event_s": d["grm_pairs_screen_seconds"],
            "bands": int(d["grm_pairs_bands"]), "flops": d["grm_pairs_flops"], "screen_bytes": int(d["grm_pairs_bytes"]),
            "n_found": int(found)}


def blocks_once(eng, divisor):
    import torch
    n = eng.n
    s0 = eng.grm_block_stats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r0 in range(0, n, BAND):
        eng.grm_block(r0, min(BAND, n - r0), r0, n - r0, divisor, device=True)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    d = delta(eng.grm_block_stats(), s0)
    return {"wall_s": wall, "event_s": d["grm_block_seconds"], "flops": d["grm_block_flops"]}


def median_of(runs):
    return dict((k, statistics.median(r[k] for r in runs)) for k in runs[0])


def screen(eng, repeats):
    import numpy as np
    lead = min(eng.n, 2048)
    k = eng.grm_block(0, lead, 0, lead, "used")
    cutoff = float(np.quantile(k[np.triu_indices(lead, 1)], 0.9999))
    out = {"cutoff": cutoff, "n_screened": eng.n}
    for divisor in ("used", "pairwise"):
        pairs_once(eng, cutoff, divisor)      # (the first call grows the workspace)
        blocks_once(eng, divisor)
        p = median_of([pairs_once(eng, cutoff, divisor) for _ in range(repeats)])
        b = median_of([blocks_once(eng, divisor) for _ in range(repeats)])
        out[divisor] = {"pairs": p, "blocks": b, "pairs_over_blocks_wall": p["wall_s"] / b["wall_s"],
                        "pairs_over_blocks_event": p["event_s"] / b["event_s"],
                        "screen_share_of_event_time": p["screen_event_s"] / p["event_s"],
                        "screen_bytes_per_s": p["screen_bytes"] / p["screen_event_s"],
                        "screen_share_of_copy_ceiling": p["screen_bytes"] / p["screen_event_s"] / COPY_CEILING}
    return out


def run_size(P, n, v, seed, triangle_max, bands_above, repeats):
    import numpy as np
    import torch
    rows = planted_bed(n, v, seed)
    call = 1 << 20
    out = {"n": n, "v": v, "bed_bytes": int(rows.numel())}
    with P.PcoaEngine(n, grm=True) as eng:
        eng.reserve(min(v, call), 2)
        for r0 in range(0, v, call):
            eng.accumulate_plink_bed(rows[r0:r0 + call])
        eng.sync()
        del rows
        torch.cuda.empty_cache()
        out["store_bytes"] = eng.grm_info()[2]
        out["device"] = eng.device_info()[0]
        if n <= triangle_max:
            out["what"] = "the whole triangle, %d bands" % (-(-n // BAND))
            out.update(screen(eng, repeats))
        else:
            lead = bands_above * BAND
            out["what"] = ("the triangle of the leading %d samples (%d bands) as a subset engine with its own allele frequencies: "
                           "a few bands, not the triangle of N" % (lead, bands_above))
            with eng.grm_subset(np.arange(lead)) as sub:
                out.update(screen(sub, repeats))
    return out


def kernel_resources(path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                              "-c", os.path.join(csrc, "grm_pairs.hip"), "-o", os.path.join(td, "x.o"), "-Rpass-analysis=kernel-resource-usage"],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if res.returncode != 0:
        raise SystemExit(res.stdout[-2000:])
    keep = re.findall(r"remark: +((?:Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size "
                      r"\[bytes/block\]): .*?) \[-Rpass", res.stdout)
    with open(path, "w") as f:
        f.write("\n".join(keep) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=DEFAULT_SIZES, help="comma-separated NxV")
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--triangle-max", type=int, default=30000, help="largest N whose whole triangle is screened")
    ap.add_argument("--bands-above", type=int, default=8, help="bands of 1,024 samples screened above --triangle-max")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None, help="write the compile-time resources of the grm_pairs.hip kernels here (needs hipcc, no GPU)")
    args = ap.parse_args()
    if args.resources:
        kernel_resources(args.resources)
        if not args.out:
            return 0
    P = importlib.import_module("spark-examples_amd")
    with P.PcoaEngine(256, grm=True) as e:      # code objects, first-use allocations
        e.accumulate_plink_bed(planted_bed(256, 512, args.seed))
        e.grm_pairs(0.05, "pairwise")
        e.grm_block(0, 256, 0, 256, "pairwise", device=True)
    doc = {"tool": "tools/grm_pairs_probe.py", "library": P._lib.load().pcoa_version().decode(), "source_hash": P._lib.source_hash(),
           "copy_ceiling_bytes_per_s": COPY_CEILING, "band_rows": BAND, "medians_of": args.repeats,
           "not_measured": ["bands of the full width at N above --triangle-max", "the count, scan and write kernels apart",
                            "host-pointer output of the blocks", "hardware counters"],
           "sizes": []}
    for n, v in [tuple(int(t) for t in s.split("x")) for s in args.sizes.split(",")]:
        doc["sizes"].append(run_size(P, n, v, args.seed, args.triangle_max, args.bands_above, args.repeats))
        print(json.dumps(doc["sizes"][-1]), flush=True)
        if args.out:      # after every size: a later size that fails leaves the earlier ones on file
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""The KING-robust screen on the 2-bit store (pcoa_grm_king_pairs) on device-resident .bed rows (not a test, not bench.py).

Per size N x V of tools/grm_probe.py, in one process: the synthetic PLINK rows of that probe are appended to a GRM engine and
the probe reports, as medians of --repeats calls after a warm one,
  king             one pcoa_grm_king_pairs(0.177, rows all, band_rows 1,024, capacity 2^20): wall clock of the call, and from
                   pcoa_get_grm_king_stats the HIP-event time of all its launches, the share of the screen kernels in it, the
                   int8 multiply-adds the count kernel issued and their rate against the matrix-core peak of
                   v_mfma_i32_32x32x32_i8 (32,768 MACs in 32 cycles per SIMD: 1,024 SIMDs x 2.4 GHz = 2.52e15 MAC/s)
  grm_pairs        one pcoa_grm_pairs(PAIRWISE) on the same store at a cutoff that reports about one pair in 10,000: the only
                   relatedness screen a GRM ctx had before
  planes           where 5 N^2 int32 fit (N <= --planes-max): the five-plane path on the same rows -- pcoa_accumulate_plink_bed_king
                   of the whole store's rows, then pcoa_king_pairs -- wall clock of each
pcoa_grm_king_pairs always walks the whole triangle, so above --triangle-max samples the probe screens a subset engine over the
leading --bands-above x 1,024 samples instead; the record says so.

--resources writes the VGPR / AGPR / scratch / LDS / occupancy lines hipcc prints for grm_king.hip.

Usage: python tools/grm_king_probe.py [--sizes 2504x1000000,20000x262144,100000x131072] [--out profiles/NAME.json]
                                      [--resources profiles/NAME.txt]
"""
import argparse
import contextlib
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

from grm_probe import DEFAULT_SIZES, planted_bed  # noqa: E402

BAND = 1024
CUTOFF = 0.177
I8_PEAK_MACS = 32768 / 32 * 1024 * 2.4e9      # per SIMD and cycle x SIMDs x clock


def delta(after, before):
    return dict((k, after[k] - before[k]) for k in after)


def median_of(runs):
    return dict((k, statistics.median(r[k] for r in runs)) for k in runs[0])


def king_once(eng):
    s0 = eng.grm_king_stats()
    t0 = time.perf_counter()
    _, found, rows = eng.grm_king_pairs(CUTOFF, rows="all", band_rows=BAND, capacity=1 << 20)
    wall = time.perf_counter() - t0
    d = delta(eng.grm_king_stats(), s0)
    return {"wall_s": wall, "event_s": d["grm_king_seconds"], "screen_event_s": d["grm_king_screen_seconds"],
            "bands": int(d["grm_king_bands"]), "macs": d["grm_king_macs"], "screen_bytes": int(d["grm_king_bytes"]),
            "n_found": int(found), "rows": int(rows)}


def pairs_once(eng, cutoff):
    s0 = eng.grm_pairs_stats()
    t0 = time.perf_counter()
    _, found = eng.grm_pairs(cutoff, "pairwise", band_rows=BAND, capacity=1 << 20)
    wall = time.perf_counter() - t0
    d = delta(eng.grm_pairs_stats(), s0)
    return {"wall_s": wall, "event_s": d["grm_pairs_seconds"], "n_found": int(found)}


def screen(eng, repeats):
    import numpy as np
    lead = min(eng.n, 2048)
    k = eng.grm_block(0, lead, 0, lead, "pairwise")
    cutoff = float(np.quantile(k[np.triu_indices(lead, 1)], 0.9999))
    king_once(eng)                 # (the first call grows the workspace)
    pairs_once(eng, cutoff)
    kg = median_of([king_once(eng) for _ in range(repeats)])
    gp = median_of([pairs_once(eng, cutoff) for _ in range(repeats)])
    count_s = kg["event_s"] - kg["screen_event_s"]
    return {"n_screened": eng.n, "king": kg, "grm_pairs_pairwise": gp, "grm_pairs_cutoff": cutoff,
            "king_over_grm_pairs_wall": kg["wall_s"] / gp["wall_s"], "screen_share_of_event_time": kg["screen_event_s"] / kg["event_s"],
            "count_kernel_event_s": count_s, "count_macs_per_s": kg["macs"] / count_s,
            "count_share_of_i8_peak": kg["macs"] / count_s / I8_PEAK_MACS}


def planes_path(P, rows, n, repeats):
    """the five-plane path on the same rows: feed, then screen"""
    import torch
    out = {}
    with contextlib.ExitStack() as stack:
        planes = [stack.enter_context(P.PcoaEngine(n)) for _ in range(5)]
        call = 1 << 17
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r0 in range(0, rows.shape[0], call):
            P.PcoaEngine.accumulate_plink_bed_king(planes, rows[r0:r0 + call])
        for e in planes:
            e.sync()
        out["accumulate_wall_s"] = time.perf_counter() - t0
        P.PcoaEngine.king_pairs(planes, CUTOFF, capacity=1 << 20)      # (finalizes the planes)
        walls = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            _, found, v, _ = P.PcoaEngine.king_pairs(planes, CUTOFF, capacity=1 << 20)
            walls.append(time.perf_counter() - t0)
        out.update({"king_pairs_wall_s": statistics.median(walls), "n_found": int(found), "rows": int(v),
                    "matrix_bytes": 5 * 4 * n * n})
    return out


def run_size(P, n, v, seed, triangle_max, bands_above, planes_max, repeats):
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
        out["store_bytes"] = eng.grm_info()[2]
        out["device"] = eng.device_info()[0]
        if n <= triangle_max:
            out["what"] = "the whole triangle, %d bands" % (-(-n // BAND))
            out.update(screen(eng, repeats))
        else:
            lead = bands_above * BAND
            out["what"] = ("the triangle of the leading %d samples (%d bands) as a subset engine: a few bands, not the triangle of N"
                           % (lead, bands_above))
            with eng.grm_subset(np.arange(lead)) as sub:
                out.update(screen(sub, repeats))
    torch.cuda.empty_cache()
    if n <= planes_max:
        out["planes"] = planes_path(P, rows, n, repeats)
        out["planes"]["same_pairs_as_king"] = out["planes"]["n_found"] == out["king"]["n_found"]
        out["king_over_planes_screen_wall"] = out["king"]["wall_s"] / out["planes"]["king_pairs_wall_s"]
    else:
        out["planes"] = "not measured: five N x N int32 matrices above --planes-max"
    return out


def kernel_resources(path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                              "-c", os.path.join(csrc, "grm_king.hip"), "-o", os.path.join(td, "x.o"), "-Rpass-analysis=kernel-resource-usage"],
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
    ap.add_argument("--planes-max", type=int, default=30000, help="largest N at which the five-plane path is run beside it")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None, help="write the compile-time resources of the grm_king.hip kernels here (needs hipcc, no GPU)")
    args = ap.parse_args()
    if args.resources:
        kernel_resources(args.resources)
        if not args.out:
            return 0
    P = importlib.import_module("spark-examples_amd")
    with P.PcoaEngine(256, grm=True) as e:      # code objects, first-use allocations
        e.accumulate_plink_bed(planted_bed(256, 512, args.seed))
        e.grm_king_pairs(CUTOFF)
        e.grm_pairs(0.05, "pairwise")
    doc = {"tool": "tools/grm_king_probe.py", "library": P._lib.load().pcoa_version().decode(), "source_hash": P._lib.source_hash(),
           "i8_peak_macs_per_s": I8_PEAK_MACS, "band_rows": BAND, "min_kinship": CUTOFF, "medians_of": args.repeats,
           "not_measured": ["bands of the full width at N above --triangle-max", "rows used (the probe counts every row)",
                            "the screen's count, scan and write kernels apart", "hardware counters", "a split along variants"],
           "sizes": []}
    for n, v in [tuple(int(t) for t in s.split("x")) for s in args.sizes.split(",")]:
        doc["sizes"].append(run_size(P, n, v, args.seed, args.triangle_max, args.bands_above, args.planes_max, args.repeats))
        print(json.dumps(doc["sizes"][-1]), flush=True)
        if args.out:      # after every size: a later size that fails leaves the earlier ones on file
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

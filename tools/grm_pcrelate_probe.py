#!/usr/bin/env python3
"""PC-Relate kinship on the 2-bit store (pcoa_grm_pcrelate_fit / _pairs) on device-resident .bed rows (not a test, not bench.py).

Per size N x V of tools/grm_probe.py, in one process: the synthetic PLINK rows of that probe are appended to a GRM engine and,
for n_cov in --covariates (a row of ones and the engine's leading n_cov - 1 axes), the probe reports as medians of --repeats
calls after a warm one
  fit              one pcoa_grm_pcrelate_fit: wall clock and HIP-event time, against one product K x on the same store
  pcrelate         one pcoa_grm_pcrelate_pairs(2^-3.5, t = 0.01, band_rows 1,024, capacity 2^20): wall clock, HIP-event time of the
                   dense launches and of the screen, the issued fp64 flop/s of the dense kernel (2 rows cols V per product, three
                   products) and the screen's share
  grm_pairs        one pcoa_grm_pairs(PAIRWISE) on the same store at a cutoff that reports about one pair in 10,000: two products
                   with a trivial decode
pcoa_grm_pcrelate_pairs always walks the whole triangle, so above --triangle-max samples the probe screens a subset engine over
the leading --bands-above x 1,024 samples instead; the record says so.

--resources writes the VGPR / AGPR / scratch / LDS / occupancy lines hipcc prints for grm_pcrelate.hip.

Usage: python tools/grm_pcrelate_probe.py [--sizes 2504x1000000,20000x262144,100000x131072] [--covariates 3,9]
                                          [--out profiles/NAME.json] [--resources profiles/NAME.txt]
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

from grm_probe import DEFAULT_SIZES, planted_bed  # noqa: E402

BAND = 1024
CUTOFF = 2.0 ** -3.5
THRESHOLD = 0.01


def delta(after, before):
    return dict((k, after[k] - before[k]) for k in after)


def median_of(runs):
    return dict((k, statistics.median(r[k] for r in runs)) for k in runs[0])


def fit_once(eng, basis, hat):
    s0 = eng.grm_pcrelate_stats()
    t0 = time.perf_counter()
    eng.grm_pcrelate_fit(basis, hat)
    wall = time.perf_counter() - t0
    return {"wall_s": wall, "event_s": delta(eng.grm_pcrelate_stats(), s0)["grm_pcrelate_fit_seconds"]}


def pcrelate_once(eng):
    s0 = eng.grm_pcrelate_stats()
    t0 = time.perf_counter()
    _, found = eng.grm_pcrelate_pairs(CUTOFF, THRESHOLD, band_rows=BAND, capacity=1 << 20)
    wall = time.perf_counter() - t0
    d = delta(eng.grm_pcrelate_stats(), s0)
    return {"wall_s": wall, "dense_event_s": d["grm_pcrelate_dense_seconds"], "screen_event_s": d["grm_pcrelate_screen_seconds"],
            "bands": int(d["grm_pcrelate_bands"]), "flops": d["grm_pcrelate_flops"], "screen_bytes": int(d["grm_pcrelate_bytes"]),
            "n_found": int(found)}


def pairs_once(eng, cutoff):
    s0 = eng.grm_pairs_stats()
    t0 = time.perf_counter()
    _, found = eng.grm_pairs(cutoff, "pairwise", band_rows=BAND, capacity=1 << 20)
    wall = time.perf_counter() - t0
    return {"wall_s": wall, "event_s": delta(eng.grm_pairs_stats(), s0)["grm_pairs_seconds"], "n_found": int(found)}


def matvec_once(eng, x):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.grm_matvec_device(x)
    torch.cuda.synchronize()
    return {"wall_s": time.perf_counter() - t0}


def screen(P, eng, covariates, repeats):
    import numpy as np
    import torch
    lead = min(eng.n, 2048)
    k = eng.grm_block(0, lead, 0, lead, "pairwise")
    cutoff = float(np.quantile(k[np.triu_indices(lead, 1)], 0.9999))
    pairs_once(eng, cutoff)        # (the first call grows the workspace)
    gp = median_of([pairs_once(eng, cutoff) for _ in range(repeats)])
    x = torch.randn(eng.n, dtype=torch.float64, device="cuda")
    matvec_once(eng, x)
    mv = median_of([matvec_once(eng, x) for _ in range(repeats)])
    comps = eng.compute(max(covariates) - 1)[0] if max(covariates) > 1 else np.zeros((eng.n, 0))
    out = {"n_screened": eng.n, "grm_pairs_pairwise": gp, "grm_pairs_cutoff": cutoff, "matvec": mv, "covariates": []}
    for n_cov in covariates:
        basis = np.ascontiguousarray(np.vstack([np.ones((1, eng.n)), comps[:, :n_cov - 1].T]))
        hat = P.pcrelate_hat(basis)
        fit_once(eng, basis, hat)
        ft = median_of([fit_once(eng, basis, hat) for _ in range(repeats)])
        pcrelate_once(eng)
        pr = median_of([pcrelate_once(eng) for _ in range(repeats)])
        out["covariates"].append({"n_cov": n_cov, "fit": ft, "fit_over_matvec_wall": ft["wall_s"] / mv["wall_s"], "pcrelate": pr,
                                  "pcrelate_over_grm_pairs_wall": pr["wall_s"] / gp["wall_s"],
                                  "dense_flops_per_s": pr["flops"] / pr["dense_event_s"],
                                  "screen_share_of_event_time": pr["screen_event_s"] / (pr["dense_event_s"] + pr["screen_event_s"])})
    return out


def run_size(P, n, v, seed, triangle_max, bands_above, covariates, repeats):
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
            out.update(screen(P, eng, covariates, repeats))
        else:
            lead = bands_above * BAND
            out["what"] = ("the triangle of the leading %d samples (%d bands) as a subset engine: a few bands, not the triangle of N"
                           % (lead, bands_above))
            with eng.grm_subset(np.arange(lead)) as sub:
                out.update(screen(P, sub, covariates, repeats))
    torch.cuda.empty_cache()
    return out


def kernel_resources(path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                              "-c", os.path.join(csrc, "grm_pcrelate.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"],
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
    ap.add_argument("--covariates", default="3,9", help="comma-separated covariate counts (an intercept and n_cov - 1 axes)")
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--triangle-max", type=int, default=30000, help="largest N whose whole triangle is screened")
    ap.add_argument("--bands-above", type=int, default=8, help="bands of 1,024 samples screened above --triangle-max")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None, help="write the compile-time resources of the grm_pcrelate.hip kernels here (needs hipcc, no GPU)")
    args = ap.parse_args()
    if args.resources:
        kernel_resources(args.resources)
        if not args.out:
            return 0
    covariates = [int(t) for t in args.covariates.split(",")]
    P = importlib.import_module("spark-examples_amd")
    import numpy as np
    with P.PcoaEngine(256, grm=True) as e:      # code objects, first-use allocations
        e.accumulate_plink_bed(planted_bed(256, 512, args.seed))
        e.grm_pcrelate_fit(np.ones((1, 256)))
        e.grm_pcrelate_pairs(CUTOFF)
        e.grm_pairs(0.05, "pairwise")
    doc = {"tool": "tools/grm_pcrelate_probe.py", "library": P._lib.load().pcoa_version().decode(), "source_hash": P._lib.source_hash(),
           "band_rows": BAND, "cutoff": CUTOFF, "maf_threshold": THRESHOLD, "medians_of": args.repeats,
           "not_measured": ["bands of the full width at N above --triangle-max", "the dense kernel's three products apart",
                            "the screen's count, scan and write kernels apart", "hardware counters (VALU against MFMA issue)"],
           "sizes": []}
    for n, v in [tuple(int(t) for t in s.split("x")) for s in args.sizes.split(",")]:
        doc["sizes"].append(run_size(P, n, v, args.seed, args.triangle_max, args.bands_above, covariates, args.repeats))
        print(json.dumps(doc["sizes"][-1]), flush=True)
        if args.out:      # after every size: a later size that fails leaves the earlier ones on file
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""The LD prune of a GRM engine's resident store (pcoa_grm_ld_prune) on device-resident .bed rows (not a test, not bench.py).

Per size N x V, in one process: the planted cohort of tools/grm_probe.py (three populations, Hardy-Weinberg genotypes, 3 %
missing calls, generated on the GPU from a fixed seed; its variants are independent, so nearly every candidate is kept -- the
band kernel's work does not depend on that, the resolve wave's barely) is appended to a GRM engine, and the probe reports
  prune wall      one pcoa_grm_ld_prune (window 50, r2 0.2), wall clock around the synchronising call: the counts and weights are
                  resident, so this is the copies into the work buffer, reach + band, resolve, scan and the hand-over of the mask
  band / resolve / scan   the HIP-event times of that call (pcoa_get_grm_ld_stats)
beside
  (a) carrier band   ld_band_seconds of pcoa_ld_plink_bed as a dry run over the SAME rows with the same window (the carrier-indicator
                  band kernel of ld.hip, the closest existing yardstick), and the ratio of the two band times
  (b) grm product    one pcoa_grm_matvec_device on the same store (median of five after one warm call)
and holds the mask of the first --check-rows rows against the numpy statement of the rule on that slice (a forward pass: the
mask of a prefix is the prune of the prefix).  --resources writes the VGPR / AGPR / LDS / scratch lines hipcc prints for grm_ld.hip.

Usage: python tools/grm_ld_probe.py [--sizes 2504x1000000,20000x262144,100000x131072] [--window 50] [--r2 0.2]
                                    [--out profiles/NAME.json] [--resources profiles/NAME.txt]
"""
import argparse
import importlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from grm_probe import DEFAULT_SIZES, planted_bed, timed  # noqa: E402


def slice_rule(bed, n, window, t):
    """The keep mask of pcoa_grm_ld_prune for the rows of `bed` ([S][ceil(n / 4)] uint8, A2 the reference allele) alone, min_maf 0.
    The six sums of every pair come from float64 matrix products (exact: every sum is an integer below 2^53)."""
    codes = ((bed[:, :, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(bed.shape[0], -1)[:, :n]
    c = (codes != 1).astype(np.float64)
    x = (codes == 2).astype(np.float64) + 2.0 * (codes == 0).astype(np.float64)
    as_int = lambda m: np.rint(m).astype(np.int64)
    nn, s, q, p = as_int(c @ c.T), as_int(x @ c.T), as_int((x * x) @ c.T), as_int(x @ x.T)
    cov = nn * p - s * s.T
    var_u, var_v = nn * q - s * s, nn * q.T - s.T * s.T
    ex = cov.astype(np.float64) * cov.astype(np.float64) > t * (var_u.astype(np.float64) * var_v.astype(np.float64))
    called, a = c.sum(axis=1).astype(np.int64), x.sum(axis=1).astype(np.int64)
    cand = (called > 0) & (a > 0) & (a < 2 * called)
    keep = np.zeros(bed.shape[0], dtype=bool)
    for r in range(bed.shape[0]):
        lo = max(0, r - window)
        keep[r] = cand[r] and not np.any(keep[lo:r] & ex[lo:r, r])
    return keep


def run_size(P, n, v, seed, window, r2, check_rows):
    import torch
    rows = planted_bed(n, v, seed)
    call = 1 << 20
    x = torch.randn(n, dtype=torch.float64, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(seed + 1))
    out = {"n": n, "v": v, "window": window, "r2": r2}
    with P.PcoaEngine(n, grm=True) as eng:
        for r0 in range(0, v, call):
            eng.accumulate_plink_bed(rows[r0:r0 + call])
        eng.sync()
        out["used_unpruned"] = eng.grm_info()[1]           # the counts and weights are resident from here on
        eng.grm_ld_prune(window, r2)                        # warm: code objects, first-use allocations
        eng.reset_timings()
        t0 = time.perf_counter()
        cand, kept = eng.grm_ld_prune(window, r2)
        out["prune_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        st = eng.grm_ld_stats()
        out.update(candidates=cand, kept=kept, pairs=st["grm_ld_pairs"], band_ms=1e3 * st["grm_ld_band_seconds"],
                   resolve_ms=1e3 * st["grm_ld_resolve_seconds"], scan_ms=1e3 * st["grm_ld_scan_seconds"])
        out["resolve_ns_per_row"] = 1e9 * st["grm_ld_resolve_seconds"] / v
        out["band_ps_per_pair_sample"] = 1e12 * st["grm_ld_band_seconds"] / (float(st["grm_ld_pairs"]) * n)
        s = min(check_rows, v)
        want = slice_rule(rows[:s].cpu().numpy(), n, window, r2)
        out.update(check_rows=s, check_kept=int(want.sum()), check_equal=bool(np.array_equal(eng.grm_ld_mask(0, s), want)))
        assert eng.grm_info()[1] == kept
        eng.grm_ld_clear()
        out["grm_product_ms"] = 1e3 * timed(lambda: eng.grm_matvec_device(x))
        out["device"] = eng.device_info()[0]
    with P.PcoaEngine(n, operator=True) as op:              # (any kind of ctx serves the carrier pruner; this one holds no S)
        for warm in (True, False):
            with op.ld_pruner(window, r2, accumulate=False) as pr:
                op.reset_timings()
                t0 = time.perf_counter()
                for r0 in range(0, v, call):
                    pr.plink_bed(rows[r0:r0 + call])
                wall = time.perf_counter() - t0
                ls = pr.stats()
        out.update(carrier_dry_run_wall_ms=1e3 * wall, carrier_band_ms=1e3 * ls["ld_band_seconds"],
                   carrier_resolve_ms=1e3 * ls["ld_resolve_seconds"], carrier_kept=ls["ld_kept"], carrier_pairs=ls["ld_pairs"])
    out["band_over_carrier_band"] = out["band_ms"] / out["carrier_band_ms"]
    out["prune_wall_over_grm_product"] = out["prune_wall_ms"] / out["grm_product_ms"]
    return out


def kernel_resources(path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                              "-c", os.path.join(csrc, "grm_ld.hip"), "-o", os.path.join(td, "x.o"), "-Rpass-analysis=kernel-resource-usage"],
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
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--r2", type=float, default=0.2)
    ap.add_argument("--check-rows", type=int, default=256)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None, help="write the compile-time resources of the grm_ld.hip kernels here (needs hipcc, no GPU)")
    args = ap.parse_args()
    if args.resources:
        kernel_resources(args.resources)
        if not args.out:
            return 0
    P = importlib.import_module("spark-examples_amd")
    doc = {"tool": "tools/grm_ld_probe.py", "library": P._lib.load().pcoa_version().decode(), "source_hash": P._lib.source_hash(),
           "input": "device-resident rows, one input form; host rows were not timed", "sizes": []}
    for n, v in [tuple(int(t) for t in s.split("x")) for s in args.sizes.split(",")]:
        doc["sizes"].append(run_size(P, n, v, args.seed, args.window, args.r2, args.check_rows))
        print(json.dumps(doc["sizes"][-1]), flush=True)
        if args.out:      # after every size: a later size that fails leaves the earlier ones on file
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

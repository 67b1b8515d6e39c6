#!/usr/bin/env python3
"""The standardised-genotype operator (pcoa_create_grm) on device-resident .bed rows (not a test, not bench.py).

Per size N x V, in one process: synthetic PLINK rows with planted population structure (three populations, Hardy-Weinberg
genotypes, 3 % missing calls, generated on the GPU from a fixed seed) are appended to a GRM engine, and the probe times, as
wall clock around calls that end in a synchronise,
  append          pcoa_accumulate_plink_bed of the device rows, in calls of 2^20 rows, to pcoa_sync
  counts          the first pcoa_grm_info: the per-variant counts, the weights and M'
  grm product     one pcoa_grm_matvec_device (median of five after one warm call)
  operator product one pcoa_operator_matvec_device (uncentred) of an operator engine fed the SAME rows, whose carrier bitsets
                  the .bed decode makes of them (median of five after one warm call)
  compute(2)      pcoa_compute wall and its Lanczos steps
and reports the GRM product against the V N / 4 bytes one pass reads at the 6.29 TB/s measured copy ceiling (a product is two
passes).  --resources writes the VGPR / scratch / occupancy lines hipcc prints for grm_bits.hip.

Usage: python tools/grm_probe.py [--sizes 2504x1000000,20000x262144,100000x131072] [--out profiles/NAME.json]
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

COPY_CEILING = 6.29e12   # bytes/s, the measured device copy ceiling the documents quote
DEFAULT_SIZES = "2504x1000000,20000x262144,100000x131072"


def planted_bed(n, v, seed, chunk_elems=1 << 28):
    """[v][ceil(n / 4)] uint8 .bed rows on cuda:0, A2 the reference allele: per variant an ancestral frequency U(0.1, 0.9), per
    population that frequency moved by N(0, 0.1) and clipped to [0.02, 0.98]; code 00 = two copies, 10 = one, 11 = none, 01 =
    missing at rate 0.03."""
    import torch
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    nb = (n + 3) // 4
    pops = torch.clamp((torch.arange(nb * 4, device=dev) * 3) // n, max=2)
    shifts = torch.tensor([1, 4, 16, 64], dtype=torch.int32, device=dev).view(1, 1, 4)
    out = torch.empty((v, nb), dtype=torch.uint8, device=dev)
    rows = max(1, min(v, chunk_elems // (nb * 4)))
    for r0 in range(0, v, rows):
        r = min(rows, v - r0)
        p = 0.1 + 0.8 * torch.rand((r, 1), generator=gen, device=dev)
        f = torch.clamp(p + 0.1 * torch.randn((r, 3), generator=gen, device=dev), 0.02, 0.98)[:, pops]
        g = (torch.rand((r, nb * 4), generator=gen, device=dev) < f).to(torch.int32) + \
            (torch.rand((r, nb * 4), generator=gen, device=dev) < f).to(torch.int32)
        codes = 3 - g - (g == 2).to(torch.int32)      # 0 copies -> 11, 1 -> 10, 2 -> 00
        codes[torch.rand((r, nb * 4), generator=gen, device=dev) < 0.03] = 1
        out[r0:r0 + r] = (codes.view(r, nb, 4) * shifts).sum(dim=2).to(torch.uint8)
        del p, f, g, codes
    torch.cuda.synchronize()
    return out


def timed(fn, repeats=5):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def run_size(P, n, v, seed):
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
        t0 = time.perf_counter()
        variants, used, store = eng.grm_info()
        out["counts_s"] = time.perf_counter() - t0
        out.update(variants=variants, used=used, store_bytes=store)
        per = timed(lambda: eng.grm_matvec_device(x))
        one_pass = v * n / 4.0
        out.update(grm_product_ms=1e3 * per, one_pass_bytes=one_pass, one_pass_at_copy_ceiling_ms=1e3 * one_pass / COPY_CEILING,
                   product_over_two_passes_at_ceiling=per / (2 * one_pass / COPY_CEILING),
                   masked_adds_per_second=6.0 * v * n / per)
        t0 = time.perf_counter()
        comps, lam, nz = eng.compute(2)
        out["compute2_wall_s"] = time.perf_counter() - t0
        t = eng.timings()
        out.update(lanczos_steps=t["lanczos_steps"], products=t["operator_products"], eigenvalues=[float(a) for a in lam],
                   nonzero_rows=nz, device=eng.device_info()[0])
    with P.PcoaEngine(n, operator=True) as op:
        for r0 in range(0, v, call):
            op.accumulate_plink_bed(rows[r0:r0 + call])
        op.sync()
        out["operator_product_ms"] = 1e3 * timed(lambda: op.operator_matvec_device(x, False))
        out["operator_store_bytes"] = op.operator_info()[1]
    out["grm_over_operator_product"] = out["grm_product_ms"] / out["operator_product_ms"]
    return out


def kernel_resources(path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                              "-c", os.path.join(csrc, "grm_bits.hip"), "-o", os.path.join(td, "x.o"), "-Rpass-analysis=kernel-resource-usage"],
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None, help="write the compile-time resources of the grm_bits.hip kernels here (needs hipcc, no GPU)")
    args = ap.parse_args()
    if args.resources:
        kernel_resources(args.resources)
        if not args.out:
            return 0
    P = importlib.import_module("spark-examples_amd")
    with P.PcoaEngine(256, grm=True) as e:      # code objects, first-use allocations
        e.accumulate_plink_bed(planted_bed(256, 512, args.seed))
        e.compute(2)
    doc = {"tool": "tools/grm_probe.py", "library": P._lib.load().pcoa_version().decode(), "source_hash": P._lib.source_hash(),
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

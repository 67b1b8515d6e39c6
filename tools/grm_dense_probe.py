#!/usr/bin/env python3
"""Reading K out (pcoa_grm_block) on device-resident .bed rows (not a test, not bench.py).

Per size N x V, in one process: the synthetic PLINK rows of tools/grm_probe.py are appended to a GRM engine, and the probe
times, as wall clock around synchronising calls, median of three after one warm call,
  triangle        the lower triangle of K in blocks of --block (4,096) rows and columns into DEVICE memory, divisor "used", once
                  without and once with out_pairs (the second MFMA pass for n(i, j))
  one block       at N > --triangle-max (60,000) the full triangle is minutes: one --block^2 block strictly below the diagonal
                  and the one on the diagonal instead (the diagonal block runs both forms of the symmetry construction)
  compute(2)      pcoa_compute wall on the same store, for scale
and reports the algorithmic rate 2 rows cols V / seconds per pass.  The microarchitecture notes at hand give no fp64 matrix
figure; the record holds the rate against --peak-flop-per-clk-simd (32, the figure the instruction's 64-cycle issue of 2,048 FLOP
implies) x SIMDs x the device's reported clock, and says that this ceiling is derived, not measured.  What the probe does NOT
measure: the num and n passes apart inside one launch, host-pointer output at size, hardware counters.
--resources writes the VGPR / AGPR / scratch / occupancy lines hipcc prints for grm_dense.hip.

Usage: python tools/grm_dense_probe.py [--sizes 2504x1000000,20000x262144,100000x131072] [--out profiles/NAME.json]
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

DEFAULT_SIZES = "2504x1000000,20000x262144,100000x131072"


def timed(fn, repeats=3):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def lower_blocks(n, block):
    return [(r0, min(block, n - r0), c0, min(block, n - c0)) for r0 in range(0, n, block) for c0 in range(0, r0 + 1, block)]


def run_size(P, n, v, seed, block, triangle_max, peak):
    import torch
    from grm_probe import planted_bed
    rows = planted_bed(n, v, seed)
    call = 1 << 20
    out = {"n": n, "v": v, "block": block}
    with P.PcoaEngine(n, grm=True) as eng:
        eng.reserve(min(v, call), 2)
        for r0 in range(0, v, call):
            eng.accumulate_plink_bed(rows[r0:r0 + call])
        eng.sync()
        del rows
        variants, used, store = eng.grm_info()
        out.update(variants=variants, used=used, store_bytes=store, device=eng.device_info()[0])
        if n <= triangle_max:
            what = {"triangle": lower_blocks(n, block)}
        else:
            what = {"block_below_diagonal": [(block, block, 0, block)], "block_on_diagonal": [(block, block, block, block)]}
        for name, rects in what.items():
            entries = sum(r * c for (_, r, _, c) in rects)
            for pairs in (False, True):
                def go():
                    for (r0, r, c0, c) in rects:
                        eng.grm_block(r0, r, c0, c, "used", pairs=pairs, device=True)
                per = timed(go)
                passes = 2 if pairs else 1
                flops = 2.0 * entries * v * passes
                key = name + ("_with_pairs" if pairs else "")
                out[key] = {"blocks": len(rects), "entries": entries, "seconds": per, "float_passes": passes,
                            "algorithmic_flop_per_s": flops / per, "share_of_derived_peak": flops / per / peak}
        st = eng.grm_block_stats()
        out["stats"] = st
        t0 = time.perf_counter()
        comps, lam, nz = eng.compute(2)
        out["compute2_wall_s"] = time.perf_counter() - t0
        out["eigenvalues"] = [float(a) for a in lam]
    return out


def kernel_resources(path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                              "-c", os.path.join(csrc, "grm_dense.hip"), "-o", os.path.join(td, "x.o"), "-Rpass-analysis=kernel-resource-usage"],
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
    ap.add_argument("--block", type=int, default=4096)
    ap.add_argument("--triangle-max", type=int, default=60000, help="largest N whose whole lower triangle is timed")
    ap.add_argument("--peak-flop-per-clk-simd", type=float, default=32.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None, help="write the compile-time resources of the grm_dense.hip kernels here (needs hipcc, no GPU)")
    args = ap.parse_args()
    if args.resources:
        kernel_resources(args.resources)
        if not args.out:
            return 0
    import torch
    from grm_probe import planted_bed
    P = importlib.import_module("spark-examples_amd")
    props = torch.cuda.get_device_properties(0)
    clock_hz = 1e3 * float(getattr(props, "clock_rate", 0) or 2.4e6)
    simds = 4 * props.multi_processor_count
    peak = args.peak_flop_per_clk_simd * simds * clock_hz
    with P.PcoaEngine(256, grm=True) as e:      # code objects, first-use allocations
        e.accumulate_plink_bed(planted_bed(256, 512, args.seed))
        e.grm_block(0, 256, 0, 256, "pairwise", pairs=True, device=True)
    doc = {"tool": "tools/grm_dense_probe.py", "library": P._lib.load().pcoa_version().decode(), "source_hash": P._lib.source_hash(),
           "derived_fp64_matrix_peak_flop_per_s": peak, "peak_is": "%g FLOP/clk/SIMD x %d SIMDs x %.0f MHz reported clock: derived, "
           "not measured" % (args.peak_flop_per_clk_simd, simds, clock_hz / 1e6),
           "not_measured": ["the num and n passes apart inside one launch", "host-pointer output at size", "hardware counters"],
           "sizes": []}
    for n, v in [tuple(int(t) for t in s.split("x")) for s in args.sizes.split(",")]:
        doc["sizes"].append(run_size(P, n, v, args.seed, args.block, args.triangle_max, peak))
        print(json.dumps(doc["sizes"][-1]), flush=True)
        if args.out:      # after every size: a later size that fails leaves the earlier ones on file
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

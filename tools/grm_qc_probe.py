#!/usr/bin/env python3
"""Variant and sample QC on a GRM store (pcoa_grm_sample_counts, pcoa_grm_hwe) on device-resident .bed rows (not a test, not
bench.py).

Per size N x V of tools/grm_probe.py, in one process: the synthetic PLINK rows of that probe are appended to a GRM engine, and
the probe reports, as HIP-event time out of the engine's own statistics (median of three calls after one warm call),
  sample counts    one pcoa_grm_sample_counts(ALL): the segment launches and the finish (pcoa_get_grm_qc_stats), as a share of
                   the 6.29 TB/s measured copy ceiling on V x pitch bytes, and against
  product          one pcoa_grm_matvec_device on the same store (operator_matvec_seconds of pcoa_get_timings): the kernels of
                   the product are the yardstick, two passes over the same bytes
  hwe              the one launch of the HWE kernel over the V rows (the engine is reset and fed again for every repeat: the
                   p-values are resident beside the counts), and against
  counts           the wall clock of the first pcoa_grm_counts behind the same feed, which runs the counts kernel
--resources writes the VGPR / scratch / occupancy lines hipcc prints for grm_qc.hip.

Usage: python tools/grm_qc_probe.py [--sizes 2504x1000000,20000x262144,100000x131072] [--out profiles/NAME.json]
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


def event_median(call, read, repeats=3):
    """median over `repeats` calls, after one warm call, of the growth of read() across call()"""
    got = []
    for k in range(repeats + 1):
        a = read()
        call()
        b = read()
        if k > 0:
            got.append(b - a)
    return statistics.median(got)


def run_size(P, n, v, seed):
    import torch
    rows = planted_bed(n, v, seed)
    call = 1 << 20
    x = torch.randn(n, dtype=torch.float64, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(seed + 1))
    out = {"n": n, "v": v}

    def feed(eng):
        for r0 in range(0, v, call):
            eng.accumulate_plink_bed(rows[r0:r0 + call])
        eng.sync()

    with P.PcoaEngine(n, grm=True) as eng:
        feed(eng)
        variants, used, store = eng.grm_info()
        pitch = ((n + 3) // 4 + 15) // 16 * 16
        out.update(variants=variants, used=used, store_bytes=store, pass_bytes=v * pitch, device=eng.device_info()[0])
        sc = event_median(lambda: eng.grm_sample_counts(), lambda: eng.grm_qc_stats()["grm_qc_sample_counts_seconds"])
        scu = event_median(lambda: eng.grm_sample_counts(used=True), lambda: eng.grm_qc_stats()["grm_qc_sample_counts_seconds"])
        pr = event_median(lambda: eng.grm_matvec_device(x), lambda: eng.timings()["operator_matvec_seconds"])
        counts = eng.grm_sample_counts()
        out.update(sample_counts_ms=1e3 * sc, sample_counts_used_ms=1e3 * scu, grm_product_ms=1e3 * pr,
                   sample_counts_over_product=sc / pr, sample_counts_bytes_per_s=v * pitch / sc,
                   sample_counts_share_of_copy_ceiling=v * pitch / sc / COPY_CEILING,
                   mean_call_rate=float(counts[:, 0].mean()) / v)
        hwe, cnt = [], []
        for k in range(4):
            eng.reset()
            feed(eng)
            t0 = time.perf_counter()
            eng.grm_counts(0, 1)
            w = time.perf_counter() - t0
            a = eng.grm_qc_stats()["grm_qc_hwe_seconds"]
            p = eng.grm_hwe()
            b = eng.grm_qc_stats()["grm_qc_hwe_seconds"]
            if k > 0:
                hwe.append(b - a)
                cnt.append(w)
        out.update(hwe_ms=1e3 * statistics.median(hwe), counts_wall_ms=1e3 * statistics.median(cnt),
                   hwe_over_counts=statistics.median(hwe) / statistics.median(cnt), hwe_p_below_1e_6=int((p < 1e-6).sum()))
    return out


def kernel_resources(path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                              "-c", os.path.join(csrc, "grm_qc.hip"), "-o", os.path.join(td, "x.o"), "-Rpass-analysis=kernel-resource-usage"],
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
    ap.add_argument("--resources", default=None, help="write the compile-time resources of the grm_qc.hip kernels here (needs hipcc, no GPU)")
    args = ap.parse_args()
    if args.resources:
        kernel_resources(args.resources)
        if not args.out:
            return 0
    P = importlib.import_module("spark-examples_amd")
    with P.PcoaEngine(256, grm=True) as e:      # code objects, first-use allocations
        e.accumulate_plink_bed(planted_bed(256, 512, args.seed))
        e.grm_sample_counts()
        e.grm_hwe()
    doc = {"tool": "tools/grm_qc_probe.py", "library": P._lib.load().pcoa_version().decode(), "source_hash": P._lib.source_hash(),
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

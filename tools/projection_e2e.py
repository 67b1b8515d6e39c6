#!/usr/bin/env python3
"""pcoa_project at the size of a panel and a study: N_ref reference samples, N_new samples to place, synthetic genotypes
(the engine's Philox model, five populations; the new samples join the last one) generated on the GPU for both engines from
the same counters, so a sample's genotypes do not depend on which engine draws them.

One JSON line: the wall time from the first accumulate call to the coordinates on the host (accumulate + finalize of both
engines, pcoa_compute on the reference, pcoa_project), each stage's wall time, and -- from a SEPARATE run of the same job
under `rocprofv3 --kernel-trace --stats` (--profile) -- the kernel time of the projection pass (the column sums over rows
[0, N_ref) of the strip, the projection kernel, their finish kernels) and its share of 8 TB/s on its algorithmic bytes:
4 N_ref N_new for the column sums, the same again per chunk of components, plus the N_ref-double vectors.
usage: tools/projection_e2e.py [--ref N] [--new M] [--variants V] [--num-pc K] [--profile] [--json out.json]"""
import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
PASS_KERNELS = ("project_band_kernel", "project_finish_kernel", "strip_band_kernel<false", "strip_finish_kernel<false")


def run_job(n_ref, n_new, variants, num_pc, seed=7):
    E = importlib.import_module("spark-examples_amd.engine")
    synth = importlib.import_module("spark-examples_amd.synth")
    n = n_ref + n_new
    offs_ref = [n_ref * p // 5 for p in range(6)]
    offs_all = offs_ref[:5] + [n]
    ref = E.PcoaEngine(n_ref)
    cross = E.PcoaEngine(n, strip=(n_ref, n_new))
    chunk = 1 << 14
    ref.reserve(chunk, num_pc)
    cross.reserve(chunk, 0)
    thr = [synth.thresholds(seed, v0, min(chunk, variants - v0)) for v0 in range(0, variants, chunk)]
    t = {}
    t0 = time.perf_counter()
    for k, v0 in enumerate(range(0, variants, chunk)):
        ref.accumulate_synthetic(seed, offs_ref, thr[k], v0)
        cross.accumulate_synthetic(seed, offs_all, thr[k], v0)
    ref.finalize()
    cross.finalize()
    t1 = time.perf_counter()
    comps, lam, _ = ref.compute(num_pc)
    t2 = time.perf_counter()
    coords = ref.project(cross, comps, lam)
    t3 = time.perf_counter()
    t.update(accumulate_finalize_s=t1 - t0, compute_s=t2 - t1, project_s=t3 - t2, first_accumulate_to_coordinates_s=t3 - t0)
    # a spot check that costs nothing: a new sample of population 4 lies nearer to population 4's reference samples
    # than to population 0's on PC1 or PC2 (not a correctness test; tests/test_gpu_projection.py holds those)
    cen = [comps[offs_ref[p]:offs_ref[p + 1]].mean(axis=0) for p in (0, 4)]
    near = float(np.mean(np.linalg.norm(coords - cen[1], axis=1) < np.linalg.norm(coords - cen[0], axis=1)))
    ref.close()
    cross.close()
    return t, dict(eigenvalues=[float(x) for x in lam], new_samples_nearer_their_population=near)


def pass_bytes(n_ref, n_new, num_pc):
    chunks, left = 0, num_pc
    while left > 0:
        left -= 8 if left >= 8 else 4 if left >= 4 else 2 if left >= 2 else 1
        chunks += 1
    strip = 4.0 * n_ref * n_new * (1 + chunks)
    vectors = 8.0 * n_ref * (1 + num_pc) * chunks
    return strip + vectors, chunks


def profile(args):
    """The same job under rocprofv3 --kernel-trace --stats in a child process; the projection pass's kernels summed."""
    d = tempfile.mkdtemp(prefix="proj_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
               "--ref", str(args.ref), "--new", str(args.new), "--variants", str(args.variants), "--num-pc", str(args.num_pc)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=1800)
        if res.returncode != 0:
            return {"error": "rocprofv3 run failed (exit %d): %s" % (res.returncode, res.stderr[-1500:])}
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            return {"error": "no kernel_stats.csv"}
        per = {}
        with open(stats[0]) as f:
            for row in csv.DictReader(f):
                for key in PASS_KERNELS:
                    if key in row["Name"]:
                        per[key] = dict(calls=int(row["Calls"]), total_ns=float(row["TotalDurationNs"]))
        return per
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", type=int, default=100000)
    ap.add_argument("--new", type=int, default=10000)
    ap.add_argument("--variants", type=int, default=16384)
    ap.add_argument("--num-pc", type=int, default=2)
    ap.add_argument("--profile", action="store_true", help="also run the job under rocprofv3 (separate process)")
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args()
    t, check = run_job(a.ref, a.new, a.variants, a.num_pc)
    byts, chunks = pass_bytes(a.ref, a.new, a.num_pc)
    out = dict(tool="projection_e2e", n_ref=a.ref, n_new=a.new, variants=a.variants, num_pc=a.num_pc, k_chunks=chunks,
               wall=t, check=check, pass_algorithmic_bytes=byts,
               pass_kernel_seconds="not measured", pass_share_of_8TBps="not measured")
    if a.profile:
        per = profile(a)
        out["pass_kernels"] = per
        if "error" not in per and "project_band_kernel" in per:
            ks = sum(v["total_ns"] for v in per.values()) * 1e-9
            out["pass_kernel_seconds"] = ks
            out["pass_share_of_8TBps"] = byts / ks / HBM_BYTES_PER_S
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

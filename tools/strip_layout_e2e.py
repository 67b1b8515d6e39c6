#!/usr/bin/env python3
"""The compiled host's strip layout at large N, end to end: a synthetic PLINK fileset (V variants x N samples, three
populations with their own carrier rates so that the top eigenpairs are well separated; codes drawn on the GPU) through
  variants_pca_driver --input-path <prefix>.bed --layout strips --gpus K --gpu-map <devices>
and one JSON line with what the run reports: the wall time of the process, ingest -> finalized strips, the Gram kernels
summed over the owners, the computePca time, its Lanczos steps and the time per step (computePca / steps: one product over
every owner plus the Lanczos work of that step -- the product alone is not timed separately).  `owners_share_one_gpu`
says whether the owners sat on one device.
usage: tools/strip_layout_e2e.py [--samples N] [--variants V] [--owners K] [--gpu-map 0,0,..] [--json out.json]"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_fileset(prefix, n, v, seed=11):
    bpv = (n + 3) // 4
    with open(prefix + ".fam", "w") as f:
        f.write("".join("F%d S%06d 0 0 0 -9\n" % (i, i) for i in range(n)))
    with open(prefix + ".bim", "w") as f:
        f.write("".join("1\trs%d\t0\t%d\tC\tA\n" % (k, 1000 + 10 * k) for k in range(v)))
    g = torch.Generator(device="cuda").manual_seed(seed)
    pop = (torch.arange(bpv * 4, device="cuda") * 3 // n).clamp(max=2)          # three contiguous populations
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6c, 0x1b, 0x01]))
        for c0 in range(0, v, 4096):
            rows = min(4096, v - c0)
            u = torch.rand((rows, bpv * 4), device="cuda", generator=g)
            which = torch.randint(0, 4, (rows, 1), device="cuda", generator=g)     # 3: no population-specific rate
            p = torch.where(pop[None, :] == which, 0.4, 0.05)
            codes = torch.full((rows, bpv * 4), 3, dtype=torch.uint8, device="cuda")   # hom A2 = reference
            codes[u < p] = 2                                                   # het
            codes[u < p * 0.2] = 0                                             # hom A1
            codes[:, n:] = 3
            q = codes.view(rows, bpv, 4)
            f.write((q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).cpu().numpy().tobytes())
    return bpv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--variants", type=int, default=32768)
    ap.add_argument("--owners", type=int, default=4)
    ap.add_argument("--gpu-map", type=str, default=None, help="device of each owner (default: all on device 0)")
    ap.add_argument("--stream-rows", type=int, default=8192)
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args()
    gpu_map = a.gpu_map or ",".join(["0"] * a.owners)
    d = tempfile.mkdtemp(prefix="strip_e2e_")
    try:
        prefix = os.path.join(d, "cohort")
        t0 = time.perf_counter()
        bpv = write_fileset(prefix, a.samples, a.variants)
        write_s = time.perf_counter() - t0
        torch.cuda.empty_cache()
        exe = os.path.join(ROOT, "spark-examples_amd", "variants_pca_driver")
        cmd = [exe, "--input-path", prefix + ".bed", "--all-references", "--layout", "strips", "--gpus", str(a.owners),
               "--gpu-map", gpu_map, "--stream-rows", str(a.stream_rows)]
        t1 = time.perf_counter()
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=3000)
        wall = time.perf_counter() - t1
    finally:
        shutil.rmtree(d, ignore_errors=True)
    if res.returncode != 0:
        sys.stderr.write(res.stderr[-4000:])
        return 1
    err = res.stderr
    ingest = re.search(r"Streamed (\d+) variants x (\d+) samples .* in ([0-9.]+) s", err)
    gram = re.search(r"Gram kernel ([0-9.]+) ms; PCoA ([0-9.]+) ms", err)
    steps = re.search(r"(\d+) Lanczos steps", err)
    layout = re.search(r"strip layout: [^;]*; columns ((?:\[\d+, \d+\) on device \d+(?:, )?)+)", err)
    nz = re.search(r"Non zero rows in matrix: (\d+)", res.stdout)
    pcoa_ms = float(gram.group(2))
    n_steps = int(steps.group(1))
    devices = sorted(set(int(t) for t in gpu_map.split(",")))
    rec = {
        "workload": "compiled host, --layout strips: synthetic PLINK fileset %d variants x %d samples (3 populations), %d owners"
                    % (a.variants, a.samples, a.owners),
        "owners": a.owners, "gpu_map": gpu_map, "owners_share_one_gpu": len(devices) == 1,
        "device": torch.cuda.get_device_name(devices[0]),
        "bed_bytes": 3 + a.variants * bpv, "fileset_write_s": write_s,
        "wall_s": wall,
        "ingest_to_strips_s": float(ingest.group(3)) if ingest else None,
        "gram_kernel_s_summed_over_owners": float(gram.group(1)) / 1e3,
        "compute_pca_s": pcoa_ms / 1e3,
        "lanczos_steps": n_steps,
        "per_step_ms": pcoa_ms / max(n_steps, 1),
        "per_step_note": "computePca wall / Lanczos steps: one product over every owner + that step's Lanczos work",
        "nonzero_rows": int(nz.group(1)) if nz else None,
        "columns": layout.group(1) if layout else None,
    }
    line = json.dumps(rec)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

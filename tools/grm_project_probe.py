#!/usr/bin/env python3
"""SNP weights and projection on a GRM engine (pcoa_grm_weights, pcoa_grm_project) against the one-vector product (not a test,
not bench.py).

Per size N x V, in one process: the synthetic PLINK rows of tools/grm_probe.py are appended to a GRM engine (the panel) and a
second draw of the same shape to a GRM study store, and the probe times, as wall clock around calls that end in a synchronise
(median of five after one warm call), for num_pc = 1, 2 and 8 with random unit "components" and eigenvalues 1:
  weights         pcoa_grm_weights, unscaled, a window of 1,024 rows (all of t is computed; the window keeps the copy to the host
                  out of the figure): ceil(num_pc / 2) first passes over the panel's rows, num_pc combine launches
  project         pcoa_grm_project with the called count: the same first passes, then ceil(num_pc / 2) second passes over the
                  study's rows and one integer pass
  product         one pcoa_grm_matvec_device on the panel's store, and one on a GRM engine that holds the study's rows: a first
                  and a second pass over one vector each
The passes cannot be timed apart through the public calls.  What can be compared: project(num_pc = 2) runs one two-vector first
pass over the panel and one two-vector second pass over the study where two products run two one-vector passes of each kind, so
`project_k2_over_two_products` < 1 says that decoding a word once for two vectors beats decoding it twice; weights(2) against
two products bounds the first pass's share from above.  --resources writes the lines hipcc prints for grm_multi.hip.

Usage: python tools/grm_project_probe.py [--sizes 2504x1000000,20000x262144,100000x131072] [--out profiles/NAME.json]
                                         [--resources profiles/NAME.txt]
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from grm_probe import DEFAULT_SIZES, planted_bed, timed   # noqa: E402


def run_size(P, n, v, seed):
    import torch
    call = 1 << 20
    rng = np.random.default_rng(seed)
    out = {"n": n, "v": v, "num_pc": {}}
    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(n, grm_study=True) as st, P.PcoaEngine(n, grm=True) as twin:
        rows = planted_bed(n, v, seed)
        for r0 in range(0, v, call):
            eng.accumulate_plink_bed(rows[r0:r0 + call])
        rows = planted_bed(n, v, seed + 7)
        for r0 in range(0, v, call):
            st.accumulate_plink_bed(rows[r0:r0 + call])
            twin.accumulate_plink_bed(rows[r0:r0 + call])
        del rows
        for e in (eng, st, twin):
            e.sync()
        variants, used, store = eng.grm_info()
        out.update(variants=variants, used=used, store_bytes=store, device=eng.device_info()[0])
        x = torch.randn(n, dtype=torch.float64, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(seed + 1))
        out["panel_product_ms"] = 1e3 * timed(lambda: eng.grm_matvec_device(x))
        out["study_store_product_ms"] = 1e3 * timed(lambda: twin.grm_matvec_device(x))
        one = 0.5 * (out["panel_product_ms"] + out["study_store_product_ms"])   # a first pass there and a second pass here: the mean
        for k in (1, 2, 8):
            comps = rng.standard_normal((n, k))
            comps /= np.linalg.norm(comps, axis=0)
            lam = np.ones(k)
            w = 1e3 * timed(lambda: eng.grm_weights(comps, lam, scaled=False, first_variant=0, n_variants=min(v, 1024)))
            p = 1e3 * timed(lambda: eng.grm_project(st, comps, lam))
            out["num_pc"][str(k)] = {"weights_ms": w, "project_ms": p, "products_of_as_many_vectors_ms": k * one,
                                     "project_over_products": p / (k * one), "weights_over_products": w / (k * one)}
        out["project_k2_over_two_products"] = out["num_pc"]["2"]["project_over_products"]
    return out


def kernel_resources(path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                              "-c", os.path.join(csrc, "grm_multi.hip"), "-o", os.path.join(td, "x.o"), "-Rpass-analysis=kernel-resource-usage"],
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
    ap.add_argument("--resources", default=None, help="write the compile-time resources of the grm_multi.hip kernels here (needs hipcc, no GPU)")
    args = ap.parse_args()
    if args.resources:
        kernel_resources(args.resources)
        if not args.out:
            return 0
    P = importlib.import_module("spark-examples_amd")
    with P.PcoaEngine(256, grm=True) as e:      # code objects, first-use allocations
        e.accumulate_plink_bed(planted_bed(256, 512, args.seed))
        comps, lam, _ = e.compute(2)
        e.grm_project(e, comps, lam)
    doc = {"tool": "tools/grm_project_probe.py", "library": P._lib.load().pcoa_version().decode(), "source_hash": P._lib.source_hash(),
           "sizes": []}
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

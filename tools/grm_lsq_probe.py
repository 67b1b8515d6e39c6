#!/usr/bin/env python3
"""The least-squares projection on a GRM engine (pcoa_grm_project_lsq) against the mean-imputed one (pcoa_grm_project) on the same
panel and study stores (not a test, not bench.py).

Per size N x V, in one process: the synthetic PLINK rows of tools/grm_probe.py are appended to a GRM engine (the panel) and a
second draw of the same shape to a GRM study store, and the probe times, for num_pc = 2 and 8 with random unit "components":
  project         pcoa_grm_project with the called count, wall clock around the call (median of five after one warm call)
  lsq             pcoa_grm_project_lsq with the called count and the flags, the same way
  pair pass       the product, pair and finish launches of one lsq call, by HIP events (pcoa_get_grm_lsq_stats, the difference of
                  the cumulative seconds over the calls timed): num_pc (num_pc + 1) / 2 product vectors, four per pass over the
                  study's store
  solve           the solve kernel of one lsq call, by HIP events
`pair_pass_over_pass2` holds the pair pass against the second passes of pcoa_grm_project at the same num_pc, taken as project
minus weights (the first passes and the combine, measured through pcoa_grm_weights with a window of 1,024 rows); by instruction
count the expectation was (pairs + chunks) / (3 num_pc + ceil(num_pc / 2)): 5 / 7 at num_pc = 2 and 45 / 28 at num_pc = 8.
--resources writes the lines hipcc prints for grm_lsq.hip.

Usage: python tools/grm_lsq_probe.py [--sizes 2504x1000000,20000x262144,100000x131072] [--out profiles/NAME.json]
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
    call = 1 << 20
    rng = np.random.default_rng(seed)
    out = {"n": n, "v": v, "num_pc": {}}
    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(n, grm_study=True) as st:
        rows = planted_bed(n, v, seed)
        for r0 in range(0, v, call):
            eng.accumulate_plink_bed(rows[r0:r0 + call])
        rows = planted_bed(n, v, seed + 7)
        for r0 in range(0, v, call):
            st.accumulate_plink_bed(rows[r0:r0 + call])
        del rows
        eng.sync()
        st.sync()
        variants, used, store = eng.grm_info()
        out.update(variants=variants, used=used, store_bytes=store, device=eng.device_info()[0])
        for k in (2, 8):
            comps = rng.standard_normal((n, k))
            comps /= np.linalg.norm(comps, axis=0)
            lam = np.ones(k)
            w = 1e3 * timed(lambda: eng.grm_weights(comps, lam, scaled=False, first_variant=0, n_variants=min(v, 1024)))
            p = 1e3 * timed(lambda: eng.grm_project(st, comps, lam))
            s0 = eng.grm_lsq_stats()
            q = 1e3 * timed(lambda: eng.grm_project_lsq(st, comps))
            s1 = eng.grm_lsq_stats()
            calls = s1["grm_lsq_calls"] - s0["grm_lsq_calls"]
            pairs_ms = 1e3 * (s1["grm_lsq_pairs_seconds"] - s0["grm_lsq_pairs_seconds"]) / calls
            solve_ms = 1e3 * (s1["grm_lsq_solve_seconds"] - s0["grm_lsq_solve_seconds"]) / calls
            pairs = k * (k + 1) // 2
            chunks, rem = 0, pairs
            while rem:      # grm_lsq_chunk: four at a time, then two, then one
                rem -= 4 if rem >= 4 else 2 if rem >= 2 else 1
                chunks += 1
            out["num_pc"][str(k)] = {"weights_ms": w, "project_ms": p, "lsq_ms": q, "lsq_over_project": q / p,
                                     "pair_pass_ms": pairs_ms, "solve_ms": solve_ms, "pass2_ms": p - w,
                                     "pair_pass_over_pass2": pairs_ms / (p - w), "pairs": pairs, "chunks": chunks,
                                     "expected_by_instruction_count": (pairs + chunks) / (3.0 * k + (k + 1) // 2),
                                     "undetermined": s1["grm_lsq_undetermined"]}
    return out


def kernel_resources(path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                              "-c", os.path.join(csrc, "grm_lsq.hip"), "-o", os.path.join(td, "x.o"), "-Rpass-analysis=kernel-resource-usage"],
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
    ap.add_argument("--resources", default=None, help="write the compile-time resources of the grm_lsq.hip kernels here (needs hipcc, no GPU)")
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
        e.grm_project_lsq(e, comps)
    doc = {"tool": "tools/grm_lsq_probe.py", "library": P._lib.load().pcoa_version().decode(), "source_hash": P._lib.source_hash(),
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

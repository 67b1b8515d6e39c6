#!/usr/bin/env python3
"""Per-variant loadings against one product of the implicit operator, on the same store (not a test, not bench.py).

Per size: device-resident planted carrier bitsets (tools/operator_probe.py's generator, fixed seed) are appended to one
operator engine; then, in the same process on the same store,
  product    pcoa_operator_matvec_device: y = S v, two passes of N V bit-adds each;
  loadings   pcoa_loadings_operator with num_pc = 1, 2, 8 unit vectors, CENTRE | UNIT, device output: num_pc N V bit-adds,
             every bit decoded once per chunk of <= 8 components.
Each is warmed once and timed over --reps calls by the library's HIP events (pcoa_timings.operator_matvec_seconds,
pcoa_loadings_stats.loadings_seconds).  Reported per case: milliseconds, variants/s, bit-adds/s, and the V N / 8 bytes of the
bit matrix over that time as a fraction of the 6.29 TB/s measured copy ceiling.  Each size runs in a child process of its own.

Usage: python tools/loadings_probe.py [--sizes 2504x1000000,20000x262144,100000x131072] [--reps 3] [--out profiles/NAME.json]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from operator_probe import COPY_CEILING, planted_bits  # noqa: E402

DEFAULT_SIZES = "2504x1000000,20000x262144,100000x131072"
NUM_PCS = (1, 2, 8)


def run_size(n, v, seed, reps):
    import numpy as np
    import torch
    P = importlib.import_module("spark-examples_amd")
    bits = planted_bits(n, v, seed)
    rng = np.random.default_rng(seed)
    call = 1 << 20
    out = {"n": n, "v": v, "reps": reps, "matrix_bytes": v * n / 8.0}
    with P.PcoaEngine(n, operator=True) as eng:
        for r0 in range(0, v, call):
            eng.accumulate_bits(bits[r0:r0 + call])
        eng.sync()
        del bits
        out["device"] = eng.device_info()[0]
        out["store_bytes"] = eng.operator_info()[1]
        vec = torch.from_numpy(rng.standard_normal(n)).cuda()
        eng.operator_matvec_device(vec, False)            # warm: code objects, the passes' workspace
        eng.reset_timings()
        for _ in range(reps):
            eng.operator_matvec_device(vec, False)
        t = eng.timings()
        per = t["operator_matvec_seconds"] / max(t["operator_products"], 1)
        out["product"] = {"ms": 1e3 * per, "bit_adds_per_second": 2.0 * v * n / per,
                          "fraction_of_copy_ceiling": 2.0 * out["matrix_bytes"] / per / COPY_CEILING}
        out["loadings"] = []
        for k in NUM_PCS:
            u, _ = np.linalg.qr(rng.standard_normal((n, k)))
            with eng.loadings(u, np.linspace(2.0, 1.0, k)) as ld:
                ld.operator(0, v, device_out=True)          # warm
                eng.reset_timings()
                for _ in range(reps):
                    w = ld.operator(0, v, device_out=True)
                st = ld.stats()
                del w
            per = st["loadings_seconds"] / reps
            out["loadings"].append({"num_pc": k, "ms": 1e3 * per, "variants_per_second": v / per,
                                    "bit_adds_per_second": float(k) * v * n / per,
                                    "fraction_of_copy_ceiling": out["matrix_bytes"] / per / COPY_CEILING,
                                    "bytes_read": st["loadings_bytes"] / reps,
                                    "ms_over_one_product": per / (out["product"]["ms"] * 1e-3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=DEFAULT_SIZES, help="comma-separated NxV")
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    sizes = [tuple(int(t) for t in s.split("x")) for s in args.sizes.split(",")]
    if args.child:
        (n, v), = sizes
        print("PROBE " + json.dumps(run_size(n, v, args.seed, args.reps)))
        return 0
    results = []
    for n, v in sizes:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--sizes", "%dx%d" % (n, v), "--seed", str(args.seed),
                              "--reps", str(args.reps)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("PROBE ")]
        row = json.loads(line[0][6:]) if res.returncode == 0 and line else {"n": n, "v": v, "error": res.stderr[-800:]}
        results.append(row)
        print(json.dumps(row), flush=True)
        if res.returncode != 0:   # a fault on the device: nothing more is started on it
            break
    doc = {"tool": "tools/loadings_probe.py", "copy_ceiling_bytes_per_s": COPY_CEILING, "sizes": results}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0 if all("error" not in r for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())

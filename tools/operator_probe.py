#!/usr/bin/env python3
"""Stored S against the implicit similarity operator on the same job (not a test, not bench.py).

The job: device-resident synthetic carrier bitsets with planted population structure (three populations, generated on the
GPU from a fixed seed, so both legs see the same bits) -> the top two principal coordinates.  Each leg runs in a child
process of its own and is timed as wall clock from the first accumulate call to the returned components (engine creation
and pcoa_reserve outside, one small warm-up job before):
  stored    a full engine (pcoa_create): bitsets -> transpose -> Gram on the matrix cores -> Lanczos over S.  With
            --stored-tree DIR the child imports the package (and its built library) from that checkout, e.g. the parent
            commit's: the leg uses nothing the parent lacks.  (PCOA_LIB alone cannot point an older library at this tree's
            binding, which demands every symbol of this tree's header.)
  implicit  an operator engine (pcoa_create_operator): bitsets -> the store -> Lanczos over S v = X^T (X v).
Per size it reports both walls, the number of products, ms per product, the bytes a product reads (two passes over the
store) over that time as a fraction of the 6.29 TB/s measured copy ceiling, and bit-adds per second (2 V N per product).

Usage: python tools/operator_probe.py [--sizes 2504x1000000,20000x262144,100000x131072,100000x1000000]
                                      [--stored-tree DIR] [--out profiles/NAME.json]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("PCOA_PROBE_TREE") or ROOT)   # (a leg's child: the tree its package comes from)

COPY_CEILING = 6.29e12   # bytes/s, the measured device copy ceiling the documents quote
DEFAULT_SIZES = "2504x1000000,20000x262144,100000x131072,100000x1000000"


def planted_bits(n, v, seed, chunk_elems=1 << 29):
    """[v][ceil(n / 32)] int32 bitsets on cuda:0: sample i of population p carries a variant of population q with probability
    0.5 if p == q else 0.05; every fourth variant is carried by everybody with one probability in [0.02, 0.4]."""
    import torch
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    w = (n + 31) // 32
    pops = torch.clamp((torch.arange(w * 32, device=dev) * 3) // n, max=2)
    live = (torch.arange(w * 32, device=dev) < n)
    weights = (torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, device=dev)).view(1, 1, 32)
    out = torch.empty((v, w), dtype=torch.int32, device=dev)
    rows = max(1, min(v, chunk_elems // (w * 32)))
    for r0 in range(0, v, rows):
        r = min(rows, v - r0)
        which = torch.randint(0, 4, (r, 1), generator=gen, device=dev)
        flat = 0.02 + 0.38 * torch.rand((r, 1), generator=gen, device=dev)
        p = torch.where(which == 3, flat, torch.where(which == pops.view(1, -1), 0.5, 0.05))
        x = (torch.rand((r, w * 32), generator=gen, device=dev) < p) & live.view(1, -1)
        words = (x.view(r, w, 32).to(torch.int64) * weights).sum(dim=2)
        out[r0:r0 + r] = words.to(torch.int32)   # (values >= 2^31 wrap into the sign bit: the same 32 bits)
        del x, words, p
    torch.cuda.synchronize()
    return out


def run_leg(leg, n, v, seed):
    import numpy as np
    import torch
    P = importlib.import_module("spark-examples_amd")
    warm = planted_bits(256, 512, seed)
    kind = {"operator": True} if leg == "implicit" else {}
    with P.PcoaEngine(256, **kind) as e:      # code objects, first-use allocations
        e.accumulate_bits(warm)
        e.compute(2)
    bits = planted_bits(n, v, seed)
    call = 1 << 20
    with P.PcoaEngine(n, **kind) as eng:
        eng.reserve(min(v, call), 2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r0 in range(0, v, call):
            eng.accumulate_bits(bits[r0:r0 + call])
        comps, lam, nz = eng.compute(2)
        wall = time.perf_counter() - t0
        t = eng.timings()
        name, cus = eng.device_info()
        info = eng.operator_info() if leg == "implicit" else None
    out = {"leg": leg, "n": n, "v": v, "wall_s": wall, "eigenvalues": [float(x) for x in lam], "nonzero_rows": nz,
           "lanczos_steps": t["lanczos_steps"], "compute_total_s": t["compute_total_seconds"], "device": name,
           "tree": "--stored-tree" if os.environ.get("PCOA_PROBE_TREE") else "this tree", "pc1_abs_sum": float(np.abs(comps[:, 0]).sum())}
    if leg == "stored":
        out.update(gram_kernel_s=t["gram_kernel_seconds"], pack_s=t["pack_seconds"], lanczos_s=t["lanczos_seconds"])
    else:
        products, secs = t["operator_products"], t["operator_matvec_seconds"]
        pitch = ((n + 31) // 32 + 3) // 4 * 4
        read = 2.0 * v * pitch * 4
        per = secs / max(products, 1)
        out.update(products=products, ms_per_product=1e3 * per, bytes_read_per_product=read,
                   fraction_of_copy_ceiling=read / per / COPY_CEILING if per > 0 else None,
                   bit_adds_per_second=2.0 * v * n / per if per > 0 else None, store_bytes=info[1], append_s=t["pack_seconds"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=DEFAULT_SIZES, help="comma-separated NxV")
    ap.add_argument("--stored-tree", default=None, help="checkout (with its library built) the stored leg imports the package from, e.g. the parent commit's")
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sizes = [tuple(int(t) for t in s.split("x")) for s in args.sizes.split(",")]
    if args.leg:
        (n, v), = sizes
        print("PROBE " + json.dumps(run_leg(args.leg, n, v, args.seed)))
        return 0
    results = []
    for n, v in sizes:
        row = {"n": n, "v": v}
        for leg in ("stored", "implicit"):
            env = dict(os.environ)
            if leg == "stored" and args.stored_tree:
                env["PCOA_PROBE_TREE"] = os.path.abspath(args.stored_tree)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--sizes", "%dx%d" % (n, v), "--seed",
                                  str(args.seed)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("PROBE ")]
            row[leg] = json.loads(line[0][6:]) if res.returncode == 0 and line else {"error": res.stderr[-800:]}
        s, i = row["stored"], row["implicit"]
        if "wall_s" in s and "wall_s" in i:
            row["stored_over_implicit_wall"] = s["wall_s"] / i["wall_s"]
            row["eigenvalue_rel_diff"] = max(abs(a - b) / abs(a) for a, b in zip(s["eigenvalues"], i["eigenvalues"]))
        results.append(row)
        print(json.dumps(row), flush=True)
    doc = {"tool": "tools/operator_probe.py", "copy_ceiling_bytes_per_s": COPY_CEILING, "sizes": results}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

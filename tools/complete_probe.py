#!/usr/bin/env python3
"""The pairwise-complete similarity (pcoa_set_call_companion, pcoa_accumulate_plink_bed_calls): not a test, not
bench.py.

One MI355X, device-resident synthetic .bed rows with 5 % missing codes (three populations, the rest of a row's codes drawn by
the population's frequency), N samples x V variants.  Per shape, in a child process of its own under its own time limit:

(a) accumulation, same build, same process, after one warm-up of each:
  pair_wall_s        pcoa_accumulate_plink_bed_calls over the rows in blocks of --block-rows, to pcoa_gram_finalize + pcoa_sync on
                     BOTH engines (host clock)
  single_wall_s      pcoa_accumulate_plink_bed over the same rows to finalize + sync on ONE engine
  pair_over_single   the ratio (the expectation is about 2: a second contraction plus the wider decode write)
  decode_pair_s, decode_single_s   HIP-event time of the decode kernel alone (pcoa_timings.densify_seconds) in the two runs
(b) pcoa_compute(2) on the same S, bound against unbound:
  compute_wall_s, lanczos_steps, step_s = lanczos_s / steps (one mat-vec plus that step's re-orthogonalisation: an upper bound of
  the mat-vec), matvec_form; bytes_per_s = bytes of S (unbound) or of S + Q (bound) one mat-vec reads over step_s, and its
  share of the 6.29 TB/s copy ceiling: a LOWER bound of the mat-vec's rate
Every run is recorded, not only the best.

Usage: python tools/complete_probe.py [--shapes 2504x1000000,20000x262144,100000x131072] [--block-rows 65536] [--runs 3]
                                      [--limit 400] [--out profiles/NAME.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING = 6.29e12   # bytes/s, the measured device copy ceiling the documents quote
MISSING_RATE = 0.05
SEED = 1504
GEN_ROWS = 4096          # rows generated at a time (N bytes each before packing)


def synthetic_bed(torch, n, v):
    """uint8 [v][ceil(n / 4)] on the device: sample i in population i % 3; a code is 01 with probability 0.05, else het (10)
    with the population's frequency of that variant, else homozygous reference (11)."""
    g = torch.Generator(device="cuda")
    g.manual_seed(SEED)
    nb = (n + 3) // 4
    out = torch.empty((v, nb), dtype=torch.uint8, device="cuda")
    pop = torch.arange(4 * nb, device="cuda") % 3
    scale = torch.tensor([0.3, 0.6, 0.9], device="cuda")
    for v0 in range(0, v, GEN_ROWS):
        rows = min(GEN_ROWS, v - v0)
        f = (0.05 + 0.45 * torch.rand((rows, 3), device="cuda", generator=g)) * scale[None, :]
        u = torch.rand((rows, 4 * nb), device="cuda", generator=g)
        code = torch.where(u < MISSING_RATE, 1, torch.where(u < MISSING_RATE + f[:, pop], 2, 3)).to(torch.uint8)
        code[:, n:] = 0
        quad = code.view(rows, nb, 4)
        out[v0:v0 + rows] = quad[:, :, 0] | (quad[:, :, 1] << 2) | (quad[:, :, 2] << 4) | (quad[:, :, 3] << 6)
    torch.cuda.synchronize()
    return out


def tile_bytes(n, form, matrices):
    if form == 1:
        nb = (n + 1023) // 1024
        return matrices * 4.0 * 1024 * 1024 * nb * (nb + 1) / 2
    return matrices * 4.0 * n * n


def timed_compute(L, lib, eng, n, matrices):
    eng._check(lib.pcoa_reset_timings(eng._ctx))
    t0 = time.perf_counter()
    comps, lam, nz = eng.compute(2)
    wall = time.perf_counter() - t0
    t = L.PcoaTimings()
    eng._check(lib.pcoa_get_timings_sized(eng._ctx, ctypes.byref(t), ctypes.sizeof(t)))
    steps = int(t.lanczos_steps)
    out = {"compute_wall_s": wall, "center_s": t.center_seconds, "lanczos_s": t.lanczos_seconds, "lanczos_steps": steps,
           "eig_method": int(t.eig_method), "matvec_form": int(t.matvec_form), "nonzero_rows": int(nz),
           "eigenvalues": [float(x) for x in lam]}
    if steps > 0:
        out["step_s"] = t.lanczos_seconds / steps
        out["bytes_per_matvec"] = tile_bytes(n, out["matvec_form"], matrices)
        out["bytes_per_s"] = out["bytes_per_matvec"] / out["step_s"]
        out["share_of_copy_ceiling"] = out["bytes_per_s"] / COPY_CEILING
    return out


def leg(n, v, block_rows, runs):
    import torch
    L = importlib.import_module("spark-examples_amd._lib")
    P = importlib.import_module("spark-examples_amd")
    lib = L.load()
    rows = synthetic_bed(torch, n, v)
    out = {"n": n, "variants": v, "block_rows": block_rows, "missing_rate": MISSING_RATE, "accumulate": {"pair": [], "single": []},
           "compute": {"bound": [], "unbound": []}}
    with P.PcoaEngine(n) as eng, P.PcoaEngine(n) as q:
        out["device"] = eng.device_info()[0]
        eng.reserve(block_rows, 2)
        q.reserve(block_rows, 0)

        def feed(pair):
            eng.reset()
            q.reset()
            eng.sync()
            q.sync()
            eng.reset_timings()
            t0 = time.perf_counter()
            for v0 in range(0, v, block_rows):
                blk = rows[v0:v0 + block_rows]
                if pair:
                    eng.accumulate_plink_bed_calls(blk, q)
                else:
                    eng.accumulate_plink_bed(blk)
            eng.finalize()
            eng.sync()
            if pair:
                q.finalize()
                q.sync()
            wall = time.perf_counter() - t0
            t = eng.timings()
            return {"wall_s": wall, "decode_s": t["densify_seconds"], "gram_kernel_s": t["gram_kernel_seconds"],
                    "variants_per_s": v / wall}

        feed(True)      # warm-up: code objects, operand buffers, the second bitset buffer
        feed(False)
        for _ in range(runs):
            out["accumulate"]["single"].append(feed(False))
            out["accumulate"]["pair"].append(feed(True))
        best = dict((k, min(r["wall_s"] for r in out["accumulate"][k])) for k in ("pair", "single"))
        out["accumulate"]["pair_over_single_best_wall"] = best["pair"] / best["single"]
        dec = dict((k, min(r["decode_s"] for r in out["accumulate"][k])) for k in ("pair", "single"))
        out["accumulate"]["decode_pair_over_single_best"] = dec["pair"] / dec["single"] if dec["single"] > 0 else None
        # (b): the last feed was the pair, so S and Q are both resident
        eng.compute(2)
        for _ in range(runs):
            out["compute"]["unbound"].append(timed_compute(L, lib, eng, n, 1))
        eng.set_call_companion(q, v)
        eng.compute(2)
        for _ in range(runs):
            out["compute"]["bound"].append(timed_compute(L, lib, eng, n, 2))
        b = min(out["compute"]["bound"], key=lambda r: r["compute_wall_s"])
        u = min(out["compute"]["unbound"], key=lambda r: r["compute_wall_s"])
        if "step_s" in b and "step_s" in u:
            out["compute"]["step_s_bound_over_unbound"] = b["step_s"] / u["step_s"]
        out["compute"]["wall_bound_over_unbound"] = b["compute_wall_s"] / u["compute_wall_s"]
    print(json.dumps(out))


def child(args, limit):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return {"error": "exceeded its time limit of %d s" % limit, "args": args}
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    if res.returncode != 0 or not lines:
        return {"error": "exit status %d" % res.returncode, "stderr": res.stderr[-2000:], "args": args}
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="2504x1000000,20000x262144,100000x131072")
    ap.add_argument("--block-rows", type=int, default=1 << 16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="seconds per child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        n, v = (int(t) for t in a.leg.split("x"))
        return leg(n, v, a.block_rows, a.runs)
    L = importlib.import_module("spark-examples_amd._lib")
    report = {"tool": "tools/complete_probe.py", "source_hash": L.source_hash(), "seed": SEED, "copy_ceiling_bytes_per_s": COPY_CEILING,
              "shapes": []}
    for shape in a.shapes.split(","):
        r = child(["--leg", shape, "--block-rows", str(a.block_rows), "--runs", str(a.runs)], a.limit)
        report["shapes"].append(r)
        print(json.dumps(r), flush=True)
        if "error" in r:       # nothing more on a device that has just failed a leg
            break
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

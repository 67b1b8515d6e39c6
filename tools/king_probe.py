#!/usr/bin/env python3
"""The KING-robust kinship screen (pcoa_accumulate_plink_bed_king, pcoa_king_pairs): not a test, not bench.py.

One MI355X, device-resident synthetic .bed rows (three populations, Hardy-Weinberg genotypes at the population's frequency,
5 % missing codes), N samples x V variants.  Per shape, in a child process of its own under its own time limit; a shape whose
six N x N int32 matrices (five planes and one plain engine) do not fit the free memory is recorded as skipped:

(a) accumulation, same build, same process, after one warm-up of each:
  king_wall_s        pcoa_accumulate_plink_bed_king over the rows in blocks of --block-rows, to pcoa_gram_finalize + pcoa_sync on
                     ALL FIVE planes (host clock)
  single_wall_s      pcoa_accumulate_plink_bed over the same rows to finalize + sync on ONE engine
  five_single_wall_s the same five times over, one plane after the other: what the planes cost without the shared decode
  king_over_single   the ratio to ONE single accumulation (the expectation is about 5: five contractions)
(b) decode_king_s, decode_single_s   HIP-event time of the decode kernel alone (pcoa_timings.densify_seconds of planes[0] / of the
                     plain engine) in those runs
(c) the screen at --cutoff: pcoa_king_stats' HIP-event time and bytes per call, bytes/s and its share of the 6.29 TB/s copy
    ceiling; beside it pcoa_similar_pairs at --jaccard on ONE matrix of that N (pcoa_pairs_stats), the same figures
Every run is recorded, not only the best.

Usage: python tools/king_probe.py [--shapes 2504x1000000,20000x262144,100000x131072] [--block-rows 65536] [--runs 3]
                                  [--cutoff 0.177] [--jaccard 0.9] [--limit 500] [--out profiles/NAME.json]
"""
import argparse
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
SEED = 1604
GEN_ROWS = 4096          # rows generated at a time (N bytes each before packing)


def synthetic_bed(torch, n, v):
    """uint8 [v][ceil(n / 4)] on the device: sample i in population i % 3; a code is 01 with probability 0.05, else the
    genotype of two alleles drawn with the population's frequency of that variant (00, 10, 11)."""
    g = torch.Generator(device="cuda")
    g.manual_seed(SEED)
    nb = (n + 3) // 4
    out = torch.empty((v, nb), dtype=torch.uint8, device="cuda")
    pop = torch.arange(4 * nb, device="cuda") % 3
    of_dosage = torch.tensor([0, 2, 3], dtype=torch.uint8, device="cuda")
    for v0 in range(0, v, GEN_ROWS):
        rows = min(GEN_ROWS, v - v0)
        f = (0.1 + 0.8 * torch.rand((rows, 1), device="cuda", generator=g) + 0.12 * torch.randn((rows, 3), device="cuda", generator=g)).clamp(0.02, 0.98)
        p = f[:, pop]
        dosage = (torch.rand((rows, 4 * nb), device="cuda", generator=g) < p).to(torch.int64) + (torch.rand((rows, 4 * nb), device="cuda", generator=g) < p)
        code = of_dosage[dosage]
        code[torch.rand((rows, 4 * nb), device="cuda", generator=g) < MISSING_RATE] = 1
        code[:, n:] = 0
        quad = code.view(rows, nb, 4)
        out[v0:v0 + rows] = quad[:, :, 0] | (quad[:, :, 1] << 2) | (quad[:, :, 2] << 4) | (quad[:, :, 3] << 6)
    torch.cuda.synchronize()
    return out


def leg(n, v, block_rows, runs, cutoff, jaccard):
    import torch
    P = importlib.import_module("spark-examples_amd")
    free, _ = torch.cuda.mem_get_info()
    need = 6 * 4 * n * n + v * ((n + 3) // 4) + 6 * (1 << 30)
    if need > free:
        print(json.dumps({"n": n, "variants": v, "skipped": "needs about %d bytes (six N x N int32 matrices, the rows, the operand "
                                                            "buffers), %d are free" % (need, free)}))
        return
    rows = synthetic_bed(torch, n, v)
    out = {"n": n, "variants": v, "block_rows": block_rows, "missing_rate": MISSING_RATE, "cutoff": cutoff, "jaccard": jaccard,
           "accumulate": {"king": [], "single": [], "five_single": []}, "screen": {"king": [], "jaccard": []}}
    engines = [P.PcoaEngine(n) for _ in range(6)]
    planes, plain = engines[:5], engines[5]
    try:
        out["device"] = plain.device_info()[0]
        for e in engines:
            e.reserve(block_rows, 0)

        def finish(which):
            for e in which:
                e.finalize()
                e.sync()

        def feed(kind):
            which = planes if kind != "single" else [plain]
            for e in which:
                e.reset()
                e.sync()
                e.reset_timings()
            t0 = time.perf_counter()
            if kind == "king":
                for v0 in range(0, v, block_rows):
                    P.PcoaEngine.accumulate_plink_bed_king(planes, rows[v0:v0 + block_rows])
            else:
                for e in which:
                    for v0 in range(0, v, block_rows):
                        e.accumulate_plink_bed(rows[v0:v0 + block_rows])
            finish(which)
            wall = time.perf_counter() - t0
            return {"wall_s": wall, "decode_s": sum(e.timings()["densify_seconds"] for e in which), "variants_per_s": v / wall}

        feed("single")      # warm-up: code objects, operand buffers, the plane rows
        feed("king")
        for _ in range(runs):
            out["accumulate"]["single"].append(feed("single"))
            out["accumulate"]["five_single"].append(feed("five_single"))
            out["accumulate"]["king"].append(feed("king"))
        best = dict((k, min(r["wall_s"] for r in out["accumulate"][k])) for k in ("king", "single", "five_single"))
        out["accumulate"]["king_over_single_best_wall"] = best["king"] / best["single"]
        out["accumulate"]["king_over_five_single_best_wall"] = best["king"] / best["five_single"]
        dec = dict((k, min(r["decode_s"] for r in out["accumulate"][k])) for k in ("king", "single"))
        out["accumulate"]["decode_king_over_single_best"] = dec["king"] / dec["single"] if dec["single"] > 0 else None
        # (c): the last feed was the king's, so the five matrices are resident; the plain engine holds the carriers' S
        P.PcoaEngine.king_pairs(planes, cutoff, capacity=1 << 20)
        plain.similar_pairs(jaccard, capacity=1 << 20)
        for _ in range(runs):
            planes[0].reset_timings()
            _, n_found, _, _ = P.PcoaEngine.king_pairs(planes, cutoff, capacity=1 << 20)
            st = planes[0].king_stats()
            out["screen"]["king"].append({"seconds": st["king_seconds"], "bytes": st["king_bytes"], "n_found": n_found,
                                          "bytes_per_s": st["king_bytes"] / st["king_seconds"],
                                          "share_of_copy_ceiling": st["king_bytes"] / st["king_seconds"] / COPY_CEILING})
            plain.reset_timings()
            _, n_found, _ = plain.similar_pairs(jaccard, capacity=1 << 20)
            t = plain.timings()
            out["screen"]["jaccard"].append({"seconds": t["pairs_seconds"], "bytes": t["pairs_bytes"], "n_found": n_found,
                                             "bytes_per_s": t["pairs_bytes"] / t["pairs_seconds"],
                                             "share_of_copy_ceiling": t["pairs_bytes"] / t["pairs_seconds"] / COPY_CEILING})
        k = min(r["seconds"] for r in out["screen"]["king"])
        j = min(r["seconds"] for r in out["screen"]["jaccard"])
        out["screen"]["king_over_jaccard_best_seconds"] = k / j
    finally:
        for e in engines:
            e.close()
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
    ap.add_argument("--cutoff", type=float, default=0.177)
    ap.add_argument("--jaccard", type=float, default=0.9)
    ap.add_argument("--limit", type=int, default=500, help="seconds per child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        n, v = (int(t) for t in a.leg.split("x"))
        return leg(n, v, a.block_rows, a.runs, a.cutoff, a.jaccard)
    L = importlib.import_module("spark-examples_amd._lib")
    report = {"tool": "tools/king_probe.py", "source_hash": L.source_hash(), "seed": SEED, "copy_ceiling_bytes_per_s": COPY_CEILING,
              "shapes": []}
    for shape in a.shapes.split(","):
        r = child(["--leg", shape, "--block-rows", str(a.block_rows), "--runs", str(a.runs), "--cutoff", str(a.cutoff),
                   "--jaccard", str(a.jaccard)], a.limit)
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

#!/usr/bin/env python3
"""The LD pruner's kernels against their models (pcoa_ld_*): not a test, not bench.py.

One MI355X.  Per (N, V, W): V rows of planted carrier bitsets resident on the device -- runs of eight noisy copies of a random
founder row, so that the pruner removes rows for the reason it exists --, a pruner with r2_max = 0.2 and no accumulation, one
warm-up call over all V rows and then three measured calls (pcoa_reset_timings in front of each).  Per call, from pcoa_ld_stats
(HIP events on the ctx stream):
  count_s, band_s, resolve_s, compact_s   the four kernel groups, separately
  band_model_s     the VALU-issue model of the band kernel: 2 instructions (v_and_b32, v_bcnt_u32_b32) per word pair, ld_pairs x
                   ceil(N / 32) word pairs, on 256 CUs x 64 lanes per clock at the clock the device reports
  band_over_model  band_s / band_model_s
  resolve_over_band  the sequential greedy pass beside the band kernel (it is reported, not folded into a sum)
  prune_s          the four groups together; wall_s: host clock around the call (it ends with the chunk's host wait)
Then, in the same process, pcoa_accumulate_bits of the same rows to pcoa_gram_finalize on the same engine (one warm-up, three
runs, host clock; gram_kernel_s from pcoa_timings), and prune_over_accumulate = median prune_s / median accumulate wall.
Every size runs in a child process of its own under its own time limit.

Usage: python tools/ld_probe.py [--cases 2504:1000000:50,2504:1000000:500,20000:262144:50,100000:131072:50]
                                [--out profiles/NAME.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CUS, LANES = 256, 64
R2 = 0.2
SEED = 1404


def planted_bits(torch, n, v, device):
    """[v][ceil(n / 32)] int32: runs of eight rows, each the run's founder (carrier density 1/4) with one genotype in 16 (even
    runs) or in 64 (odd runs) flipped."""
    words = (n + 31) // 32
    g = torch.Generator(device=device)
    g.manual_seed(SEED)
    out = torch.empty((v, words), dtype=torch.int32, device=device)

    def rnd(rows):
        return torch.randint(-2 ** 31, 2 ** 31, (rows, words), dtype=torch.int64, device=device, generator=g).to(torch.int32)

    step = 1 << 15
    for v0 in range(0, v, step):
        rows = min(step, v - v0)
        runs = (rows + 7) // 8
        founder = (rnd(runs) & rnd(runs)).repeat_interleave(8, dim=0)[:rows]
        noise = rnd(rows) & rnd(rows) & rnd(rows) & rnd(rows)
        odd = ((torch.arange(rows, device=device) // 8) & 1).bool()[:, None]
        noise = torch.where(odd, noise & rnd(rows) & rnd(rows), noise)
        out[v0:v0 + rows] = founder ^ noise
    return out


def reported_clock_hz():
    """hipDeviceAttributeClockRate of device 0 (the peak engine clock, in kHz) from the HIP runtime torch has loaded."""
    hip = ctypes.CDLL("libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
    khz = ctypes.c_int(0)
    HIP_DEVICE_ATTRIBUTE_CLOCK_RATE = 5
    if hip.hipDeviceGetAttribute(ctypes.byref(khz), HIP_DEVICE_ATTRIBUTE_CLOCK_RATE, 0) != 0 or khz.value <= 0:
        raise RuntimeError("hipDeviceGetAttribute(hipDeviceAttributeClockRate) failed")
    return 1e3 * khz.value


def leg(n, v, w):
    import torch
    L = importlib.import_module("spark-examples_amd._lib")
    P = importlib.import_module("spark-examples_amd")
    dev = torch.device("cuda", 0)
    clock_hz = reported_clock_hz()
    bits = planted_bits(torch, n, v, dev)
    torch.cuda.synchronize()
    words = (n + 31) // 32
    out = {"leg": "ld", "n": n, "variants": v, "window": w, "r2_max": R2, "clock_hz_reported": clock_hz, "calls": []}
    with P.PcoaEngine(n) as eng:
        out["device"] = eng.device_info()[0]
        with eng.ld_pruner(w, R2, accumulate=False) as pr:
            pr.bits(bits)                                     # warm-up: code objects, first touch of the buffers
            for _ in range(3):
                pr.break_contig()
                eng.reset_timings()
                t0 = time.perf_counter()
                keep = pr.bits(bits)
                wall = time.perf_counter() - t0
                st = pr.stats()
                model = 2.0 * st["ld_pairs"] * words / (CUS * LANES * clock_hz)
                prune = st["ld_count_seconds"] + st["ld_band_seconds"] + st["ld_resolve_seconds"] + st["ld_compact_seconds"]
                out["calls"].append({"count_s": st["ld_count_seconds"], "band_s": st["ld_band_seconds"],
                                     "resolve_s": st["ld_resolve_seconds"], "compact_s": st["ld_compact_seconds"], "prune_s": prune,
                                     "wall_s": wall, "pairs": st["ld_pairs"], "kept": st["ld_kept"], "monomorphic": st["ld_monomorphic"],
                                     "band_model_s": model, "band_over_model": st["ld_band_seconds"] / model,
                                     "resolve_over_band": st["ld_resolve_seconds"] / st["ld_band_seconds"]})
            out["kept_fraction"] = float(keep.mean())
        acc = []
        for i in range(4):                                    # the first is the warm-up
            eng.reset()
            eng.sync()
            eng.reset_timings()
            t0 = time.perf_counter()
            eng.accumulate_bits(bits)
            eng.finalize()
            wall = time.perf_counter() - t0
            if i:
                acc.append({"wall_s": wall, "gram_kernel_s": eng.timings()["gram_kernel_seconds"]})
        out["accumulate"] = acc
    med = lambda key, rows: statistics.median(r[key] for r in rows)
    out["median"] = dict((k, med(k, out["calls"])) for k in ("count_s", "band_s", "resolve_s", "compact_s", "prune_s", "wall_s",
                                                             "band_over_model", "resolve_over_band"))
    out["median"]["accumulate_wall_s"] = med("wall_s", acc)
    out["median"]["prune_over_accumulate"] = out["median"]["prune_s"] / out["median"]["accumulate_wall_s"]
    out["resolve_exceeds_band"] = bool(out["median"]["resolve_s"] > out["median"]["band_s"])
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
    ap.add_argument("--cases", default="2504:1000000:50,2504:1000000:500,20000:262144:50,100000:131072:50", help="N:V:W,...")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        n, v, w = (int(t) for t in a.leg.split(":"))
        return leg(n, v, w)
    L = importlib.import_module("spark-examples_amd._lib")
    report = {"tool": "tools/ld_probe.py", "source_hash": L.source_hash(), "seed": SEED,
              "band_model": "2 instructions per word pair on %d CUs x %d lanes per clock" % (CUS, LANES), "cases": []}
    for case in a.cases.split(","):
        r = child(["--leg", case], a.limit)
        report["cases"].append(r)
        print(json.dumps(r), flush=True)
        if "error" in r:       # nothing more on a device that has just failed a leg
            break
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 1 if any("error" in r for r in report["cases"]) else 0


if __name__ == "__main__":
    sys.exit(main() or 0)

#!/usr/bin/env python3
"""The reduction of S over k engines: the pcoa_gram_reduce_from chain against pcoa_gram_reduce_peers (not a test, not bench.py).

k engines on device 0, each holding an N x N int32 partial S of a few thousand synthetic variants of its own (N = 16,384:
1 GiB of S each).  Three legs per k, each in a child process of its own under its own time limit, each reduction timed by wall
and by the library's own HIP-event counters, `--repeats` times on the same engines (sums of integers: a reduced S reduces again):
  chain       for g in 1..k-1: reduce_from(engine 0, engine g) -- what --reduce peer runs.  With PCOA_LIB naming another build
              of the library (the parent commit's: PCOA_LIB=/path/to/libpcoa_hip.so python tools/reduce_probe.py) this leg
              runs on that build; it binds only the symbols that build exports and uses nothing the parent lacks.  HIP-event
              time: pcoa_timings.finalize_seconds of engine 0 (its add kernels).
  allgather   reduce_peers(engines, root_only=False): every engine ends with the total.
  root_only   reduce_peers(engines, root_only=True): engine 0 ends with the total, the others reset -- what --reduce scatter
              runs.  Engines 1.. take part in phase 1 only, so their reduce_peers_seconds is the chunk kernel alone: the
              kernel's rate is (k + 1) 4 N^2 / k bytes (k chunks read, one written) over that time, against the 6.29 TB/s
              measured copy ceiling the documents quote.
ALL ENGINES SHARE ONE DEVICE here: the numbers are kernel and copy cost in one HBM -- the k chunk kernels run beside each
other and share its bandwidth -- and say nothing about links between devices.

Usage: python tools/reduce_probe.py [--samples 16384] [--engines 2,4,8] [--variants 4096] [--out profiles/NAME.json]
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


def run_leg(leg, n, k, v, repeats, seed):
    L = importlib.import_module("spark-examples_amd._lib")
    if leg == "chain" and os.environ.get("PCOA_LIB"):   # another build: bind what it exports (the chain needs nothing newer)
        other = ctypes.CDLL(L.LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        L._SIGNATURES[:] = [s for s in L._SIGNATURES if hasattr(other, s[0])]
    elif leg != "chain":
        L.LIB_PATH = os.path.join(ROOT, "spark-examples_amd", "libpcoa_hip.so")   # the new call is this tree's
    P = importlib.import_module("spark-examples_amd")
    synth = importlib.import_module("spark-examples_amd.synth")
    lib = L.load()

    def timings(e):   # pcoa_timings alone: the one struct every build fills
        t = L.PcoaTimings()
        e._check(lib.pcoa_get_timings_sized(e._ctx, ctypes.byref(t), ctypes.sizeof(t)))
        return t

    def reduce_once(engines):
        if leg == "chain":
            for e in engines[1:]:
                engines[0].reduce_from(e)
        else:
            P.reduce_peers(engines, root_only=(leg == "root_only"))

    warm = [P.PcoaEngine(256) for _ in range(k)]      # code objects, first-use allocations
    for g, e in enumerate(warm):
        e.accumulate_synthetic(seed, synth.pop_offsets(256), synth.thresholds(seed, 128 * g, 128), 128 * g)
    reduce_once(warm)
    for e in warm:
        e.close()
    offs = synth.pop_offsets(n)
    engines = [P.PcoaEngine(n) for _ in range(k)]
    rec = {"leg": leg, "engines": k, "library": os.path.relpath(L.LIB_PATH, ROOT), "version": lib.pcoa_version().decode(), "device": engines[0].device_info()[0],
           "runs": []}
    for g, e in enumerate(engines):
        e.accumulate_synthetic(seed, offs, synth.thresholds(seed, v * g, v), v * g)
        e.finalize()
    for _ in range(repeats):
        for e in engines:
            e.reset_timings()
        t0 = time.perf_counter()
        reduce_once(engines)
        wall = time.perf_counter() - t0
        run = {"wall_ms": 1e3 * wall}
        if leg == "chain":
            t = timings(engines[0])
            run.update(engine0_add_kernels_ms=1e3 * t.finalize_seconds, reduce_int32_calls=int(t.reduce_int32_calls))
        else:
            ts = [e.timings() for e in engines]
            run.update(reduce_peers_ms=[1e3 * t["reduce_peers_seconds"] for t in ts],
                       reduce_peers_bytes_in=[int(t["reduce_peers_bytes_in"]) for t in ts],
                       reduce_int32_calls=[int(t["reduce_int32_calls"]) for t in ts])
            if leg == "root_only" and k > 1:   # engines 1..: the chunk kernel alone
                per_owner = (k + 1) * 4.0 * n * n / k
                rates = [per_owner / t["reduce_peers_seconds"] for t in ts[1:] if t["reduce_peers_seconds"] > 0]
                run.update(chunk_kernel_bytes_per_owner=per_owner, chunk_kernel_GB_per_s=[r / 1e9 for r in rates],
                           chunk_kernel_fraction_of_copy_ceiling=[r / COPY_CEILING for r in rates])
        rec["runs"].append(run)
    for e in engines:
        e.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16384)
    ap.add_argument("--engines", default="2,4,8")
    ap.add_argument("--variants", type=int, default=4096, help="synthetic variants fed to each engine")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--leg-timeout", type=float, default=150.0, help="seconds a leg's child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)   # (a child: run one leg, print its record)
    args = ap.parse_args()
    if args.leg:
        leg, k = args.leg.split(":")
        print("LEG " + json.dumps(run_leg(leg, args.samples, int(k), args.variants, args.repeats, args.seed)))
        return 0
    n = args.samples
    doc = {"tool": "tools/reduce_probe.py", "samples": n, "variants_per_engine": args.variants, "s_bytes_per_engine": 4 * n * n,
           "copy_ceiling_bytes_per_s": COPY_CEILING,
           "note": "every engine on ONE device: kernel and copy cost inside one HBM, no link between devices is crossed",
           "chain_library": os.path.relpath(os.environ["PCOA_LIB"], ROOT) if os.environ.get("PCOA_LIB") else "this tree's", "legs": []}
    status = 0
    for k in [int(x) for x in args.engines.split(",")]:
        for leg in ("chain", "allgather", "root_only"):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", "%s:%d" % (leg, k), "--samples", str(n), "--variants",
                   str(args.variants), "--repeats", str(args.repeats), "--seed", str(args.seed)]
            try:
                res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=args.leg_timeout)
            except subprocess.TimeoutExpired:
                doc["legs"].append({"leg": leg, "engines": k, "failed": "time limit of %.0f s" % args.leg_timeout})
                status = 124
                break
            lines = [ln for ln in res.stdout.splitlines() if ln.startswith("LEG ")]
            if res.returncode != 0 or not lines:   # nothing more is started on the device after a leg that did not end well
                doc["legs"].append({"leg": leg, "engines": k, "failed": "exit status %d" % res.returncode, "stderr": res.stderr[-2000:]})
                status = res.returncode or 1
                break
            doc["legs"].append(json.loads(lines[-1][4:]))
            print("%s k=%d: %s" % (leg, k, ", ".join("%.3f ms" % r["wall_ms"] for r in doc["legs"][-1]["runs"])), flush=True)
        if status:
            break
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())

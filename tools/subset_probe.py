#!/usr/bin/env python3
"""One outlier-removal round on a stored S: subset + computePca against accumulating the reduced cohort again (not a test,
not bench.py).

The job: a full engine over N synthetic samples (the Balding-Nichols model of synth.py, generated on the device) holds S
of V variants and has computed its principal components once.  `removed` samples, evenly spread, are then dropped:
  subset      PcoaEngine.subset(keep) + compute(num_pc) on the result: the round as --outlier-iterations runs it.  Reported:
              the wall of the round, the HIP-event time of the gather (pcoa_timings.subset_seconds), its bytes (8 m^2: every
              entry of the int32 sub-matrix read once and written once) over that time, and that rate as a fraction of the
              6.29 TB/s measured copy ceiling the documents quote.
  reaccumulate  what a round costs without it: a fresh engine over m = N - removed samples fed V variants of the same model
              again, then compute(num_pc).  (The synthetic generator draws its bits per (variant, column), so this cohort has
              the shape of the reduced one, not its bits: the walls compare, the eigenvalues are not meant to.)
A second keep set that drops every other sample shows the gather where it is only correct, not fast.
Both rounds need a new engine over m samples, i.e. 4 m^2 bytes of HBM from the runtime (40 GB at m = 99,900): the subset wall
contains it (pcoa_create_subset creates the engine; subset_call_wall_outside_the_gather_s is what the call takes beyond the
gather), and the reaccumulate round reports its engine creation as create_wall_s and counts it in round_wall_s.  What the
allocation costs is the runtime's and can dominate either figure: read the parts.  pcoa_reserve and the host-side thresholds
are outside both.

Usage: python tools/subset_probe.py [--samples 100000] [--variants 1000000] [--removed 100] [--out profiles/NAME.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING = 6.29e12   # bytes/s, the measured device copy ceiling the documents quote


def feed(eng, synth, seed, offs, thr_all, chunk):
    for v0 in range(0, thr_all.shape[0], chunk):
        eng.accumulate_synthetic(seed, offs, thr_all[v0:v0 + chunk], v0)


def gather_record(sub, m):
    t = sub.timings()
    secs, nbytes = t["subset_seconds"], t["subset_bytes"]
    return {"m": m, "gather_ms": 1e3 * secs, "gather_bytes": nbytes, "gather_GB_per_s": nbytes / secs / 1e9 if secs > 0 else None,
            "fraction_of_copy_ceiling": nbytes / secs / COPY_CEILING if secs > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--variants", type=int, default=1000000)
    ap.add_argument("--removed", type=int, default=100)
    ap.add_argument("--num-pc", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    P = importlib.import_module("spark-examples_amd")
    synth = importlib.import_module("spark-examples_amd.synth")
    n, v, k = args.samples, args.variants, args.num_pc
    now = time.perf_counter
    thr_all = synth.thresholds(args.seed, 0, v)
    with P.PcoaEngine(256) as e:      # code objects, first-use allocations: the gather and computePca included
        feed(e, synth, args.seed, synth.pop_offsets(256), thr_all[:512], 512)
        e.compute(k)
        with e.subset(np.arange(0, 256, 2)) as s:
            s.compute(k)
    gone = np.linspace(0, n - 1, args.removed).astype(np.int64) if args.removed else np.zeros(0, dtype=np.int64)
    keep = np.setdiff1d(np.arange(n), gone).astype(np.int32)
    m = int(keep.size)
    doc = {"tool": "tools/subset_probe.py", "samples": n, "variants": v, "removed": int(n - m), "num_pc": k,
           "copy_ceiling_bytes_per_s": COPY_CEILING}
    with P.PcoaEngine(n) as full:
        full.reserve(min(v, args.chunk), k)
        t0 = now()
        feed(full, synth, args.seed, synth.pop_offsets(n), thr_all, args.chunk)
        full.finalize()
        doc["full_accumulate_wall_s"] = now() - t0
        t0 = now()
        _, lam_full, _ = full.compute(k)
        doc["full_compute_wall_s"] = now() - t0
        doc["device"] = full.device_info()[0]
        # the round: subset + computePca
        t0 = now()
        sub = full.subset(keep)
        t1 = now()
        _, lam_sub, _ = sub.compute(k)
        t2 = now()
        rec = gather_record(sub, m)
        rec.update(subset_call_wall_s=t1 - t0, subset_call_wall_outside_the_gather_s=(t1 - t0) - 1e-3 * rec["gather_ms"],
                   compute_wall_s=t2 - t1, round_wall_s=t2 - t0, eigenvalues=[float(x) for x in lam_sub],
                   matvec_form=sub.timings()["matvec_form"], lanczos_steps=sub.timings()["lanczos_steps"])
        doc["subset_round"] = rec
        sub.close()
        # a second call, after the first result was destroyed: how much the allocation of 4 m^2 bytes varies
        t0 = now()
        sub = full.subset(keep)
        doc["subset_call_again_wall_s"] = now() - t0
        doc["subset_again"] = gather_record(sub, m)
        sub.close()
        # the gather where it is only correct: every other sample
        sparse = np.arange(0, n, 2, dtype=np.int32)
        t0 = now()
        sub = full.subset(sparse)
        doc["sparse_call_wall_s"] = now() - t0
        doc["sparse_keep_every_other_sample"] = gather_record(sub, int(sparse.size))
        sub.close()
        doc["full_eigenvalues"] = [float(x) for x in lam_full]
    # the same round without the subset: the reduced cohort's shape accumulated again
    tc = now()
    fresh = P.PcoaEngine(m)
    create_wall = now() - tc
    with fresh:
        fresh.reserve(min(v, args.chunk), k)
        offs = synth.pop_offsets(m)
        t0 = now()
        feed(fresh, synth, args.seed, offs, thr_all, args.chunk)
        fresh.finalize()
        t1 = now()
        fresh.compute(k)
        t2 = now()
        t = fresh.timings()
        doc["reaccumulate_round"] = {"m": m, "create_wall_s": create_wall, "accumulate_wall_s": t1 - t0, "compute_wall_s": t2 - t1,
                                     "round_wall_s": create_wall + (t2 - t0), "gram_kernel_s": t["gram_kernel_seconds"]}
    doc["reaccumulate_over_subset_round_wall"] = doc["reaccumulate_round"]["round_wall_s"] / doc["subset_round"]["round_wall_s"]
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

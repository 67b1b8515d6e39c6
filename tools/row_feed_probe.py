#!/usr/bin/env python3
"""The HOST-row legs of the boundaries that share the row feed (csrc/row_feed.h): not a test, not bench.py.

tools/ld_probe.py, loadings_probe.py and complete_probe.py time their kernels over device-resident rows; this probe times what
they leave out, the path of a host caller's rows through the staging ring, for every boundary that has one.  One MI355X,
N = 2504, pageable numpy rows, V rows per call (several chunks of every boundary: 2^17 rows, 2^16 for the pruner); per leg one
warm-up call, then --reps calls timed by the host clock from the call to the end of pcoa_sync (both engines for the pair):
  accumulate_bits, accumulate_plink_bed, accumulate_plink_bed_calls      to S (and Q)
  loadings_bits, loadings_plink_bed                                      2 components, host `out`
  ld_bits, ld_plink_bed                                                  window 50, r2_max 0.2, no accumulation
and, as `device.<leg>`, the same rows as CUDA tensors for the five boundaries whose device rows go through the feed as well (device
bitsets of accumulate_bits and loadings_bits go to their consumer whole).  Prints one JSON line: per leg every run in variants/s.  Run it once per process (A/B: alternate two builds through PCOA_LIB).

Usage: python tools/row_feed_probe.py [--variants 524288] [--reps 5]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 2504


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=1 << 19)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    P = importlib.import_module("spark-examples_amd")
    v, words, nb = a.variants, (N + 31) // 32, (N + 3) // 4
    rng = np.random.default_rng(2504)
    bits = rng.integers(0, 2 ** 32, size=(v, words), dtype=np.uint32) & rng.integers(0, 2 ** 32, size=(v, words), dtype=np.uint32)
    bits[:, -1] &= np.uint32((1 << (N & 31)) - 1)
    bed = rng.integers(0, 256, size=(v, nb), dtype=np.uint8) | np.uint8(0xAA)      # codes 10 / 11: a sparse-ish cohort
    u = np.linalg.qr(rng.standard_normal((N, 2)))[0]
    out = {"tool": "tools/row_feed_probe.py", "n": N, "variants": v, "lib": os.environ.get("PCOA_LIB", "in-tree"), "legs": {}}

    def timed(name, call, engines):
        runs = []
        for i in range(a.reps + 1):                  # the first is the warm-up
            for e in engines:
                e.reset()
                e.sync()
            t0 = time.perf_counter()
            call()
            for e in engines:
                e.sync()
            if i:
                runs.append(v / (time.perf_counter() - t0))
        out["legs"][name] = runs

    import torch  # plumbing only: the device copies of the rows
    bits_d = torch.from_numpy(bits.view(np.int32)).cuda()
    bed_d = torch.from_numpy(bed).cuda()
    with P.PcoaEngine(N) as eng, P.PcoaEngine(N) as q:
        out["device"] = eng.device_info()[0]
        timed("accumulate_bits", lambda: eng.accumulate_bits(bits), [eng])
        timed("accumulate_plink_bed", lambda: eng.accumulate_plink_bed(bed), [eng])
        timed("accumulate_plink_bed_calls", lambda: eng.accumulate_plink_bed_calls(bed, q), [eng, q])
        timed("device.accumulate_plink_bed", lambda: eng.accumulate_plink_bed(bed_d), [eng])
        timed("device.accumulate_plink_bed_calls", lambda: eng.accumulate_plink_bed_calls(bed_d, q), [eng, q])
        with eng.loadings(u, np.array([2.0, 1.0])) as ld:
            timed("loadings_bits", lambda: ld.bits(bits), [eng])
            timed("loadings_plink_bed", lambda: ld.plink_bed(bed), [eng])
            timed("device.loadings_plink_bed", lambda: ld.plink_bed(bed_d), [eng])
        with eng.ld_pruner(50, 0.2, accumulate=False) as pr:
            timed("ld_bits", lambda: pr.bits(bits), [eng])
            timed("ld_plink_bed", lambda: pr.plink_bed(bed), [eng])
            timed("device.ld_bits", lambda: pr.bits(bits_d), [eng])
            timed("device.ld_plink_bed", lambda: pr.plink_bed(bed_d), [eng])
    print("PROBE " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""computePca under the three similarity measures (pcoa_set_similarity): not a test, not bench.py.

One MI355X, N synthetic samples x 2^17 variants (the generator of bench.py's configs, accumulated on the device), S resident.
Per N and per measure (shared, jaccard, cosine), after one warm-up computePca of that measure:
  compute_wall_s     wall of pcoa_compute(2), host clock around the call
  center_s           HIP-event time of the centring: the row-sum pass (shared: integer row sums; a measure: the diagonal, the
                     uncentred mat-vec with x = 1, the fp64 stats) plus rowSums / N -- pcoa_timings.center_seconds
  lanczos_s, steps   HIP-event time of the whole Lanczos iteration and its step count
  step_s             lanczos_s / steps: one mat-vec PLUS that step's re-orthogonalisation and its share of the Ritz checks (the
                     library has no timer around the mat-vec alone).  The re-orthogonalisation reads at most steps x N doubles
                     per pass and is the same work under every measure, so the DIFFERENCE of step_s between two measures is
                     the difference of their mat-vecs, and step_s itself bounds a mat-vec from above
  s_bytes_per_s      bytes of S one mat-vec reads (matvec_form 1: the upper-triangular 1024 x 1024 tiles, 4 bytes per entry;
                     form 0: all N^2 entries) over step_s, and its share of the 6.29 TB/s copy ceiling: a LOWER bound of the
                     mat-vec's rate, for the same reason
Every N runs in a child process of its own under its own time limit.

--ab-lib PATH: the check that the default path did not move.  Shared-measure pcoa_compute at the largest N with this tree's
library and with the library at PATH (the parent commit's build), `--ab-runs` runs each, alternating, every run a child process
of its own (PCOA_LIB names the library, as tools/reduce_probe.py does; only the symbols that build exports are bound).  Both
series and their medians are recorded; this is a record, not a test.

Usage: python tools/measure_probe.py [--sizes 2504,20000,100000] [--variants 131072] [--ab-lib PATH] [--ab-runs 5]
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

COPY_CEILING = 6.29e12   # bytes/s, the measured device copy ceiling the documents quote
MEASURES = ("shared", "jaccard", "cosine")
SEED = 1004
CHUNK = 1 << 15


def load(bind_only_exported):
    L = importlib.import_module("spark-examples_amd._lib")
    if bind_only_exported:   # another build of the library: bind what it exports
        other = ctypes.CDLL(L.LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        L._SIGNATURES[:] = [s for s in L._SIGNATURES if hasattr(other, s[0])]
    P = importlib.import_module("spark-examples_amd")
    return L, P, importlib.import_module("spark-examples_amd.synth")


def resident_engine(P, synth, n, v):
    offs = synth.pop_offsets(n)
    thr = synth.thresholds(SEED, 0, v)
    eng = P.PcoaEngine(n)
    eng.reserve(CHUNK, 2)
    for v0 in range(0, v, CHUNK):
        eng.accumulate_synthetic(SEED, offs, thr[v0:v0 + CHUNK], v0)
    eng.finalize()
    eng.sync()
    return eng


def s_bytes_per_matvec(n, form):
    if form == 1:
        nb = (n + 1023) // 1024
        return 4.0 * 1024 * 1024 * nb * (nb + 1) / 2
    return 4.0 * n * n


def timed_compute(L, lib, eng):
    """One pcoa_compute(2) with the counters of pcoa_timings alone (the one struct every build fills)."""
    eng._check(lib.pcoa_reset_timings(eng._ctx))
    t0 = time.perf_counter()
    comps, lam, nz = eng.compute(2)
    wall = time.perf_counter() - t0
    t = L.PcoaTimings()
    eng._check(lib.pcoa_get_timings_sized(eng._ctx, ctypes.byref(t), ctypes.sizeof(t)))
    steps = int(t.lanczos_steps)
    out = {"compute_wall_s": wall, "compute_total_s": t.compute_total_seconds, "center_s": t.center_seconds,
           "lanczos_s": t.lanczos_seconds, "lanczos_steps": steps, "lanczos_block_steps": int(t.lanczos_block_steps),
           "eig_method": int(t.eig_method), "matvec_form": int(t.matvec_form), "nonzero_rows": int(nz),
           "eigenvalues": [float(x) for x in lam]}
    if steps > 0:
        out["step_s"] = t.lanczos_seconds / steps
    return out


def leg_measures(n, v):
    L, P, synth = load(False)
    lib = L.load()
    eng = resident_engine(P, synth, n, v)
    out = {"leg": "measures", "n": n, "variants": v, "device": eng.device_info()[0], "per_measure": {}}
    for kind in MEASURES:
        eng.set_similarity(kind)
        eng.compute(2)                                   # warm-up: code objects, workspaces
        runs = [timed_compute(L, lib, eng) for _ in range(3)]
        best = min(runs, key=lambda r: r["compute_wall_s"])
        if "step_s" in best:
            b = s_bytes_per_matvec(n, best["matvec_form"])
            best["s_bytes_per_matvec"] = b
            best["s_bytes_per_s"] = b / best["step_s"]
            best["share_of_copy_ceiling"] = b / best["step_s"] / COPY_CEILING
        best["compute_wall_s_all"] = [r["compute_wall_s"] for r in runs]
        out["per_measure"][kind] = best
    sh = out["per_measure"]["shared"]
    for kind in MEASURES[1:]:
        m = out["per_measure"][kind]
        if "step_s" in m and "step_s" in sh:
            m["step_s_over_shared"] = m["step_s"] / sh["step_s"]
        m["center_s_over_shared"] = m["center_s"] / sh["center_s"] if sh["center_s"] > 0 else None
        m["compute_wall_over_shared"] = m["compute_wall_s"] / sh["compute_wall_s"]
    eng.close()
    print(json.dumps(out))


def leg_ab(n, v):
    other = bool(os.environ.get("PCOA_LIB"))
    L, P, synth = load(other)
    lib = L.load()
    eng = resident_engine(P, synth, n, v)
    eng.compute(2)
    runs = [timed_compute(L, lib, eng) for _ in range(3)]
    best = min(runs, key=lambda r: r["compute_wall_s"])
    best["compute_wall_s_all"] = [r["compute_wall_s"] for r in runs]
    best.update({"leg": "ab", "n": n, "variants": v, "library": "other" if other else "this tree"})
    eng.close()
    print(json.dumps(best))


def child(args, env, limit):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env, timeout=limit)
    except subprocess.TimeoutExpired:
        return {"error": "exceeded its time limit of %d s" % limit, "args": args}
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    if res.returncode != 0 or not lines:
        return {"error": "exit status %d" % res.returncode, "stderr": res.stderr[-2000:], "args": args}
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="2504,20000,100000")
    ap.add_argument("--variants", type=int, default=1 << 17)
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--ab-runs", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg == "measures":
        return leg_measures(a.n, a.variants)
    if a.leg == "ab":
        return leg_ab(a.n, a.variants)
    sizes = [int(t) for t in a.sizes.split(",")]
    L = importlib.import_module("spark-examples_amd._lib")
    report = {"tool": "tools/measure_probe.py", "source_hash": L.source_hash(), "variants": a.variants, "seed": SEED,
              "copy_ceiling_bytes_per_s": COPY_CEILING, "sizes": []}
    here = dict((k, val) for k, val in os.environ.items() if k != "PCOA_LIB")
    for n in sizes:
        r = child(["--leg", "measures", "--n", str(n), "--variants", str(a.variants)], here, a.limit)
        report["sizes"].append(r)
        print(json.dumps(r), flush=True)
        if "error" in r:       # nothing more on a device that has just failed a leg
            break
    if a.ab_lib and not any("error" in r for r in report["sizes"]):
        n = max(sizes)
        ab = {"n": n, "library_other": os.path.relpath(os.path.abspath(a.ab_lib), ROOT), "this_tree": [], "other": []}
        there = dict(here, PCOA_LIB=os.path.abspath(a.ab_lib))
        for _ in range(a.ab_runs):
            for key, env in (("this_tree", here), ("other", there)):
                r = child(["--leg", "ab", "--n", str(n), "--variants", str(a.variants)], env, a.limit)
                ab[key].append(r)
                print(json.dumps(r), flush=True)
                if "error" in r:
                    break
            if any("error" in r for r in ab["this_tree"] + ab["other"]):
                break
        for key in ("this_tree", "other"):
            walls = [r["compute_wall_s"] for r in ab[key] if "compute_wall_s" in r]
            if walls:
                ab[key + "_median_compute_wall_s"] = statistics.median(walls)
                ab[key + "_min_max_compute_wall_s"] = [min(walls), max(walls)]
        report["shared_measure_ab"] = ab
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

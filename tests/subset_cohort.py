"""The planted cohort of the outlier-round tests (test_subset_cpu.py, test_gpu_subset.py) and what is known about it: three
populations of 23 / 22 / 22 samples over 700 variants, with samples 5 and 40 overwritten by near-universal carriers.  The
sets below were worked out with numpy.linalg.eigh and confirmed with the oracle (test_subset_cpu.py recomputes them and
their margins on every run)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 2          # searched: none needed, the oracle agrees with the sets below at the first seed tried
N, V = 67, 700
NUM_PC = 2
# sigma -> the samples each round removes, in round order; the last round removes nobody
EXPECTED = {3.0: [[5, 40], []], 1.8: [[5, 40, 64], [9], []]}
MIN_MARGIN = 0.02  # every sample's largest |z| / sigma stays at least this far from 1, or the fixture is invalid


def planted_cohort():
    """bool [V][N]: x[v, i] = sample i carries variant v."""
    rng = np.random.default_rng(SEED)
    pop = np.repeat([0, 1, 2], [23, 22, 22])
    f = rng.uniform(0.05, 0.5, (V, 3))
    x = rng.random((V, N)) < f[:, pop]
    for i in (5, 40):
        x[:, i] = rng.random(V) < 0.85
    return x


def name_of(i):
    return "S%04d" % i


def z_over_sigma(components, sigma):
    """[n]: per sample the largest |u_c[i] - mean_c| / (sigma sd_c) over the axes (population sd; numpy's own sums -- this is
    the margin check, not the rule under test)."""
    u = np.asarray(components, dtype=np.float64)
    dev = np.abs(u - u.mean(axis=1, keepdims=True))
    return (dev / (sigma * u.std(axis=1, keepdims=True))).max(axis=0)


def rounds_on(compute, s, sigma, iterations, rule):
    """The loop of --outlier-iterations over a dense S with `compute(S_sub) -> [num_pc][m] components`: the removed samples
    (original indices) of every round that applied the rule, the kept indices at the end, and the smallest margin met."""
    kept = np.arange(s.shape[0])
    removed_per_round, margin, done = [], np.inf, 0
    while True:
        u = compute(s[np.ix_(kept, kept)])
        if done == iterations:
            break
        margin = min(margin, float(np.abs(z_over_sigma(u, sigma) - 1.0).min()))
        gone = rule(u, sigma)
        removed_per_round.append([int(i) for i in kept[gone]])
        if not gone.any():
            break
        kept = kept[~gone]
        done += 1
    return removed_per_round, kept, margin


def write_plink(x, prefix, names):
    """x bool [V][n] as a PLINK 1 fileset with A2 the reference allele: a carrier is heterozygous (10), everybody else
    homozygous reference (11); chromosome 17 inside the hosts' default --references."""
    v, n = x.shape
    os.makedirs(os.path.dirname(prefix), exist_ok=True)
    with open(prefix + ".fam", "w") as f:
        for i, nm in enumerate(names):
            f.write("FAM%d %s 0 0 0 -9\n" % (i, nm))
    with open(prefix + ".bim", "w") as f:
        for k in range(v):
            f.write("17\trs%d\t0\t%d\tC\tA\n" % (k, 41196312 + 7 * k))
    bpv = (n + 3) // 4
    codes = np.full((v, bpv * 4), 3, dtype=np.uint8)
    codes[:, :n] = np.where(x, 2, 3)
    quad = codes.reshape(v, bpv, 4)
    out = quad[:, :, 0] | (quad[:, :, 1] << 2) | (quad[:, :, 2] << 4) | (quad[:, :, 3] << 6)
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6c, 0x1b, 0x01]))
        f.write(np.ascontiguousarray(out, dtype=np.uint8).tobytes())


def driver_exe():
    exe = os.path.join(ROOT, "spark-examples_amd", "variants_pca_driver")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "spark-examples_amd", "host")])
    return exe


def run_driver(args):
    return subprocess.run([driver_exe()] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                          timeout=300)


def run_python(args):
    code = ("import sys, importlib; sys.path.insert(0, %r); "
            "sys.exit(importlib.import_module('spark-examples_amd.variants_pca').main(%r))" % (ROOT, list(args)))
    return subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                          timeout=300)

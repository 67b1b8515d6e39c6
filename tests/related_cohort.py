"""The cohort of the related-pairs tests (test_pairs_cpu.py, test_gpu_pairs.py): conftest.planted_callsets with three
duplicates and three first-degree-like relatives planted into it, and the check that the screen's threshold separates them
from everybody else by a margin -- a fixture that does not discriminate fails loudly instead of testing nothing."""
import numpy as np

from conftest import int_gram, planted_callsets
from subset_cohort import driver_exe, name_of, run_driver, run_python, write_plink  # noqa: F401  (the host tests take them from here)

THRESHOLD = 0.35      # --related-min-jaccard of the host tests
MIN_MARGIN = 0.05     # every pair's J / THRESHOLD stays at least this far from 1, or the fixture is invalid
SIZES = [(70, 3000), (260, 2000), (1100, 1500)]   # (n, v); the hosts run the n = 260 cohort
# (smallest planted J, largest other J) at those sizes, to three decimals: what margins() must find again
KNOWN = {70: (0.384, 0.276), 260: (0.501, 0.309), 1100: (0.503, 0.330)}
HOST_N, HOST_V = 260, 2000


def plan(n):
    """(duplicates [(a, b, flips)], relatives [(a, b)]): column b is made from column a."""
    return [(3, 40, 0), (5, 41, 25), (n - 1, 7, 60)], [(10, 50), (11, 51), (12, 52)]


def planted_pairs(n):
    dups, rels = plan(n)
    return sorted((min(a, b), max(a, b)) for a, b in [(a, b) for a, b, _ in dups] + rels)


def related_cohort(n, v):
    """bool [v][n]: x[r, i] = sample i carries variant r.  A duplicate b is a copy of a with `flips` variants toggled; a
    relative b takes a's call at a random half of the variants and keeps its own at the others."""
    rng = np.random.default_rng(n)
    x = planted_callsets(rng, n, v) > 0
    dups, rels = plan(n)
    for a, b, flips in dups:
        x[:, b] = x[:, a]
        at = rng.choice(v, size=flips, replace=False)
        x[at, b] = ~x[at, b]
    for a, b in rels:
        half = rng.random(v) < 0.5
        x[half, b] = x[half, a]
    return x


def jaccard_matrix(s):
    """J(i, j) = S(i, j) / (d_i + d_j - S(i, j)) in double, 0 where the union is empty; the diagonal is set to 0."""
    s = np.asarray(s, dtype=np.int64)
    d = np.diagonal(s)
    u = d[:, None] + d[None, :] - s
    j = np.where(u > 0, s / np.maximum(u, 1), 0.0)
    np.fill_diagonal(j, 0.0)
    return j


def margins(x, threshold=THRESHOLD):
    """(smallest planted J, largest planted J, largest J of any other pair) of the cohort x, after ASSERTING that the planted
    pairs lie above the threshold, every other pair below it, and every pair's J / threshold at least MIN_MARGIN from 1."""
    n = x.shape[1]
    j = np.triu(jaccard_matrix(int_gram(x.astype(np.float32))), 1)
    planted = planted_pairs(n)
    pj = np.array([j[a, b] for a, b in planted])
    rest = j.copy()
    for a, b in planted:
        rest[a, b] = 0.0
    other = float(rest.max())
    assert pj.min() / threshold >= 1.0 + MIN_MARGIN, "fixture invalid: a planted pair at J = %.4f, threshold %.2f" % (pj.min(), threshold)
    assert other / threshold <= 1.0 - MIN_MARGIN, "fixture invalid: an unplanted pair at J = %.4f, threshold %.2f" % (other, threshold)
    return float(pj.min()), float(pj.max()), other


def write_vcf(x, path, names):
    """x bool [V][n] as a VCF inside the hosts' default --references: a carrier is 0/1, everybody else 0/0."""
    cells = np.where(x, "0/1", "0/0")
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n")
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n")
        for k in range(x.shape[0]):
            f.write("chr17\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t%s\n" % (41196312 + 7 * k, "\t".join(cells[k])))

"""The cohort of the KING-robust kinship tests (test_king_cpu.py, test_gpu_king.py): genotypes of three populations whose
allele frequencies differ, up to 20 % missing calls per sample, with three duplicates, two trios and a second child planted
into them -- and the checks that the kinship cutoff separates the planted pairs from everybody else by a margin while no
carrier-Jaccard threshold does.  A fixture that does not discriminate fails loudly instead of testing nothing."""
import os

import numpy as np

from subset_cohort import driver_exe, name_of, run_driver, run_python  # noqa: F401  (the host tests take them from here)

CUTOFF = 0.177        # --king-cutoff of the tests: the usual first-degree cutoff
MIN_MARGIN = 0.05     # every pair's kinship / CUTOFF stays at least this far from 1, or the fixture is invalid
SIZES = [(70, 3000), (260, 2000), (1100, 1500)]   # (n, v); the hosts run the n = 260 cohort
# (smallest planted kinship, largest other kinship) at those sizes, to three decimals: what margins() must find again
KNOWN = {70: (0.245, 0.064), 260: (0.241, 0.098), 1100: (0.248, 0.109)}
HOST_N, HOST_V = 260, 2000
CODE_OF_DOSAGE = np.array([0, 2, 3], dtype=np.uint8)   # A2 alleles 0, 1, 2 -> .bed code 00 (hom A1), 10 (het), 11 (hom A2)


def plan(n):
    """(duplicates [(a, b, flips)], children [(child, parent, parent)]): sample b is made from sample a; each haplotype of a
    child is a per-variant pick of one parent's two."""
    return [(3, 40, 0), (5, 41, 25), (n - 1, 7, 60)], [(50, 10, 13), (51, 11, 14), (52, 10, 13)]


def planted_pairs(n):
    """The 10 pairs of first-degree relatives and duplicates: 3 duplicates, 6 parent-child pairs, the siblings 50-52."""
    dups, kids = plan(n)
    pairs = [(a, b) for a, b, _ in dups] + [(c, p) for c, p, _ in kids] + [(c, q) for c, _, q in kids] + [(50, 52)]
    return sorted((min(a, b), max(a, b)) for a, b in pairs)


def codes(n, v):
    """uint8 [v][n] of PLINK .bed codes (0 hom A1, 1 missing, 2 het, 3 hom A2).  Sample i belongs to population i % 3; a
    variant's frequency in a population is clip(p + N(0, 0.12), 0.02, 0.98) around a shared p ~ U(0.1, 0.9)."""
    rng = np.random.default_rng(n)
    p = rng.uniform(0.1, 0.9, size=v)
    freq = np.clip(p[:, None] + rng.normal(0.0, 0.12, size=(v, 3)), 0.02, 0.98)
    hap = rng.random((2, v, n)) < freq[:, np.arange(n) % 3][None, :, :]
    dups, kids = plan(n)
    for a, b, flips in dups:
        hap[:, :, b] = hap[:, :, a]
        at = rng.choice(v, size=flips, replace=False)
        dosage = (hap[0, at, b].astype(np.int64) + hap[1, at, b] + rng.integers(1, 3, size=flips)) % 3   # another class
        hap[0, at, b], hap[1, at, b] = dosage >= 1, dosage >= 2
    for child, pa, pb in kids:
        for k, parent in enumerate((pa, pb)):
            pick = rng.integers(0, 2, size=v)
            hap[k, :, child] = np.where(pick == 0, hap[0, :, parent], hap[1, :, parent])
    code = CODE_OF_DOSAGE[hap[0].astype(np.int64) + hap[1]]
    rate = rng.uniform(0.0, 0.2, size=n)
    code[rng.random((v, n)) < rate[None, :]] = 1
    return code


def gram(plane):
    """X^T X of a bool [v][n] plane as int64 (exact in float32 up to 2^24 variants)."""
    x = np.asarray(plane, dtype=np.float32)
    return (x.T @ x).astype(np.int64)


def kinship_matrix(vp, code):
    """num / het_sum of every pair in double (0 where het_sum = 0), the diagonal set to 0; vp is variants_pca."""
    _, _, hethet, ibs0, het_sum = vp.king_counts([gram(p) for p in vp.king_planes(code)])
    k = np.where(het_sum > 0, (hethet - 2 * ibs0) / np.maximum(het_sum, 1), 0.0)
    np.fill_diagonal(k, 0.0)
    return k


def margins(vp, code, cutoff=CUTOFF):
    """(smallest planted kinship, largest kinship of any other pair) of the cohort, after ASSERTING that every planted pair has
    kinship / cutoff >= 1 + MIN_MARGIN and every other pair <= 1 - MIN_MARGIN."""
    n = code.shape[1]
    k = kinship_matrix(vp, code)
    planted = planted_pairs(n)
    pk = np.array([k[a, b] for a, b in planted])
    rest = np.triu(k, 1)
    rest[np.tril_indices(n)] = -1.0
    for a, b in planted:
        rest[a, b] = -1.0
    other = float(rest.max())
    assert pk.min() / cutoff >= 1.0 + MIN_MARGIN, "fixture invalid: a planted pair at kinship %.4f, cutoff %.3f" % (pk.min(), cutoff)
    assert other / cutoff <= 1.0 - MIN_MARGIN, "fixture invalid: an unplanted pair at kinship %.4f, cutoff %.3f" % (other, cutoff)
    return float(pk.min()), other


def carriers(code, ref_is_a1=False):
    """bool [v][n]: what pcoa_accumulate_plink_bed decodes as a carrier -- het, and the homozygote of the non-reference allele."""
    return (code == 2) | (code == (3 if ref_is_a1 else 0))


def jaccard_extremes(code):
    """(smallest carrier-Jaccard of a planted pair, largest of any other pair): the second exceeds the first on these cohorts,
    so no --related-min-jaccard separates the relatives from the rest."""
    n = code.shape[1]
    s = gram(carriers(code))
    d = np.diagonal(s)
    u = d[:, None] + d[None, :] - s
    j = np.where(u > 0, s / np.maximum(u, 1), 0.0)
    planted = planted_pairs(n)
    lo = min(j[a, b] for a, b in planted)
    rest = j.copy()
    rest[np.tril_indices(n)] = -1.0
    for a, b in planted:
        rest[a, b] = -1.0
    return float(lo), float(rest.max())


def bed_rows(code):
    """uint8 [v][ceil(n / 4)]: the variant-major .bed rows of the codes (sample i in bits 2 (i % 4) of byte i / 4; the padding
    codes of the last byte are 00)."""
    v, n = code.shape
    padded = np.zeros((v, (n + 3) // 4 * 4), dtype=np.uint8)
    padded[:, :n] = code
    q = padded.reshape(v, -1, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def write_plink(code, prefix, names):
    """prefix.bed / .bim / .fam of the codes, variant-major (the magic bytes 6c 1b 01)."""
    v, n = code.shape
    os.makedirs(os.path.dirname(prefix), exist_ok=True)
    with open(prefix + ".fam", "w") as f:
        for i, name in enumerate(names):
            f.write("FAM%d %s 0 0 0 -9\n" % (i, name))
    with open(prefix + ".bim", "w") as f:
        for k in range(v):
            f.write("17\trs%d\t0\t%d\tC\tA\n" % (k, 41196312 + 7 * k))
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(bed_rows(code).tobytes())

"""The numpy and Python statement of the variant and sample QC of a GRM engine (include/pcoa.h, "variant and sample QC on the
resident GRM store"), imported by tests/test_grm_qc_cpu.py and tests/test_gpu_grm_qc.py.  No tests in here.

A cohort is `codes`, [V][N] uint8 PLINK codes, and ref_is_a1, as in tests/test_grm_cpu.py.  The Hardy-Weinberg exact test is
stated with Python integers and fractions.Fraction: the reference is exact, the kernel's fp64 value is held to it."""
import functools
import math
from fractions import Fraction

import numpy as np

from test_grm_cpu import spec_grm_counts

TIE = Fraction(2 ** 24 + 1, 2 ** 24)          # P(k) <= P(h) (1 + 2^-24) is counted
TIE_BAND = Fraction(1, 2 ** 20)               # a test cohort has no term ratio this close to 1 other than exactly 1


@functools.lru_cache(maxsize=None)
def hwe_terms(n, h, o):
    """(ks, weights): the heterozygote counts k of R's parity in [0, R] and integers proportional to P(k):
    w(k) = n! 2^k / (((R - k) / 2)! k! (n - (R + k) / 2)!).  None when n = 0 or R = 0."""
    a = h + 2 * o
    r_ = min(a, 2 * n - a)
    if n == 0 or r_ == 0:
        return None
    ks, ws = [], []
    k = r_ & 1
    r, c = (r_ - k) // 2, n - (r_ + k) // 2
    w = math.factorial(n) // (math.factorial(r) * math.factorial(k) * math.factorial(c)) * 2 ** k
    while True:
        ks.append(k)
        ws.append(w)
        if k + 2 > r_:
            break
        num = w * 4 * r * c
        den = (k + 2) * (k + 1)
        assert num % den == 0
        w = num // den
        k, r, c = k + 2, r - 1, c - 1
    return ks, ws


@functools.lru_cache(maxsize=None)
def spec_hwe_exact(n, h, o):
    """p_v as a Fraction: the sum of P(k) over the k with P(k) <= P(h) (1 + 2^-24), over the sum of all P(k)."""
    t = hwe_terms(n, h, o)
    if t is None:
        return Fraction(1)
    ks, ws = t
    wh = ws[ks.index(h)]
    return Fraction(sum(w for w in ws if w <= wh * TIE), sum(ws))


@functools.lru_cache(maxsize=None)
def wrong_hwe_one_sided(n, h, o):
    """A plausible wrong kernel: the lower tail alone, P(het <= h) (the test for an excess of homozygotes)."""
    t = hwe_terms(n, h, o)
    if t is None:
        return Fraction(1)
    ks, ws = t
    return Fraction(sum(w for k, w in zip(ks, ws) if k <= h), sum(ws))


def near_ties(n, h, o):
    """The k whose P(k) / P(h) lies in [1 - 2^-20, 1 + 2^-20] without being exactly 1: a cohort must have none, so that the fp64
    comparison of the kernel and the exact one count the same terms."""
    t = hwe_terms(n, h, o)
    if t is None:
        return []
    ks, ws = t
    wh = ws[ks.index(h)]
    return [k for k, w in zip(ks, ws) if w != wh and wh * (1 - TIE_BAND) <= w <= wh * (1 + TIE_BAND)]


def hwe_bound(n_samples):
    """Relative: every term is at most 3 R / 2 roundings away from the mode, each of the two sums of positive terms adds at most
    R / 2 + 1, the quotient one more; R <= N."""
    return Fraction(4 * n_samples + 32, 2 ** 53)


def hwe_of_counts(counts):
    """[V] Fractions of [V][3] counts"""
    return [spec_hwe_exact(int(n), int(h), int(o)) for n, h, o in np.asarray(counts)]


def hwe_within(got, exact, n_samples):
    """the kernel's value against the exact one: relative (4 N + 32) 2^-53; below 2^-900 only a value in [0, 2^-800]"""
    got = float(got)
    if exact < Fraction(1, 2 ** 900):
        return 0.0 <= got <= 2.0 ** -800
    return abs(Fraction(got) - exact) <= hwe_bound(n_samples) * exact


def spec_used(counts, n_samples, min_maf=0.0, max_missing=1.0, hwe_min_p=0.0, keep=None, missing_lt=False):
    """used_v under min_maf, the two filters and a keep mask, in the header's expressions; the p-values are the exact ones.
    missing_lt: the deliberately wrong missing test, < in place of <=."""
    counts = np.asarray(counts)
    n = counts[:, 0].astype(np.int64)
    a = counts[:, 1].astype(np.int64) + 2 * counts[:, 2].astype(np.int64)
    nf = n.astype(np.float64)
    used = (n > 0) & (a > 0) & (a < 2 * n) & (np.minimum(a, 2 * n - a).astype(np.float64) >= min_maf * (2.0 * nf))
    miss = (n_samples - n).astype(np.float64)
    lim = max_missing * float(n_samples)
    used &= (miss < lim) if missing_lt else (miss <= lim)
    if hwe_min_p != 0.0:
        thr = Fraction(hwe_min_p)
        used &= np.array([p >= thr for p in hwe_of_counts(counts)], dtype=bool)
    if keep is not None:
        used &= np.asarray(keep, dtype=bool)
    return used


def spec_fails(counts, n_samples, min_maf=0.0, max_missing=1.0, hwe_min_p=0.0):
    """(MAF, missing, HWE): the variants that fail each test, judged alone (pcoa_grm_qc_stats)"""
    counts = np.asarray(counts)
    v = counts.shape[0]
    maf = v - int(spec_used(counts, n_samples, min_maf).sum())
    n = counts[:, 0].astype(np.int64)
    missing = int((~((n_samples - n).astype(np.float64) <= max_missing * float(n_samples))).sum())
    hwe = 0 if hwe_min_p == 0.0 else sum(1 for p in hwe_of_counts(counts) if p < Fraction(hwe_min_p))
    return maf, missing, hwe


def spec_sample_counts(codes, ref_is_a1, rows=None):
    """[N][3] int64: the rows (all, or those of the boolean mask `rows`) at which a sample is called, het, hom non-reference"""
    codes = np.asarray(codes)
    if rows is not None:
        codes = codes[np.asarray(rows, dtype=bool)]
    hom = 3 if ref_is_a1 else 0
    return np.stack([(codes != 1).sum(axis=0), (codes == 2).sum(axis=0), (codes == hom).sum(axis=0)], axis=1).astype(np.int64)


# ---- cohorts ----------------------------------------------------------------------------------------------------------------
def planted_hwe_rows(n, seed):
    """rows at N = n that a random cohort does not reach: all het, no het at an intermediate frequency (p far below 2^-900 at
    n = 4096), two rows in equilibrium, a singleton, a row with one called sample, and a sparse row; A2 is the reference"""
    rng = np.random.default_rng(seed)
    rows = []
    rows.append(np.full(n, 2, np.uint8))                                                  # all het
    r = np.full(n, 3, np.uint8)
    r[: n // 2] = 0
    rows.append(rng.permutation(r))                                                       # no het, frequency 1 / 2
    for p in (0.5, 0.2):                                                                  # in equilibrium
        g = (rng.random(n) < p).astype(np.uint8) + (rng.random(n) < p).astype(np.uint8)
        rows.append(np.array([3, 2, 0], dtype=np.uint8)[g])
    r = np.full(n, 3, np.uint8)
    r[n // 3] = 2
    rows.append(r)                                                                        # a singleton
    r = np.full(n, 1, np.uint8)
    r[n // 5] = 2
    rows.append(r)                                                                        # one called sample, het
    g = (rng.random(n) < 0.3).astype(np.uint8) + (rng.random(n) < 0.3).astype(np.uint8)
    r = np.array([3, 2, 0], dtype=np.uint8)[g]
    r[rng.random(n) < 0.6] = 1
    rows.append(r)                                                                        # sparsely called
    r = np.full(n, 3, np.uint8)
    r[: n // 8] = 0
    r[n // 8: n // 8 + 6] = 2
    rows.append(rng.permutation(r))                                                       # few het at a low frequency
    return np.stack(rows)


def filter_cohort(n, v, seed):
    """A cohort for the filter tests at n a multiple of 8: Hardy-Weinberg rows with little missingness, then planted rows --
    missing shares of exactly 1/8 (kept at max_missing = 0.125), one above and one below it, rows far from equilibrium (het
    deficit and het excess), monomorphic and uncalled rows."""
    from test_grm_cpu import edge_rows, random_codes
    assert n % 8 == 0
    rng = np.random.default_rng(seed)
    codes = edge_rows(random_codes(rng, v, n, missing=0.02, lo=0.1, hi=0.9))
    codes[:, 1] = codes[:, 2]                      # (edge_rows leaves sample 1 uncalled: here it is called like sample 2)
    for j, extra in enumerate((0, 0, 1, -1, 0, 2, -2)):
        r = 10 + 3 * j
        row = codes[r]
        row[row == 1] = 3
        row[rng.choice(n, size=n // 8 + extra, replace=False)] = 1
    for j in range(6):                             # far from equilibrium
        r = 40 + 5 * j
        row = np.full(n, 3, np.uint8)
        if j % 2 == 0:
            row[: n // 3] = 0                      # no het
        else:
            row[: (3 * n) // 4] = 2                # het excess
        codes[r] = rng.permutation(row)
    return codes

"""The cohorts of the similarity-measure tests (test_measure_cpu.py, test_gpu_measure.py) and what is known about them.

exact_groups(n): sample i belongs to group i % 4 and every group carries its own 256 variants, so d_i = 256, q_i = 1 / 16,
K in {0, 1} under both measures, r_i = n / 4, rowmean = mm = 0.25 and B in {0.75, -0.25} -- all exact in fp64, and for an
integer x with |x| <= 8 every partial sum of B x is a multiple of 0.25 far below 2^53: every form of the mat-vec, in every
order of addition, must return the numpy product bit for bit.  exact_case() ASSERTS all of that at the shape it is asked for.

populations(n, v): three populations (sample i in population i % 3, so every tile holds all three) with different allele
frequencies AND different carrier rates (0.3, 0.6, 0.9 of the population's frequency), so that d_i varies about 3x across
samples -- the situation the measures exist for.  eig_reference() ASSERTS that the two leading eigenvalues of the reference B
are separated from each other and from the third by MIN_GAP of lambda_1, so the eigenvectors are conditioned well enough for
the 1e-6 bar of the eigenpair tests; a shape that fails it needs another shape or seed, not another bar."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from conftest import int_gram, load_pkg  # noqa: E402
from subset_cohort import driver_exe, name_of, run_driver, run_python  # noqa: E402,F401  (the host tests take them from here)
from related_cohort import write_vcf  # noqa: E402,F401

MEASURES = ("jaccard", "cosine")
KIND = {"shared": 0, "jaccard": 1, "cosine": 2}      # PCOA_SIMILARITY_*

# ---- shapes of the GPU tests (the CPU tests run the helpers' assertions at every one of them) ----------------------------------
EXACT_TILE_N = (4, 64, 1020, 1024, 1028, 1044, 1540, 2044, 2048, 2052, 3076)     # form 1 (and 0, 2)
EXACT_ROW_N = (252, 256, 260, 768, 772, 1024, 1028, 1796)                        # forms 0 and 2
ROUNDED_N = (5, 63, 65, 260, 513, 1025, 1044, 2052)
ROUNDED_V = 700
I64_N = (65, 772, 1028)
I64_SCALE = 2 ** 22
I64_V = 3000        # variants of the int64 cases: d_i reaches 512, so 2^22 S leaves int32 (at 700 variants it would not)
EIG_N = (6, 20, 260, 1025, 2052)
HOST_N, HOST_V = 40, 400
NUM_PC = 2
MIN_GAP = 0.05
EMPTY = (1, 3)     # the two samples the rounded entry cases leave without a carrier (both below the smallest N)


def vp():
    return load_pkg("variants_pca")


# ---- the exact cohort -----------------------------------------------------------------------------------------------------------
def exact_groups(n):
    """bool [1024][n]: x[v, i] = sample i carries variant v  <=>  v // 256 == i % 4."""
    assert n % 4 == 0 and n >= 4
    return (np.arange(1024)[:, None] // 256) == (np.arange(n)[None, :] % 4)


def integer_vectors(n, seed=17):
    """[3, n] integer vectors with |x| <= 8."""
    return np.random.default_rng(seed + n).integers(-8, 9, size=(3, n)).astype(np.float64)


def exact_case(n, kind):
    """(S int64, B float64, x [3, n], B x [n, 3]) of the exact cohort, after asserting every closed form in numpy."""
    V = vp()
    s = int_gram(exact_groups(n))
    same = (np.arange(n)[:, None] % 4) == (np.arange(n)[None, :] % 4)
    assert np.array_equal(s, np.where(same, 256, 0)) and np.all(np.diagonal(s) == 256)
    k = V.similarity_measure(s, kind)
    assert np.array_equal(k, same.astype(np.float64)), kind                       # K in {0, 1}, whichever measure
    b, r, mm, nz = V.centred_measure(k)
    assert np.all(r == n / 4) and mm == 0.25 and nz == n
    assert np.array_equal(b, np.where(same, 0.75, -0.25))
    xs = integer_vectors(n)
    assert np.abs(xs).max() <= 8
    ref = b @ xs.T                                                                # multiples of 0.25 below 8 n: exact in any order
    assert np.array_equal(4 * ref, np.rint(4 * ref)) and np.abs(ref).max() < 2.0 ** 40
    i64 = (4 * b).astype(np.int64) @ xs.T.astype(np.int64)                        # the float64 product itself against int64
    assert np.array_equal(4 * ref, i64.astype(np.float64))
    assert not (b @ np.ones(n)).any()
    return s, b, xs, ref


# ---- the rounded cohorts --------------------------------------------------------------------------------------------------------
def populations(n, v, seed=None, empty=()):
    """bool [v][n]; the samples named in `empty` carry nothing."""
    rng = np.random.default_rng(n if seed is None else seed)
    pop = np.arange(n) % 3
    f = rng.uniform(0.05, 0.5, (v, 3)) * np.array([0.3, 0.6, 0.9])[None, :]
    x = rng.random((v, n)) < f[:, pop]
    for i in empty:
        x[:, i] = False
    return x


def measure_longdouble(s, kind):
    """The rule of variants_pca.similarity_measure evaluated in np.longdouble from the integer S: the reference the rounded
    cases compare against (its own error is 2^-11 of the fp64 unit roundoff where long double is x87 extended)."""
    s = np.asarray(s, dtype=np.int64)
    ld = np.longdouble
    d = np.diagonal(s)
    sl = s.astype(ld)
    if kind == "jaccard":
        u = d[:, None] + d[None, :] - s
        return np.where(u > 0, sl / np.where(u > 0, u, 1).astype(ld), ld(0))
    assert kind == "cosine"
    q = np.where(d > 0, ld(1) / np.sqrt(np.where(d > 0, d, 1).astype(ld)), ld(0))
    return (sl * q[:, None]) * q[None, :]


def reference(s, kind):
    """(B, r, mm, nonzero_rows) in np.longdouble from the integer S."""
    return vp().centred_measure(measure_longdouble(s, kind))


def entry_bound(n):
    """|B_device - B_reference| per entry: (4 N + 32) 2^-53.  |K| <= 1 with at most 4 roundings (a division that need not be
    correctly rounded, or two products and q's own rounding); a row sum of N terms <= 1 in any order errs by at most
    N^2 2^-53, hence N 2^-53 on a mean; the matrix mean errs by the same order again; three add / subtracts on magnitudes
    <= 2.  A wrong d_j, a dropped term or a misplaced column is 10^6 or more times larger."""
    return (4 * n + 32) * 2.0 ** -53


def row_sum_bound(n):
    return n * n * 2.0 ** -53


def matvec_bound(n, b_abs, x):
    """|y_i - ref_i| <= N 2^-52 (|B| |x|)_i + (4 N + 32) 2^-53 ||x||_1: the summation bound of the existing forms test (N - 1
    additions and one product rounding per term, any order, doubled) plus the entry bound above on every term."""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    return n * 2.0 ** -52 * (b_abs @ ax) + entry_bound(n) * ax.sum()


def eig_reference(s, kind, num_pc=NUM_PC):
    """(eigenvalues [num_pc], vectors [n, num_pc], B float64, relative gaps) of the reference B by numpy.linalg.eigh, largest
    |lambda| first; asserts the gaps (lambda_k - lambda_{k+1}) / lambda_1 >= MIN_GAP for k = 1 .. num_pc."""
    V = vp()
    b = V.centred_measure(V.similarity_measure(s, kind))[0]
    w, z = np.linalg.eigh(b)
    order = np.argsort(-np.abs(w), kind="stable")
    w, z = w[order], z[:, order]
    assert np.all(w[:num_pc] > 0)
    gaps = [(w[k] - w[k + 1]) / w[0] for k in range(num_pc)]
    assert min(gaps) >= MIN_GAP, "fixture invalid: N = %d, %s: relative gaps %s" % (s.shape[0], kind, gaps)
    return w[:num_pc], z[:, :num_pc], b, gaps


def private_populations(n, v, seed=None):
    """bool [v][n] for the cohorts below the Lanczos path (N = 6, 20): a handful of samples under a Jaccard or cosine
    measure is K = I + small, a nearly flat spectrum, unless the populations are sharply drawn -- every variant is private to
    one population (carried at 0.95 there, 0.02 elsewhere), times carrier rates of 0.4, 0.65, 0.95 (d_i varies 2 - 3x)."""
    rng = np.random.default_rng(n if seed is None else seed)
    pop = np.arange(n) % 3
    home = rng.integers(0, 3, size=v)
    f = np.where(home[:, None] == np.arange(3)[None, :], 0.95, 0.02) * np.array([0.4, 0.65, 0.95])[None, :]
    return rng.random((v, n)) < f[:, pop]


HOST_SEED = 4      # searched: the first seed at which populations(40, 400) has its gaps under both measures (seed 40: 0.03)


def eig_cohort(n):
    """The cohort of the eigenpair cases at N = n (nobody empty)."""
    if n == HOST_N:
        return populations(HOST_N, HOST_V, seed=HOST_SEED)
    return private_populations(n, ROUNDED_V) if n < 32 else populations(n, ROUNDED_V, seed=1000 + n)


def edge_columns(n):
    """Columns on both sides of every tile, half-tile and quad-group edge."""
    return sorted(set(k for k in (0, 3, 4, 255, 256, 511, 512, 1023, 1024, 1027, 1028, 1535, 1536, n - 4, n - 1) if 0 <= k < n))

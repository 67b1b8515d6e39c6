"""The cohorts of the pairwise-complete similarity tests (test_complete_cpu.py, test_gpu_complete.py) and what is known about
them.  The rule is variants_pca.call_complete_measure: K = S / M, M(i, j) = the variants at which samples i and j are both called.

exact_calls(n, extra): V = 256 (4 + extra) variants in blocks of 256.  Sample i carries variant v iff v // 256 == i % 4, and is
CALLED only on its own block and on the `extra` trailing blocks; everywhere else its call is missing.  So
    same group        s = 256,  M = 256 (1 + extra),  K = 1 / (1 + extra) = kappa
    different groups  s = 0,    M = 256 extra,        K = 0            (extra = 0: M = 0, the guard, on 3/4 of the entries)
r_i = n kappa / 4, mm = kappa / 4 and B in {0.75 kappa, -0.25 kappa} -- kappa in {1, 1/2, 1/4}, all exact in fp64, and for an
integer x with |x| <= 8 every partial sum of B x is a multiple of kappa / 4 far below 2^53: every form of the mat-vec, in every
order of addition, must return the numpy product bit for bit.  exact_case() ASSERTS all of that at the shape it is asked for.

populations_with_missing(n, v, seed): measure_cohort's populations (private_populations below N = 32) with a per-sample
missing rate drawn from U(0, 0.4), unrelated to the population; the carriers are the CALLED carriers.  s <= M everywhere (a
shared carrier is jointly called), so |K| <= 1 with one division and exact integer conversions: measure_cohort's entry_bound,
row_sum_bound and matvec_bound apply unchanged.  eig_reference() asserts positive leading eigenvalues and the relative gaps."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import measure_cohort as M  # noqa: E402
from conftest import int_gram, load_pkg  # noqa: E402
from measure_cohort import (EIG_N, EXACT_ROW_N, EXACT_TILE_N, HOST_N, HOST_V, I64_N, I64_SCALE, I64_V, MIN_GAP, NUM_PC,  # noqa: E402,F401
                            ROUNDED_N, ROUNDED_V, edge_columns, entry_bound, integer_vectors, matvec_bound, row_sum_bound,
                            driver_exe, name_of, run_driver, run_python)

EXTRAS = (0, 1, 3)
DECODE_N = (5, 63, 65, 260)
DECODE_V = (1, 131, 1000)
DECODE_CALL_ROWS = 37


def vp():
    return load_pkg("variants_pca")


# ---- the exact cohort -----------------------------------------------------------------------------------------------------------
def exact_calls(n, extra):
    """(carriers bool [V][n], missing bool [V][n], V)."""
    assert n % 4 == 0 and n >= 4 and extra in EXTRAS
    v = 256 * (4 + extra)
    block = np.arange(v)[:, None] // 256
    group = np.arange(n)[None, :] % 4
    carriers = block == group
    called = carriers | (block >= 4)
    return carriers, ~called, v


def exact_case(n, extra):
    """(S, Q int64, V, B float64, x [3, n], B x [n, 3]) of the exact cohort, after asserting every closed form in numpy."""
    V = vp()
    carriers, missing, v = exact_calls(n, extra)
    s, q = int_gram(carriers), int_gram(missing)
    same = (np.arange(n)[:, None] % 4) == (np.arange(n)[None, :] % 4)
    kappa = 1.0 / (1 + extra)
    assert np.array_equal(s, np.where(same, 256, 0))
    c = v - np.diagonal(q)
    assert np.all(c == 256 * (1 + extra))
    m = c[:, None] + c[None, :] - v + q
    assert np.array_equal(m, np.where(same, 256 * (1 + extra), 256 * extra))
    k = V.call_complete_measure(s, q, v)
    assert np.array_equal(k, np.where(same, kappa, 0.0))
    if extra == 0:
        assert (m == 0).sum() == 3 * n * n // 4                                  # the M > 0 guard on 3/4 of the entries
    b, r, mm, nz = V.centred_measure(k)
    assert np.all(r == n * kappa / 4) and mm == kappa / 4 and nz == n
    assert np.array_equal(b, np.where(same, 0.75 * kappa, -0.25 * kappa))
    xs = integer_vectors(n)
    assert np.abs(xs).max() <= 8
    ref = b @ xs.T                                                                # multiples of kappa / 4 below 8 n: exact in any order
    unit = 4 * (1 + extra)
    assert np.array_equal(unit * ref, np.rint(unit * ref)) and np.abs(ref).max() < 2.0 ** 40
    i64 = np.rint(unit * b).astype(np.int64) @ xs.T.astype(np.int64)              # the float64 product itself against int64
    assert np.array_equal(unit * b, np.rint(unit * b)) and np.array_equal(unit * ref, i64.astype(np.float64))
    assert not (b @ np.ones(n)).any()
    return s, q, v, b, xs, ref


# ---- the rounded cohorts --------------------------------------------------------------------------------------------------------
def populations_with_missing(n, v, seed=None, all_missing=(), called_empty=()):
    """(carriers bool [v][n], missing bool [v][n], rate [n]).  The samples in `all_missing` have no call at all, those in
    `called_empty` are called everywhere and carry nothing."""
    seed = n if seed is None else seed
    x = M.private_populations(n, v, seed) if n < 32 else M.populations(n, v, seed)
    rng = np.random.default_rng(seed + 7919)
    rate = rng.uniform(0.0, 0.4, n)
    missing = rng.random((v, n)) < rate[None, :]
    for i in all_missing:
        missing[:, i] = True
    for i in called_empty:
        missing[:, i] = False
        x[:, i] = False
    return x & ~missing, missing, rate


def measure_longdouble(s, q, v):
    """The rule evaluated in np.longdouble from the integer matrices: the reference the rounded cases compare against."""
    s, q = np.asarray(s, dtype=np.int64), np.asarray(q, dtype=np.int64)
    ld = np.longdouble
    c = int(v) - np.diagonal(q)
    m = c[:, None] + c[None, :] - int(v) + q
    assert np.all(s <= np.maximum(m, 0)) and np.all(s >= 0)                      # a shared carrier is jointly called: |K| <= 1
    return np.where(m > 0, s.astype(ld) / np.where(m > 0, m, 1).astype(ld), ld(0))


def reference(s, q, v):
    """(B, r, mm, nonzero_rows) in np.longdouble from the integer matrices."""
    return vp().centred_measure(measure_longdouble(s, q, v))


def eig_reference(s, q, v, num_pc=NUM_PC):
    """(eigenvalues [num_pc], vectors [n, num_pc], B float64, relative gaps) of the reference B by numpy.linalg.eigh, largest
    |lambda| first; asserts that the leading eigenvalues are positive (K is not positive semi-definite in general) and the
    gaps (lambda_k - lambda_{k+1}) / lambda_1 >= MIN_GAP for k = 1 .. num_pc."""
    V = vp()
    b = V.centred_measure(V.call_complete_measure(s, q, v))[0]
    w, z = np.linalg.eigh(b)
    order = np.argsort(-np.abs(w), kind="stable")
    w, z = w[order], z[:, order]
    assert np.all(w[:num_pc] > 0), "fixture invalid: N = %d: leading eigenvalues %s" % (s.shape[0], w[:num_pc])
    gaps = [(w[k] - w[k + 1]) / w[0] for k in range(num_pc)]
    assert min(gaps) >= MIN_GAP, "fixture invalid: N = %d: relative gaps %s" % (s.shape[0], gaps)
    return w[:num_pc], z[:, :num_pc], b, gaps


HOST_SEED = 1      # searched: the first seed at which populations_with_missing(40, 400) has its gaps (seed 0: 0.03, seed 4: 0.01)


def i64_cohort(n):
    """(carriers, missing, S, Q, V) of the int64 cases: S reaches 512, so 2^22 S leaves int32."""
    x, m, _ = populations_with_missing(n, I64_V)
    s, q = int_gram(x), int_gram(m)
    assert (s * I64_SCALE).max() >= 2 ** 31
    return x, m, s, q, I64_V


def eig_cohort(n):
    """(carriers, missing) of the eigenpair cases at N = n."""
    if n == HOST_N:
        return populations_with_missing(HOST_N, HOST_V, seed=HOST_SEED)[:2]
    return populations_with_missing(n, ROUNDED_V, seed=1000 + n)[:2]


# ---- PLINK .bed rows ------------------------------------------------------------------------------------------------------------
def bed_rows(carriers, missing, ref_is_a1=False, seed=0, row_bytes=None, pad_code=1):
    """uint8 [V][row_bytes] raw .bed rows: a missing call is code 01; a carrier is the het code 10 or the homozygous
    non-reference code (00 with A2 the reference, 11 with A1), a called non-carrier the homozygous reference code.  The
    padding pairs of the last byte (samples >= N) hold pad_code (01: they would be missing calls if they were decoded)."""
    v, n = carriers.shape
    rng = np.random.default_rng(seed + 31 * n + v)
    hom_alt, hom_ref = (3, 0) if ref_is_a1 else (0, 3)
    codes = np.where(carriers, np.where(rng.random((v, n)) < 0.5, 2, hom_alt), hom_ref)
    codes = np.where(missing, 1, codes).astype(np.uint8)
    nb = (n + 3) // 4
    padded = np.full((v, 4 * nb), pad_code, dtype=np.uint8)
    padded[:, :n] = codes
    quad = padded.reshape(v, nb, 4)
    rows = (quad[:, :, 0] | (quad[:, :, 1] << 2) | (quad[:, :, 2] << 4) | (quad[:, :, 3] << 6)).astype(np.uint8)
    if row_bytes is not None and row_bytes > nb:
        wide = rng.integers(0, 256, size=(v, row_bytes), dtype=np.uint8)         # what lies behind a row is not the row's
        wide[:, :nb] = rows
        rows = wide
    return np.ascontiguousarray(rows)


def decode_pair(rows, n, ref_is_a1=False):
    """numpy restatement of plink_bed_to_bits_pair_kernel: (carriers bool [V][n], missing bool [V][n]).  Sample s is in bits
    2 (s % 4) of byte s / 4; code = 2 hi + lo: 00 hom A1, 01 missing, 10 het, 11 hom A2.  Carrier (hasVariation with A2 the
    reference): 00 or 10; with A1 the reference: 11 or 10.  Missing: 01 under either."""
    rows = np.asarray(rows, dtype=np.uint8)
    s = np.arange(n)
    code = (rows[:, s // 4] >> (2 * (s % 4))[None, :]) & 3
    carriers = (code == 2) | (code == (3 if ref_is_a1 else 0))
    return carriers, code == 1


def random_codes(n, v, seed):
    """uint8 [v][ceil(n / 4)]: uniformly random codes, the padding pairs of the last byte set to 01."""
    rng = np.random.default_rng(seed)
    nb = (n + 3) // 4
    codes = np.full((v, 4 * nb), 1, dtype=np.uint8)
    codes[:, :n] = rng.integers(0, 4, size=(v, n), dtype=np.uint8)
    quad = codes.reshape(v, nb, 4)
    return np.ascontiguousarray((quad[:, :, 0] | (quad[:, :, 1] << 2) | (quad[:, :, 2] << 4) | (quad[:, :, 3] << 6)).astype(np.uint8))


# ---- the hosts' fileset ---------------------------------------------------------------------------------------------------------
def write_plink(prefix, carriers, missing, names):
    """prefix.bed / .bim / .fam of the cohort: A2 the reference allele, variant-major, chromosome 17 inside the hosts' default
    --references (as subset_cohort.write_plink), missing calls as code 01."""
    v, n = carriers.shape
    os.makedirs(os.path.dirname(prefix), exist_ok=True)
    with open(prefix + ".fam", "w") as f:
        for i, nm in enumerate(names):
            f.write("FAM%d %s 0 0 0 -9\n" % (i, nm))
    with open(prefix + ".bim", "w") as f:
        for k in range(v):
            f.write("17\trs%d\t0\t%d\tC\tA\n" % (k, 41196312 + 7 * k))
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(bed_rows(carriers, missing, pad_code=0).tobytes())


def call_rate_lines(names, missing):
    """The lines of --call-rate-output-path: name, called variants c_i, V, rate with six decimals."""
    v = missing.shape[0]
    c = v - missing.sum(axis=0)
    return ["%s\t%d\t%d\t%.6f" % (nm, int(ci), v, (float(ci) / v) if v else 0.0) for nm, ci in zip(names, c)]

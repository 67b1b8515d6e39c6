"""Numpy twins of the band passes over a strip (csrc/center.hip: strip_band_kernel / strip_finish_kernel behind
pcoa_strip_col_sums and pcoa_strip_matvec[_device]; project_band_kernel / project_finish_kernel behind pcoa_project), the
cohorts they are compared on and the shape lists of tests/test_gpu_strip_band.py.  No GPU, no test.

The twins restate the CONTRACT -- include/pcoa.h and the comments of center.hip -- operation by operation: every fp64
operation rounded on its own (no fused multiply-add), rows of a 256-row band added in order into an accumulator that
starts at 0.0, the bands' accumulators added in order into a total that starts at 0.0.  They were not fitted to the device.

EXACT cohorts: every term and every partial sum is an integer far below 2^53, so any order of addition gives the same double
and the reference is plain int64 arithmetic; a failure there is a wrong TERM (an index, a mask, a pipeline slot, lo + hi).
ROUNDED cohorts: real-valued means / vectors; the device must return the twin's doubles bit for bit, which holds only if the
order and the rounding are the documented ones."""
import functools

import numpy as np

# ---- the constants of center.hip the shapes below are tied to
BAND = 256        # STRIP_BAND: rows of one band (one accumulator per band and column)
DEPTH = 4         # STRIP_NB: rows in flight; prologue of 4 loads, steady loop while k + 8 <= rows, two drain blocks of 4
WAVE_COLS = 256   # columns of one wave (a lane owns lane + 64 q, q < 4); FULL / masked is decided per wave
WG_COLS = 1024    # columns of one workgroup (4 waves); blockIdx.x = column / 1024
HI = 3 * 2 ** 31  # added to every entry of an "int64 part" variant: nothing fits int32, S lives in the int64 matrix
POISON32 = 2 ** 30 + 12345   # rows >= n_ref of a cross strip that is meant to stay int32
POISON64 = 2 ** 40 + 12345   # ... and of one with an int64 part (a single such entry moves the whole strip to int64)
SMALLEST_N = 1    # pcoa_create_strip accepts any n_samples >= 1 (strip (0, 1)): one row, the first drain block alone

# ---- shapes (n, col0, cols), cols <= n - col0
# row tails of the 4-deep pipeline behind one full band: n - 256 = 1, 2, 3 (first drain block only, 1..3 slots), 4 (prologue
# exactly), 5, 7 (second drain block 1 and 3 slots), 8 (one steady iteration, empty drains), 9, 12; 512 = two full bands, 513
ROW_TAILS = [BAND + d for d in (1, 2, 3, 4, 5, 7, 8, 9, 12)] + [2 * BAND, 2 * BAND + 1]
# fewer rows than one band: 33 (8 steady iterations + 1), 64, 255 (band minus one), 256 (one band exactly);
# DEPTH and DEPTH + 1 rows: the prologue alone / one row in the second drain block
SHORT_ROWS = [DEPTH, DEPTH + 1, 33, 64, BAND - 1, BAND]
# the 1,024-column workgroup: 1289 = 1024 + 256 + 9 -> a second workgroup with one full wave and a 9-column masked wave;
# (7, 1023 / 1024 / 1025): one column short of, exactly, one column past a workgroup; 1536 = 1024 + 2 full waves, 6 bands
WIDE = {1289: [(0, 1289), (7, 1023), (7, 1024), (7, 1025), (8, 1281), (1000, 289)],
        1536: [(0, 1536), (256, 1024)]}


def tail_strips(n):
    """(0, n): one full wave + a masked wave (a single column at n = 257); 65 = one lane past q = 0 -> q = 1 of lane 0;
    (5, 1) one column; (3, 63) / (1, 64): one short of / exactly the lanes of a wave, col0 != 0."""
    return [(0, n), (n - 65, 65), (5, 1), (3, 63), (1, 64)]


def strip_shapes():
    out = [(n, c0, w) for n in ROW_TAILS for (c0, w) in tail_strips(n)]
    out += [(n, c0, w) for n in SHORT_ROWS for (c0, w) in ((0, n), (n - 1, 1))]
    out += [(SMALLEST_N, SMALLEST_N - 1, 1)]
    out += [(n, c0, w) for n in sorted(WIDE) for (c0, w) in WIDE[n]]
    assert all(w >= 1 and c0 >= 0 and c0 + w <= n for n, c0, w in out) and len(out) == len(set(out))
    return out


# the rounded mat-vec with an int64 part: the two wide n and three row tails (1, 3 and 7 rows behind a band)
I64_ROUNDED_STRIPS = [(1289, 8, 1281), (1536, 256, 1024), (257, 0, 257), (259, 194, 65), (263, 3, 63)]

# ---- projection shapes (n_ref, cols): n_ref over the row list above, cols = n_new free
ALL_ROWS = [SMALLEST_N] + SHORT_ROWS + ROW_TAILS + sorted(WIDE)
PROJECT_COLS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1281]   # lane / wave / workgroup edges, each -1, 0, +1
PROJECT_NARROW, PROJECT_WIDE = (261, 65), (1289, 1281)
NUM_PCS = [1, 2, 3, 4, 7, 8, 9, 15]   # chunks: 1 | 2 | 2+1 | 4 | 4+2+1 | 8 | 8+1 | 8+4+2+1 (project_chunk)
MAX_PC = 15
I64_ROUNDED_PROJECT = [(257, 1), (261, 65), (1289, 1281)]
I64_REFERENCE_PROJECT = (261, 65)


def project_shapes():
    out = [(n, w) for n in ALL_ROWS for w in (1, 65)]
    out += [(n, w) for n in (261, 1289) for w in PROJECT_COLS if (n, w) not in out]
    return out


def num_pc_at(n_ref):
    """pcoa_project refuses num_pc > n_ref: the rows below 15 run with every component they have."""
    return min(MAX_PC, n_ref)


# ---- the twins -----------------------------------------------------------------------------------------------------------
def twin_strip_col_sums(s):
    """pcoa_strip_col_sums: exact int64 column sums, converted once."""
    return np.asarray(s, dtype=np.int64).sum(axis=0, dtype=np.int64).astype(np.float64)


def twin_strip_matvec(s, col0, v, means, mm, band=BAND, swap=False):
    """pcoa_strip_matvec on the strip s = S[:, col0:col0 + cols] ([n][cols] int64): y[j] = sum_i B(col0 + j, i) v[i] with
    B(j, i) = ((S(i, j) - means[j]) - means[i]) + mm.  band=None and swap=True are the WRONG orders the CPU test tells the
    twin apart from (one accumulator over all rows; the two subtractions traded)."""
    s = np.asarray(s, dtype=np.int64)
    n, cols = s.shape
    v = np.asarray(v, dtype=np.float64)
    means = np.asarray(means, dtype=np.float64)
    mm = np.float64(mm)
    mj = means[col0:col0 + cols]
    total = np.zeros(cols, dtype=np.float64)
    step = n if band is None else band
    for i0 in range(0, n, step):
        acc = np.zeros(cols, dtype=np.float64)
        for i in range(i0, min(n, i0 + step)):
            data = s[i].astype(np.float64)
            if swap:
                t = data - means[i]
                t = t - mj
            else:
                t = data - mj
                t = t - means[i]
            t = t + mm
            p = t * v[i]          # the product is rounded ...
            acc = acc + p         # ... before the addition is
        total = total + acc
    return total


def reference_centring(r):
    """What pcoa_project recomputes on the reference engine: mean[i] = (double)rs_i / n (col_means_kernel) and
    mm = (double)sum(rs) / n / n, two divisions in that order (stats_kernel), from the exact int64 row sums."""
    r = np.asarray(r, dtype=np.int64)
    n = np.float64(r.shape[0])
    rs = r.sum(axis=1, dtype=np.int64)
    return rs.astype(np.float64) / n, np.float64(int(rs.sum())) / n / n


def twin_col_means(x, n_ref):
    """m_q: the exact int64 column sum over rows [0, n_ref), one division."""
    x = np.asarray(x, dtype=np.int64)
    return x[:n_ref].sum(axis=0, dtype=np.int64).astype(np.float64) / np.float64(n_ref)


def twin_project(x, n_ref, mean, mm, u, lam, band=BAND, swap=False):
    """pcoa_project: x is the cross strip ([>= n_ref][cols] int64; rows >= n_ref are not read), mean / mm the reference's
    centring, u [k][n_ref], lam [k].  Returns [cols][k] (the layout of engine.project).  Every component is accumulated on
    its own, so the result of one does not depend on k."""
    x = np.asarray(x, dtype=np.int64)
    cols = x.shape[1]
    u = np.asarray(u, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    mean = np.asarray(mean, dtype=np.float64)
    mm = np.float64(mm)
    k = u.shape[0]
    mq = twin_col_means(x, n_ref)
    total = np.zeros((k, cols), dtype=np.float64)
    step = n_ref if band is None else band
    for i0 in range(0, n_ref, step):
        acc = np.zeros((k, cols), dtype=np.float64)
        for i in range(i0, min(n_ref, i0 + step)):
            data = x[i].astype(np.float64)
            if swap:
                t = data - mean[i]
                t = t - mq
            else:
                t = data - mq
                t = t - mean[i]
            t = t + mm
            p = t[None, :] * u[:, i, None]
            acc = acc + p
        total = total + acc
    return np.ascontiguousarray((total / lam[:, None]).T)


# ---- long-double evaluations and the bound of the CPU test -----------------------------------------------------------------
def longdouble_strip_matvec(s, col0, v, means, mm):
    """(sum_i t_i v_i, sum_i |t_i v_i|) per column with t and the sums in long double (the inputs are the same doubles)."""
    ld = np.longdouble
    s = np.asarray(s, dtype=np.int64)
    cols = s.shape[1]
    t = ((s.astype(ld) - np.asarray(means[col0:col0 + cols], dtype=ld)[None, :]) - np.asarray(means, dtype=ld)[:, None]) + ld(mm)
    p = t * np.asarray(v, dtype=ld)[:, None]
    return p.sum(axis=0), np.abs(p).sum(axis=0)


def longdouble_project(x, n_ref, mean, mm, u, lam):
    """The same for the projection, [cols][k]: m_q, mean and mm are the doubles the contract defines (their divisions are
    part of the spec, not of the error), everything after them in long double."""
    ld = np.longdouble
    x = np.asarray(x, dtype=np.int64)[:n_ref]
    t = ((x.astype(ld) - twin_col_means(x, n_ref).astype(ld)[None, :]) - np.asarray(mean, dtype=ld)[:, None]) + ld(mm)   # [n_ref][cols]
    ul = np.asarray(u, dtype=ld)
    val = np.stack([(t * ul[c][:, None]).sum(axis=0) for c in range(ul.shape[0])], axis=1)
    mag = np.stack([np.abs(t * ul[c][:, None]).sum(axis=0) for c in range(ul.shape[0])], axis=1)
    lam = np.asarray(lam, dtype=ld)
    return val / lam[None, :], mag / np.abs(lam)[None, :]


def rounding_bound(n, magnitude):
    """(n + 8) 2^-52 sum_i |t_i v_i|: n sequential additions (256 in a band, then the bands: fewer than n in all) plus the four
    roundings of a term (three of t, one of the product), and for the projection the division; unit roundoff is 2^-53, so
    the factor has a margin of two.  Derived, not measured."""
    return (n + 8) * np.longdouble(2.0) ** -52 * magnitude


# ---- cohorts ---------------------------------------------------------------------------------------------------------------
def _symmetric(rng, n, bound):
    a = rng.integers(0, bound, size=(n, n), dtype=np.int64)
    return np.triu(a) + np.triu(a, 1).T


@functools.lru_cache(maxsize=None)
def strip_matrix(n):
    """The symmetric N x N integer matrix (entries in [0, 2^20)) whose column slices are the strips of every shape with
    this n: strips cut from it share their columns, which is what the column-independence test needs."""
    s = _symmetric(np.random.default_rng(7000 + n), n, 2 ** 20)
    s.setflags(write=False)
    return s


def strip_of(n, col0, cols, big=False):
    s = np.ascontiguousarray(strip_matrix(n)[:, col0:col0 + cols])
    return s + HI if big else s


@functools.lru_cache(maxsize=None)
def exact_strip_inputs(n):
    """(v, means, mm): integers in [-8, 8], integer-valued doubles in [0, 2^20), 2^19."""
    rng = np.random.default_rng(8000 + n)
    v = rng.integers(-8, 9, size=n).astype(np.float64)
    means = rng.integers(0, 2 ** 20, size=n).astype(np.float64)
    return v, means, 2.0 ** 19


@functools.lru_cache(maxsize=None)
def rounded_strip_inputs(n):
    """(v, means, mm): standard normal, uniform in [100, 3000), a non-integer.  An entry near 2^19 minus a mean near 2^10
    rounds at 2^-34, and the second subtraction rounds again: the order of the two is visible in the last bits."""
    rng = np.random.default_rng(9000 + n)
    v = rng.standard_normal(n)
    means = rng.uniform(100.0, 3000.0, size=n)
    return v, means, 1571.0 + 1.0 / 3.0


def int_strip_matvec(s, col0, v, means, mm):
    """The exact cohort's product in int64 arithmetic."""
    s = np.asarray(s, dtype=np.int64)
    cols = s.shape[1]
    vi, mi, mmi = v.astype(np.int64), means.astype(np.int64), int(mm)
    assert np.array_equal(vi, v) and np.array_equal(mi, means) and mmi == mm
    t = s - mi[col0:col0 + cols][None, :] - mi[:, None] + mmi
    assert int(np.abs(t).max()) * 8 * s.shape[0] < 2 ** 53
    return (t * vi[:, None]).sum(axis=0, dtype=np.int64).astype(np.float64)


class ProjectCohort(object):
    """r: the reference matrix [n_ref][n_ref]; x: the cross block [n_ref][cols]; u [k][n_ref], lam [k], k = num_pc_at(n_ref).
    cross(big): the [n_ref + cols][cols] matrix a cross strip owner (n = n_ref + cols, strip (n_ref, cols)) is loaded with:
    x on top, rows >= n_ref filled with a value the projection must not read and the column sums must ignore."""

    def __init__(self, r, x, u, lam):
        self.r, self.x, self.u, self.lam = r, x, u, lam
        self.n_ref, self.cols = x.shape
        for a in (r, x, u, lam):
            a.setflags(write=False)

    def reference(self, big=False):
        return self.r + HI if big else self.r

    def cross(self, big=False):
        top = self.x + HI if big else self.x
        fill = np.full((self.cols, self.cols), POISON64 if big else POISON32, dtype=np.int64)
        return np.ascontiguousarray(np.concatenate([top, fill], axis=0))

    def comps(self, k=None):
        """[n_ref][k]: what engine.project takes."""
        return np.ascontiguousarray(self.u[:k].T)


@functools.lru_cache(maxsize=None)
def exact_project_cohort(n_ref, cols):
    """Integer means by construction: a symmetric draw below 2^20; (-rs_i) mod n_ref on the diagonal makes every row sum a
    multiple of n_ref, n_ref ((-sum rs_i / n_ref) mod n_ref) on entry (0, 0) the matrix sum a multiple of n_ref^2; in the
    cross block (-colsum_q) mod n_ref goes to row 0 of each column.  u: integers in [-8, 8]; lam: +- powers of two."""
    rng = np.random.default_rng(10000 * n_ref + cols)
    r = _symmetric(rng, n_ref, 2 ** 20)
    r[np.arange(n_ref), np.arange(n_ref)] += (-r.sum(axis=1)) % n_ref
    r[0, 0] += n_ref * ((-(int(r.sum()) // n_ref)) % n_ref)
    x = rng.integers(0, 2 ** 20, size=(n_ref, cols), dtype=np.int64)
    x[0] += (-x.sum(axis=0)) % n_ref
    k = num_pc_at(n_ref)
    u = rng.integers(-8, 9, size=(k, n_ref)).astype(np.float64)
    lam = np.array([(-1.0) ** c * 2.0 ** (c - 7) for c in range(k)])
    assert not (r.sum(axis=1) % n_ref).any() and int(r.sum()) % (n_ref * n_ref) == 0 and not (x.sum(axis=0) % n_ref).any()
    assert np.array_equal(r, r.T) and max(int(r.max()), int(x.max())) < 2 ** 31
    return ProjectCohort(r, x, u, lam)


@functools.lru_cache(maxsize=None)
def rounded_project_cohort(n_ref, cols):
    """No construction: a symmetric reference with entries in [0, 2^8) (row means near 2^7, full mantissas), a cross block with
    entries in [0, 2^20) (column means near 2^19), u standard normal, lam real with mixed signs.  The two means sit in
    different binades ON PURPOSE: x - m_q is then exact or nearly so and the next subtraction rounds once, while x - mean_i
    rounds at 2^-33 first -- the two orders of the subtractions give different doubles in a large share of the terms.  (With
    both means at the scale of x either order returns the correctly rounded t and a swapped kernel would pass.)"""
    rng = np.random.default_rng(20000 * n_ref + cols)
    r = _symmetric(rng, n_ref, 2 ** 8)
    x = rng.integers(0, 2 ** 20, size=(n_ref, cols), dtype=np.int64)
    k = num_pc_at(n_ref)
    u = rng.standard_normal((k, n_ref))
    lam = rng.uniform(0.5, 50.0, size=k) * np.where(np.arange(k) % 3 == 1, -1.0, 1.0)
    return ProjectCohort(r, x, u, lam)


def int_project(co):
    """The exact cohort's coordinates [cols][k]: int64 arithmetic, then the division by a power of two."""
    n = co.n_ref
    rs = co.r.sum(axis=1, dtype=np.int64)
    mean, mm, mq = rs // n, int(rs.sum()) // (n * n), co.x.sum(axis=0, dtype=np.int64) // n
    t = co.x - mq[None, :] - mean[:, None] + mm      # [n_ref][cols]
    ui = co.u.astype(np.int64)
    assert np.array_equal(ui, co.u) and int(np.abs(t).max()) * 8 * n < 2 ** 53
    return np.ascontiguousarray(((ui @ t).astype(np.float64) / co.lam[:, None]).T)

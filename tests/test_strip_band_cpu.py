"""The twins and cohorts of tests/strip_cohort.py held to their own promises: on the exact cohorts a twin IS the int64
arithmetic, on the rounded ones it stays inside the derived rounding bound of a long-double evaluation, and it has teeth --
the documented order (bands of 256 rows; (S - mean_col) - mean_row) gives other doubles than the two nearest wrong orders.
No GPU."""
import numpy as np
import pytest

import strip_cohort as C

STRIPS = [(1, 0, 1), (5, 4, 1), (33, 0, 33), (257, 0, 257), (261, 196, 65), (513, 3, 63), (1289, 8, 1281)]
PROJECTS = [(1, 1), (33, 1), (261, 65), (1289, 1281)]


def test_shape_lists_hold_what_they_are_tied_to():
    shapes = C.strip_shapes()
    ns = sorted(set(n for n, _, _ in shapes))
    assert [n - C.BAND for n in C.ROW_TAILS[:9]] == [1, 2, 3, 4, 5, 7, 8, 9, 12] and C.ROW_TAILS[9:] == [512, 513]
    assert set(ns) == set(C.ALL_ROWS) and C.SMALLEST_N == 1
    for n in C.ROW_TAILS:
        assert set((n, c0, w) for c0, w in [(0, n), (n - 65, 65), (5, 1), (3, 63), (1, 64)]) <= set(shapes)
    for s in [(1289, 0, 1289), (1289, 7, 1023), (1289, 7, 1024), (1289, 7, 1025), (1289, 8, 1281), (1289, 1000, 289),
              (1536, 0, 1536), (1536, 256, 1024)]:
        assert s in shapes
    assert set(C.I64_ROUNDED_STRIPS) <= set(shapes)
    # wherever a strip can start past column 0, some shape of that n does: means[col0 + j] is told from means[j]
    assert all(any(c0 > 0 for m, c0, _ in shapes if m == n) for n in ns if n > 1)
    ps = C.project_shapes()
    assert len(ps) == len(set(ps))
    assert set((n, w) for n in C.ALL_ROWS for w in (1, 65)) <= set(ps)
    assert set((n, w) for n in (261, 1289) for w in C.PROJECT_COLS) <= set(ps)
    assert set(C.I64_ROUNDED_PROJECT + [C.I64_REFERENCE_PROJECT, C.PROJECT_NARROW, C.PROJECT_WIDE]) <= set(ps)
    assert [C.num_pc_at(n) for n in (1, 4, 5, 33)] == [1, 4, 5, 15]


@pytest.mark.parametrize("n,col0,cols", STRIPS)
@pytest.mark.parametrize("big", [False, True])
def test_strip_twins_are_the_int64_arithmetic_on_exact_cohorts(n, col0, cols, big):
    s = C.strip_of(n, col0, cols, big)
    assert s.shape == (n, cols) and (s.min() >= 2 ** 31 if big else s.max() < 2 ** 20)
    assert np.array_equal(C.strip_matrix(n), C.strip_matrix(n).T)
    v, means, mm = C.exact_strip_inputs(n)
    want = C.int_strip_matvec(s, col0, v, means, mm)
    assert np.array_equal(C.twin_strip_matvec(s, col0, v, means, mm), want)
    # any order: that is what makes the cohort exact
    assert np.array_equal(C.twin_strip_matvec(s, col0, v, means, mm, band=None, swap=True), want)
    cs = C.twin_strip_col_sums(s)
    assert cs.dtype == np.float64 and [int(c) for c in cs[:5]] == [sum(int(a) for a in s[:, j]) for j in range(min(cols, 5))]
    assert n < 33 or len(set(want.tolist())) > min(cols, 8) // 2


@pytest.mark.parametrize("n_ref,cols", PROJECTS)
def test_projection_twin_is_the_int64_arithmetic_on_exact_cohorts(n_ref, cols):
    co = C.exact_project_cohort(n_ref, cols)
    mean, mm = C.reference_centring(co.r)
    assert np.array_equal(mean, np.rint(mean)) and mm == np.rint(mm)
    assert np.array_equal(C.twin_col_means(co.x, n_ref), np.rint(C.twin_col_means(co.x, n_ref)))
    want = C.int_project(co)
    assert want.shape == (cols, C.num_pc_at(n_ref))
    assert np.array_equal(C.twin_project(co.x, n_ref, mean, mm, co.u, co.lam), want)
    assert np.array_equal(C.twin_project(co.x, n_ref, mean, mm, co.u, co.lam, band=None, swap=True), want)
    # the int64 part cancels exactly, in the cross strip (whose rows >= n_ref are never read) and in the reference
    for big in (False, True):
        x = co.cross(big)
        assert x.shape == (n_ref + cols, cols) and int(x[n_ref:].min()) == (C.POISON64 if big else C.POISON32)
        assert (x.max() < 2 ** 31) != big
        assert np.array_equal(C.twin_project(x, n_ref, mean, mm, co.u, co.lam), want)
    mean_b, mm_b = C.reference_centring(co.reference(True))
    assert np.array_equal(C.twin_project(co.x, n_ref, mean_b, mm_b, co.u, co.lam), want)
    assert len(set(np.sign(co.lam).tolist())) == min(2, co.lam.size)


@pytest.mark.parametrize("n,col0,cols", STRIPS)
def test_strip_twin_stays_inside_the_rounding_bound_of_a_long_double_sum(n, col0, cols):
    s = C.strip_of(n, col0, cols)
    v, means, mm = C.rounded_strip_inputs(n)
    assert means.min() >= 100.0 and means.max() < 3000.0 and mm != np.rint(mm)
    val, mag = C.longdouble_strip_matvec(s, col0, v, means, mm)
    got = C.twin_strip_matvec(s, col0, v, means, mm)
    assert np.all(np.abs(got.astype(np.longdouble) - val) <= C.rounding_bound(n, mag))


@pytest.mark.parametrize("n_ref,cols", PROJECTS)
def test_projection_twin_stays_inside_the_rounding_bound_of_a_long_double_sum(n_ref, cols):
    co = C.rounded_project_cohort(n_ref, cols)
    mean, mm = C.reference_centring(co.r)
    val, mag = C.longdouble_project(co.x, n_ref, mean, mm, co.u, co.lam)
    got = C.twin_project(co.x, n_ref, mean, mm, co.u, co.lam)
    assert got.shape == val.shape
    assert np.all(np.abs(got.astype(np.longdouble) - val) <= C.rounding_bound(n_ref, mag))
    assert n_ref < 3 or len(set(np.sign(co.lam).tolist())) == 2


@pytest.mark.parametrize("n", [261, 777])
def test_the_documented_order_is_visible_in_the_doubles(n):
    """Teeth: the same terms added left to right without bands, and the twin with the two subtractions traded, are other
    doubles in at least one entry (in fact in most) -- a kernel with either order fails the bit-for-bit comparison."""
    s = C.strip_of(n, 0, n)
    v, means, mm = C.rounded_strip_inputs(n)
    twin = C.twin_strip_matvec(s, 0, v, means, mm)
    unbanded = C.twin_strip_matvec(s, 0, v, means, mm, band=None)
    swapped = C.twin_strip_matvec(s, 0, v, means, mm, swap=True)
    assert np.any(twin != unbanded) and np.any(twin != swapped)
    co = C.rounded_project_cohort(n, 65)
    mean, cm = C.reference_centring(co.r)
    twin = C.twin_project(co.x, n, mean, cm, co.u, co.lam)
    assert np.any(twin != C.twin_project(co.x, n, mean, cm, co.u, co.lam, band=None))
    assert np.any(twin != C.twin_project(co.x, n, mean, cm, co.u, co.lam, swap=True))
    # and a BLAS product of the same centred matrix is yet another rounding
    b = ((s.astype(np.float64) - means[None, :]) - means[:, None]) + mm
    assert np.any(C.twin_strip_matvec(s, 0, v, means, mm) != b.T @ v)

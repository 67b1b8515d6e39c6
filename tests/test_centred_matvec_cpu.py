"""The exact reference of the centred mat-vec tests (eig_spectra.integer_centred, tests/test_gpu_centred_matvec_forms.py) held
to its own promises and to the oracle's centring, at the shapes the GPU tests use.  No GPU."""
import numpy as np
import pytest

import eig_spectra as E
import test_gpu_centred_matvec_forms as M
from conftest import load_oracle

SHAPES = M.exact_shapes()


@pytest.fixture(scope="module")
def O():
    return load_oracle()


def _seed(n, scale, zero_row):
    return M.SEEDS.get((n, scale, zero_row), n)


@pytest.mark.parametrize("n,scale,zero_row", [(1, 1, None), (5, 1, 3), (36, 1, None), (36, 7, 3), (260, 2 ** 22, 3), (1044, 1, 3)])
def test_builder_gives_divisible_sums_and_a_symmetric_integer_b(n, scale, zero_row):
    s, b = E.integer_centred(n, _seed(n, scale, zero_row), scale=scale, zero_row=zero_row)
    assert s.dtype == np.int64 and b.dtype == np.int64 and s.shape == (n, n)
    assert np.array_equal(s, s.T) and np.array_equal(b, b.T)
    r = s.sum(axis=1)
    assert not (r % n).any() and int(r.sum()) % (n * n) == 0
    assert not (s % scale).any() and s.min() >= 0
    if zero_row is not None:
        assert not s[zero_row].any() and not s[:, zero_row].any() and int((r > 0).sum()) == n - 1
    # B = J S J exactly: rows and columns sum to zero, and B differs from S by rank-one terms of the means
    assert not b.sum(axis=0).any() and not b.sum(axis=1).any()
    assert np.array_equal(b, s - (r // n)[:, None] - (r // n)[None, :] + int(r.sum()) // (n * n))
    if scale == 2 ** 22:
        assert np.abs(s).max() >= 2 ** 31
    # another seed is another matrix; the vectors are integers in range and not constant
    assert n == 1 or not np.array_equal(s, E.integer_centred(n, _seed(n, scale, zero_row) + 1000, scale=scale, zero_row=zero_row)[0])
    xs = E.integer_vectors(n, 17)
    assert xs.shape == (3, n) and np.array_equal(xs, np.rint(xs)) and np.abs(xs).max() <= E.INT_X_MAX
    assert n < 8 or all(len(set(x.tolist())) > 8 for x in xs)


def test_every_shape_of_the_gpu_tests_keeps_partial_sums_below_2_53():
    """n max|B| max|x| < 2^53 (asserted by the builder), so a float64 product in any order of addition is the integer one;
    where S is meant to fit int32 it does."""
    assert len(SHAPES) == len(set(SHAPES))
    for n, scale, zero_row in SHAPES:
        s, b = E.integer_centred(n, _seed(n, scale, zero_row), scale=scale, zero_row=zero_row)
        assert n * int(np.abs(b).max()) * E.INT_X_MAX < 2 ** 53, (n, scale)
        assert (np.abs(s).max() < 2 ** 31) == (scale == 1), (n, scale)


@pytest.mark.parametrize("n,scale,zero_row", [t for t in SHAPES if t[0] <= 1300], ids=lambda v: str(v))
def test_oracle_centring_returns_the_integer_b(O, n, scale, zero_row):
    s, b, bf, xs, ref = M.exact_case(n, scale, zero_row)
    got, rs, nz, mm = O.center_matrix(s)
    assert np.array_equal(got, bf)
    assert np.array_equal(rs, s.sum(axis=1).astype(np.float64)) and mm == float(int(s.sum()) // (n * n))
    assert nz == (n if zero_row is None else n - 1)
    # the float64 reference product is the int64 one, on every row
    assert np.array_equal(b @ xs.T.astype(np.int64), ref.astype(np.int64))

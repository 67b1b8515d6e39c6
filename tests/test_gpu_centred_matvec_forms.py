"""Every form of the eigensolver's centred mat-vec y = B x (csrc/eig_lanczos.hip) held to exact references, at the sample
counts where its loops change path ("Forms of the Lanczos path").

    form 0  symv_centered_kernel<false / true>   one wave per row over S, centred on the fly (row_dot)
    form 1  symv_sym_tiles_kernel                upper-triangular 1024 x 1024 tiles; row sums from rowsums_sym_tiles_kernel
    form 2  symv_kernel                          one wave per row over the materialised B (row_dot)

EXACT cases: S = eig_spectra.integer_centred, whose centred matrix is an integer matrix.  For an integer x every partial sum
of B x is an integer below 2^53, so every form, in every order of addition, must return the int64 product bit for bit
(np.array_equal): a dropped, doubled or misplaced entry cannot hide behind a tolerance.  The reference is a float64 matmul
(exact for the same reason), itself held to an int64 product on the last 64 rows; B 1 = 0 is checked as well.  The sample
counts, by what they reach:

  upper-triangle form, N mod 1024 (a wave walks every second row of a tile, four row buffers deep):
    4, 8, 64, 1020           the corner tile alone (nbi = 0)
    1024, 2048               no ragged tile; an interior tile at 2048
    1028 .. 1060             a ragged tile of 4 .. 36 rows: 2, 4, 6, 8, 10, 14, 18 rows per wave -- below, at and above the
                             eight rows of the steady-state loop, with 1, 2 and 3 (mod 4) rows left for the refill / drain tail
    1280 .. 2044             the valid columns of the ragged tile end at, one quad before and one quad behind the boundary of
                             a lane's column groups (256 / 512 / 768): the `jw + 256 q < n` mask
    2052                     interior tile + ragged block column + corner
    3076                     the interior-tile index loop with bi > 0
  row forms (row_dot): N % 4 != 0 takes 4-byte loads (main loop j + 448 < n), N % 4 == 0 16-byte loads (main loop
    j + 768 < n: lanes leave it at different N between 772 and 1024)
  int64 part live (symv_centered_kernel<true>, center_kernel / row_sums_kernel with s64): scale = 2^22 takes S out of int32;
    PCOA_NO_NARROW=1 (a child process: the knob is read once) holds the int64 kernels to the same S as the int32 ones.

ROUNDED cases: genotype counts (binary X, 700 variants), whose means are not integers, so the order of the centring
operations matters.  A unit vector must return the oracle's column of B bit for bit in every form, at columns on both sides
of every tile, half-tile and quad-group edge; for Gaussian x every form stays within
    |y_i - ref_i| <= N 2^-52 (|B| |x|)_i        (ref: the oracle's B times x in long double)
which holds for EVERY order of addition: N - 1 additions and one product rounding per term at unit roundoff 2^-53 give
(N 2^-53) (|B| |x|)_i to first order; doubled.  A single dropped term is about 1e9 times larger.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import eig_spectra as E  # noqa: E402
from conftest import load_oracle, load_pkg  # noqa: E402

pytestmark = pytest.mark.gpu

PCOA_ERR_STATE = -8
SYT = 1024                    # tile of the upper-triangle form

UPPER_N = (4, 8, 64, 1020,
           1024, 2048,
           1028, 1032, 1036, 1040, 1044, 1052, 1060,
           1280, 1284, 1532, 1536, 1540, 1792, 2044,
           2052,
           3076)
ROW_SCALAR_N = (1, 2, 3, 5, 63, 65, 449, 511, 513, 961, 1023, 1025)
ROW_QUAD_N = (252, 256, 260, 768, 772, 1020, 1024, 1028, 1792, 1796)
I64_SCALE = 2 ** 22
I64_N = (5, 65, 513, 772, 1028)
NO_NARROW_N = (63, 260, 1025, 1796)
CENTER_N = (5, 260, 1025)
CENTER_ZERO_ROW = 3
CENTER_AFTER_UPPER_N = 1044
ROUNDED_N = (260, 1025, 1044, 1540, 2052)
ROUNDED_V = 700
NO_NARROW_LIMIT = 30          # seconds: about 10x the 2.5 s the child takes on an idle MI355X, start-up included

# integer_centred raises S[0, 0] by up to n (n - 1), and with it max |B|; times 2^22 the bound n max|B| max|x| < 2^53 of the
# builder holds only where the draw leaves that raise small.  The seeds below are the first for which it does (the builder
# asserts it; tests/test_centred_matvec_cpu.py runs it at every shape).  Everywhere else the seed is n.
SEEDS = {(772, I64_SCALE, None): 0, (1025, I64_SCALE, CENTER_ZERO_ROW): 1}


def exact_shapes():
    """(n, scale, zero_row) of every exact case of this module."""
    out = [(n, 1, None) for n in sorted(set(UPPER_N + ROW_SCALAR_N + ROW_QUAD_N + NO_NARROW_N))]
    out += [(n, I64_SCALE, None) for n in I64_N]
    out += [(n, scale, CENTER_ZERO_ROW) for n in CENTER_N for scale in (1, I64_SCALE)]
    out.append((CENTER_AFTER_UPPER_N, 1, CENTER_ZERO_ROW))
    return out


def exact_case(n, scale=1, zero_row=None):
    """(S, B int64, B float64, x [3, n], B x [n, 3]) of one exact case."""
    s, b = E.integer_centred(n, SEEDS.get((n, scale, zero_row), n), scale=scale, zero_row=zero_row)
    bf = b.astype(np.float64)
    xs = E.integer_vectors(n, 17)
    ref = bf @ xs.T
    r0 = max(0, n - 64)       # the float64 reference itself against int64 on the last (ragged) 64 rows
    assert np.array_equal(b[r0:] @ xs.T.astype(np.int64), ref[r0:].astype(np.int64)) and np.array_equal(ref, np.rint(ref))
    assert not b.sum(axis=1).any()
    return s, b, bf, xs, ref


def _mismatch(n, form, what, got, want):
    bad = np.nonzero(got != want)[0]
    i = int(bad[0])
    return "N = %d, form %d, %s: %d of %d entries differ; first y[%d] = %r, want %r (tile row %d, row %d of it; rows %s ..)" % (
        n, form, what, bad.size, n, i, float(got[i]), float(want[i]), i // SYT, i % SYT, bad[:8].tolist())


def _check_forms(eng, n, forms, xs, ref):
    for form in forms:
        for v in range(xs.shape[0]):
            y = eng.debug_centred_matvec(xs[v], form)
            assert np.array_equal(y, ref[:, v]), _mismatch(n, form, "integer x %d" % v, y, ref[:, v])
        y = eng.debug_centred_matvec(np.ones(n), form)
        assert not y.any(), _mismatch(n, form, "B 1", y, np.zeros(n))


def _refuses_upper_triangle_form(P, eng, n):
    with pytest.raises(P.PcoaError) as err:
        eng.debug_centred_matvec(np.ones(n), 1)
    assert err.value.code == PCOA_ERR_STATE, err.value


def _check_center(eng, n, s, b, bf):
    got_b, rs, nz, mm = eng.center()
    r = s.sum(axis=1)
    assert np.array_equal(got_b, bf), "N = %d: center() differs from the integer B in %d entries" % (n, int((got_b != bf).sum()))
    assert np.array_equal(rs, r.astype(np.float64)) and mm == float(int(r.sum()) // (n * n))
    assert nz == n - 1


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def O():
    return load_oracle()


# ------------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("n", UPPER_N)
def test_upper_triangle_form_returns_the_integer_product(P, n):
    """Form 1 at every tile kind and tail of the row-buffer loop; forms 0 and 2 give the same integers."""
    s, b, bf, xs, ref = exact_case(n)
    with P.PcoaEngine(n) as eng:
        eng.load_gram(s)
        assert eng.timings()["gram_i64_live"] == 0
        _check_forms(eng, n, (1, 0, 2), xs, ref)


# (1020, 1024, 1028 and 1792 of the 16-byte list run all three forms above)
@pytest.mark.parametrize("n", [n for n in ROW_SCALAR_N + ROW_QUAD_N if n not in UPPER_N])
def test_row_forms_return_the_integer_product(P, n):
    """Forms 0 and 2 (row_dot over S centred on the fly and over the materialised B): 4-byte loads at N % 4 != 0, 16-byte
    loads else, around the ends of their main loops."""
    s, b, bf, xs, ref = exact_case(n)
    with P.PcoaEngine(n) as eng:
        eng.load_gram(s)
        assert eng.timings()["gram_i64_live"] == 0
        _check_forms(eng, n, (0, 2), xs, ref)
        if n % 4:
            _refuses_upper_triangle_form(P, eng, n)


@pytest.mark.parametrize("n", I64_N)
def test_row_forms_with_the_int64_part_live(P, n):
    """S times 2^22 leaves int32: symv_centered_kernel<true> and the s64 branches of the centring; form 1 refuses."""
    s, b, bf, xs, ref = exact_case(n, I64_SCALE)
    assert np.abs(s).max() >= 2 ** 31
    with P.PcoaEngine(n) as eng:
        eng.load_gram(s)
        assert eng.timings()["gram_i64_live"] == 1
        _refuses_upper_triangle_form(P, eng, n)
        _check_forms(eng, n, (0, 2), xs, ref)


@pytest.mark.parametrize("scale", [1, I64_SCALE], ids=["int32", "int64"])
@pytest.mark.parametrize("n", CENTER_N)
def test_center_returns_the_integer_b(P, n, scale):
    """pcoa_center_read_f64 on an S with one all-zero sample: B, row sums and matrix mean exact, nonzero_rows = N - 1."""
    s, b, bf, xs, ref = exact_case(n, scale, CENTER_ZERO_ROW)
    with P.PcoaEngine(n) as eng:
        eng.load_gram(s)
        assert eng.timings()["gram_i64_live"] == (0 if scale == 1 else 1)
        _check_center(eng, n, s, b, bf)
        _check_forms(eng, n, (0, 2), xs, ref)
        _check_center(eng, n, s, b, bf)


def test_center_after_an_upper_triangle_call(P):
    """The form-1 hook fills the row sums from rowsums_sym_tiles_kernel; center() afterwards returns the same exact B."""
    n = CENTER_AFTER_UPPER_N
    s, b, bf, xs, ref = exact_case(n, 1, CENTER_ZERO_ROW)
    with P.PcoaEngine(n) as eng:
        eng.load_gram(s)
        _check_forms(eng, n, (1,), xs, ref)
        _check_center(eng, n, s, b, bf)
        _check_forms(eng, n, (1, 0, 2), xs, ref)


# ---------------------------------------------------------------------------------- PCOA_NO_NARROW=1: one child process
def child_main(argv):
    """Every N of argv[0] in turn with the knob of the parent's environment: one JSON line per N."""
    P = load_pkg()
    for n in [int(a) for a in argv[0].split(",")]:
        s, b, bf, xs, ref = exact_case(n)
        out = {"n": n, "int32_range": bool(np.abs(s).max() < 2 ** 31)}
        with P.PcoaEngine(n) as eng:
            eng.load_gram(s)
            out["gram_i64_live"] = int(eng.timings()["gram_i64_live"])
            try:
                eng.debug_centred_matvec(np.ones(n), 1)
                out["form1"] = 0
            except P.PcoaError as exc:
                out["form1"] = exc.code
            bad = []
            for form in (0, 2):
                for v in range(xs.shape[0]):
                    y = eng.debug_centred_matvec(xs[v], form)
                    if not np.array_equal(y, ref[:, v]):
                        bad.append(_mismatch(n, form, "integer x %d" % v, y, ref[:, v]))
                y = eng.debug_centred_matvec(np.ones(n), form)
                if y.any():
                    bad.append(_mismatch(n, form, "B 1", y, np.zeros(n)))
            got_b, rs, nz, mm = eng.center()
            if not (np.array_equal(got_b, bf) and np.array_equal(rs, s.sum(axis=1).astype(np.float64))):
                bad.append("N = %d: center() differs from the integer B" % n)
            out["bad"] = bad
        print(json.dumps(out))
        sys.stdout.flush()


_RUN = {}


def _no_narrow_run():
    """The child, once per session, never retried."""
    if _RUN:
        return _RUN
    env = dict(os.environ, PCOA_NO_NARROW="1")
    cmd = [sys.executable, os.path.abspath(__file__), ",".join(str(n) for n in NO_NARROW_N)]
    try:
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env,
                             timeout=NO_NARROW_LIMIT)
    except subprocess.TimeoutExpired as e:
        _RUN["error"] = "child exceeded its time limit of %d s; stdout so far:\n%s" % (NO_NARROW_LIMIT, e.stdout)
        return _RUN
    lines = [json.loads(t) for t in res.stdout.splitlines() if t.startswith("{")]
    _RUN["cases"] = dict((d["n"], d) for d in lines)
    if res.returncode != 0:
        _RUN["error"] = "child exited with status %d\n%s" % (res.returncode, res.stderr[-4000:])
    return _RUN


@pytest.mark.parametrize("n", NO_NARROW_N)
def test_int64_kernels_on_an_s_that_fits_int32(n):
    """PCOA_NO_NARROW=1: the S of the int32 cases stays int64, and the int64 kernels return the same integers."""
    run = _no_narrow_run()
    assert "error" not in run, run["error"]
    assert n in run["cases"], "no result for N = %d" % n
    r = run["cases"][n]
    assert r["int32_range"] and r["gram_i64_live"] == 1, r
    assert r["form1"] == PCOA_ERR_STATE, r
    assert not r["bad"], "\n".join(r["bad"])


# ------------------------------------------------------------------------------------------------------- rounded cases
@pytest.mark.parametrize("n", ROUNDED_N)
def test_genotype_counts_every_form_against_the_oracle_b(P, O, n):
    rng = np.random.default_rng(n)
    x8 = (rng.random((ROUNDED_V, n)) < rng.uniform(0.02, 0.4, size=(ROUNDED_V, 1))).astype(np.uint8)
    forms = (0, 1, 2) if n % 4 == 0 else (0, 2)
    with P.PcoaEngine(n) as eng:
        eng.accumulate_dense_u8(x8)
        b = O.center_matrix(eng.gram())[0]
        for k in sorted(set(k for k in (0, 255, 256, 511, 512, 1023, 1024, 1027, n - 4, n - 1) if 0 <= k < n)):
            e = np.zeros(n)
            e[k] = 1.0
            for form in forms:
                y = eng.debug_centred_matvec(e, form)
                assert np.array_equal(y, b[:, k]), _mismatch(n, form, "column %d of B" % k, y, b[:, k])
        bl = b.astype(np.longdouble)
        ab = np.abs(b)
        for seed in range(3):
            xv = np.random.default_rng(seed).standard_normal(n)
            ref = bl @ xv.astype(np.longdouble)
            bound = n * 2.0 ** -52 * (ab @ np.abs(xv))
            for form in forms:
                y = eng.debug_centred_matvec(xv, form)
                err = np.abs((y.astype(np.longdouble) - ref).astype(np.float64))
                worst = int(np.argmax(err / bound))
                print("N = %d, form %d, x %d: max |y - ref| / bound = %.3g (row %d)" % (n, form, seed, err[worst] / bound[worst], worst))
                assert np.all(err <= bound), "N = %d, form %d, x %d: |y - ref| = %.3g > %.3g at row %d" % (
                    n, form, seed, err[worst], bound[worst], worst)


if __name__ == "__main__":
    child_main(sys.argv[1:])

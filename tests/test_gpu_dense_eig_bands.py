"""The dense fp64 eigensolver (csrc/eig.hip) held to exact spectra at every launch band, `eig="householder"`.

The host launchers pick a kernel form by the sample count ("Launch bands of the dense solver"):

    tridiag_hw_kernel alone                         N = 1
    two-kernel reduction (hw + update)              2 <= N <= 7, N >= 6,785
    fused step, one launch per column               8 <= N <= 6,784   (24 N bytes of LDS <= 162,816)
      with more than 64 KiB of dynamic LDS          N >= 2,731
      grid capped at 256 workgroups                 N >= 2,050
    bisection from LDS                              N <= 4,080
    inverse iteration from LDS                      N <= 3,490        (more than 64 KiB from N = 1,490)
      one workgroup per vector                      from LDS, k > 1, no two selected lambda within 1e-2 max|lambda|
    blocked compact-WY back-transform               N - 2 >= 128
    `auto` takes the dense solver                   N < 32

Every case loads an integer S with a known spectrum (tests/eig_spectra.py) through pcoa_gram_load_i64 and checks: the
method and `eig_dense_form` against the bits the bands name (a moved threshold fails with the band's name), eigenvalues,
host residuals, orthogonality, vectors or cluster subspaces against the reference (eig_spectra.check_pairs), the sign rule,
and a second compute on the same engine bit-identical to the first.  One JSON line per case reports the observed maxima.
"""
import json
import time

import numpy as np
import pytest

import eig_spectra as E
from conftest import load_oracle, load_pkg

pytestmark = pytest.mark.gpu

FUSED, FUSED_BIG_LDS, TWO_KERNEL, BISECT_LDS, INVIT_LDS, PER_VECTOR, WY = 1, 2, 4, 8, 16, 32, 64


def bands(n, lam):
    """(band, bit, taken) for every form bit of pcoa_timings.eig_dense_form at N = n with the selected eigenvalues lam."""
    big = np.abs(lam).max() if len(lam) else 0.0
    separated = len(lam) > 1 and all(abs(lam[i] - lam[j]) > 1e-2 * big for i in range(len(lam)) for j in range(i))
    return [
        ("fused Householder step (8 <= N <= 6,784)", FUSED, 8 <= n <= 6784),
        ("fused step with more than 64 KiB of LDS (2,731 <= N <= 6,784)", FUSED_BIG_LDS, 2731 <= n <= 6784),
        ("two-kernel reduction (2 <= N <= 7, N >= 6,785)", TWO_KERNEL, 2 <= n <= 7 or n >= 6785),
        ("bisection from LDS (N <= 4,080)", BISECT_LDS, n <= 4080),
        ("inverse iteration from LDS (N <= 3,490)", INVIT_LDS, n <= 3490),
        ("inverse iteration, one workgroup per vector (LDS, k > 1, separated)", PER_VECTOR, n <= 3490 and separated),
        ("blocked compact-WY back-transform (N >= 130)", WY, n >= 130),
    ]


def check_form(t, n, lam):
    assert t["eig_method"] == 2, t
    got = t["eig_dense_form"]
    wrong = ["%s: expected %s" % (name, "taken" if on else "not taken") for name, bit, on in bands(n, lam)
             if bool(got & bit) != on]
    assert not wrong and got < 128, "N = %d, eig_dense_form = %d: %s" % (n, got, "; ".join(wrong))


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def O():
    return load_oracle()


def _bmul(O, sp):
    """U -> B U on the host: the oracle's B up to N = 4,100, the centred mat-vec over S beyond."""
    if sp.n <= 4100:
        b = getattr(sp, "b", None)
        if b is None:
            b = O.center_matrix(sp.s)[0]
        return lambda u: b @ u
    return E.centred_matmul_host(sp.s.astype(np.float64))


def _report(case, sp, t, obs, wall):
    rec = {"case": case, "n": sp.n, "k": sp.k, "family": sp.family, "form": t["eig_dense_form"],
           "gpu_ms": round(1e3 * t["compute_total_seconds"], 2), "host_s": round(wall, 2)}
    rec.update(dict((key, float("%.3g" % v)) for key, v in obs.items()))
    print("DENSE_EIG " + json.dumps(rec))


def run(P, O, case, sp, eig="householder"):
    """Two computes on one engine: the pairs, bit-identical the second time, checked against the reference."""
    t0 = time.time()
    with P.PcoaEngine(sp.n, eig=eig) as eng:
        eng.load_gram(sp.s)
        comps, lam, nz = eng.compute(sp.k)
        t = eng.timings()
        comps2, lam2, _ = eng.compute(sp.k)
    assert np.array_equal(comps, comps2) and np.array_equal(lam, lam2), "%s: second compute differs" % case
    if eig == "householder":
        check_form(t, sp.n, lam)
    obs = E.check_pairs(sp, comps, lam, _bmul(O, sp), case)
    _report(case, sp, t, obs, time.time() - t0)
    return comps, lam, t


# case id -> builder.  Edge pairs of the table above, the full decomposition at N = 1 .. 9 and 31, the limit of the `auto`
# fallback, and on each side of 3,490 the families whose clusters decide the inverse-iteration form.
CASES = {}
for _n in range(1, 10):
    CASES["full-%d" % _n] = (lambda n: lambda: E.planted(n, n))(_n)
CASES["full-31"] = lambda: E.planted(31, 31)
for _n in (129, 130, 131, 258, 1489, 1490, 2049, 2050, 2730, 2731, 3490, 3491, 4080, 4081):
    CASES["planted-%d" % _n] = (lambda n: lambda: E.planted(n, 2))(_n)
for _n, _m in ((3490, 2), (3491, 3)):
    CASES["multiplicity%d-%d" % (_m, _n)] = (lambda n, m: lambda: E.multiplicity(n, 4, m))(_n, _m)
for _n in (3490, 3491):
    CASES["near-tie-%d" % _n] = (lambda n: lambda: E.near_tie(n, 2))(_n)
    CASES["rank-deficient-%d" % _n] = (lambda n: lambda: E.shifted_low_rank(n, 5, v=3, c=0))(_n)
CASES["low-rank-16pcs-6784"] = lambda: E.shifted_low_rank(6784, 16, v=24)
CASES["noisy-6785"] = lambda: E.shifted_low_rank(6785, 2, v=8, noise=True)
CASES["int64-1490"] = lambda: E.shifted_low_rank(1490, 2, scale=2 ** 24)
CASES["noisy-16384"] = lambda: E.shifted_low_rank(16384, 2, v=8, noise=True)


@pytest.mark.parametrize("case", list(CASES))
def test_dense_solver_band(P, O, case):
    sp = CASES[case]()
    _, _, t = run(P, O, case, sp)
    if case.startswith("int64"):
        assert t["gram_i64_live"] == 1


@pytest.mark.parametrize("n", [3490, 3491])
def test_negative_dominant_spectrum_ranks_by_magnitude_like_auto(P, O, n):
    """S = c I - X^T X: the eigenvalues of largest |lambda| are negative.  Both solvers return them signed, ranked by
    |lambda| (MLlib's order), and agree."""
    sp = E.negative_dominant(n, 2)
    _, lam, _ = run(P, O, "negative-dominant-%d" % n, sp)
    _, lam_auto, t = run(P, O, "negative-dominant-auto-%d" % n, sp, eig="auto")
    assert np.all(lam < 0) and np.all(np.diff(np.abs(lam)) <= 0)
    assert np.all(np.abs(lam_auto - lam) <= 2 * E.EIG_BAR * sp.norm)
    assert (t["eig_dense_form"] == 0) == (t["eig_method"] == 1)


def test_separated_and_clustered_spectra_take_both_inverse_iteration_forms(P, O):
    """At one N from LDS: separated eigenvalues get one workgroup per vector, a cluster the sequential form."""
    n = 3490
    forms = {}
    for name, sp in (("separated", E.planted(n, 4)), ("clustered", E.multiplicity(n, 4, 3))):
        _, _, t = run(P, O, "invit-%s-%d" % (name, n), sp)
        forms[name] = t["eig_dense_form"]
    assert forms["separated"] & PER_VECTOR and not forms["clustered"] & PER_VECTOR, forms


@pytest.mark.parametrize("n", [31, 32])
def test_auto_takes_the_dense_solver_below_32_samples(P, O, n):
    sp = E.planted(n, 2)
    _, lam, t = run(P, O, "auto-%d" % n, sp, eig="auto")
    if n < 32:
        check_form(t, n, lam)
    else:
        assert t["eig_method"] == 1 and t["eig_dense_form"] == 0, t


def test_workspace_regrowth_matches_single_runs(P, O):
    """compute(2), compute(16), compute(3) on one engine (the eigenvector workspaces grow, then are reused): each within the
    bars, and equal to a fresh engine's compute(3) bit for bit."""
    n = 4081
    sp16 = E.shifted_low_rank(n, 16, v=24)
    bmul = _bmul(O, sp16)
    with P.PcoaEngine(n, eig="householder") as eng:
        eng.load_gram(sp16.s)
        out = {}
        for k in (2, 16, 3):
            comps, lam, _ = eng.compute(k)
            t = eng.timings()
            check_form(t, n, lam)
            sp = sp16.top(k)
            _report("regrowth-%d-k%d" % (n, k), sp, t, E.check_pairs(sp, comps, lam, bmul, "k = %d" % k), 0.0)
            out[k] = (comps, lam)
    with P.PcoaEngine(n, eig="householder") as eng:
        eng.load_gram(sp16.s)
        comps, lam, _ = eng.compute(3)
    assert np.array_equal(comps, out[3][0]) and np.array_equal(lam, out[3][1])

"""The reference of the dense-eigensolver band tests (tests/eig_spectra.py) held to float64 LAPACK on the oracle's B at small
N: every family's eigenvalues, predicted multiplicities, vectors and cluster subspaces, the Weyl estimate of the perturbed
family, and the checker itself on LAPACK's own answer.  No GPU."""
import numpy as np
import pytest

import eig_spectra as E
from conftest import load_oracle


@pytest.fixture(scope="module")
def O():
    return load_oracle()


def _lapack(O, sp):
    b = O.center_matrix(sp.s)[0]
    w, u = np.linalg.eigh(b)
    order = sorted(range(len(w)), key=lambda i: (-abs(w[i]), -w[i]))[:sp.k]
    u = u[:, order]
    u = u * np.where(u.max(axis=0) >= -u.min(axis=0), 1.0, -1.0)     # the sign rule pcoa_compute applies
    return b, w, u, w[order]


FAMILIES = [
    ("planted", lambda: E.planted(257, 4)),
    ("planted full", lambda: E.planted(9, 9)),
    ("shifted low rank", lambda: E.shifted_low_rank(300, 4, v=8)),
    ("shifted low rank, 16 pcs", lambda: E.shifted_low_rank(700, 16, v=24)),
    ("rank deficient", lambda: E.shifted_low_rank(211, 6, v=3, c=0)),
    ("noisy", lambda: E.shifted_low_rank(600, 2, v=8, noise=True)),
    ("multiplicity 2", lambda: E.multiplicity(300, 4, 2)),
    ("multiplicity 3", lambda: E.multiplicity(301, 4, 3)),
    ("near tie", lambda: E.near_tie(300, 2)),
    ("negative dominant", lambda: E.negative_dominant(300, 3)),
    ("int64", lambda: E.shifted_low_rank(200, 2, scale=2 ** 24)),
]


@pytest.mark.parametrize("name,build", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_reference_spectrum_matches_lapack_on_the_oracle_b(O, name, build):
    sp = build()
    assert sp.s.dtype == np.int64 and np.array_equal(sp.s, sp.s.T)
    b, w, u, lam = _lapack(O, sp)
    scale = np.abs(w).max()
    assert abs(sp.norm - scale) <= 1e-12 * scale + sp.lam_tol
    # the whole predicted spectrum, multiplicities included (a level of the planted family below its top k + 1 stands for
    # everything below it)
    left = np.sort(w)[::-1].tolist()
    for value, mult in sorted(sp.levels, key=lambda t: -t[0]):
        near = [x for x in left if abs(x - value) <= 1e-12 * scale + sp.lam_tol]
        if sp.family == "planted" and mult > 1:
            assert all(x <= value + 1e-12 * scale for x in left) and len(left) == mult
            continue
        assert len(near) >= mult, (value, mult, near[:5])
        for x in sorted(near, key=lambda x: abs(x - value))[:mult]:
            left.remove(x)
    assert sp.family == "planted" or not left
    # the top k, their vectors and cluster subspaces, through the same checker as the GPU tests
    E.check_pairs(sp, u, lam, lambda x: b @ x, name)
    if name == "int64":
        assert np.abs(sp.s).max() > 2 ** 31


def test_weyl_estimate_bounds_the_exact_norm():
    rng = np.random.default_rng(3)
    for n in (50, 333, 700):
        a = E.symmetric_noise(rng, n)
        exact = np.abs(np.linalg.eigvalsh(a.astype(np.float64))).max()
        est = E.norm_estimate(a)
        assert est <= exact * (1 + 1e-6) and 1.1 * est >= exact, (n, est, exact)


def test_families_have_the_structure_they_promise():
    assert np.all(E.negative_dominant(400, 2).lam < 0)
    sp = E.multiplicity(400, 4, 3)
    assert ([0, 1, 2], True) in sp.groups
    sp = E.near_tie(400, 2)
    assert 0 < abs(sp.lam[0] - sp.lam[1]) <= 1e-8 * sp.norm and sp.groups == [([0, 1], True)]
    sp = E.shifted_low_rank(300, 5, v=3, c=0)
    assert ([3, 4], False) in sp.groups and np.all(sp.lam[3:] == 0)


def test_parity_helpers_are_the_module_s():
    from test_gpu_parity import _block_constant_similarity, _centred_matvec_host, _reduced_eigenvalues
    assert _block_constant_similarity is E._block_constant_similarity
    assert _reduced_eigenvalues is E._reduced_eigenvalues and _centred_matvec_host is E._centred_matvec_host


def test_checker_rejects_what_each_bar_is_for(O):
    """A perturbed answer fails the check that is meant to catch it."""
    sp = E.shifted_low_rank(300, 3, v=8)
    b, _, u, lam = _lapack(O, sp)
    bmul = lambda x: b @ x   # noqa: E731
    E.check_pairs(sp, u, lam, bmul)
    with pytest.raises(AssertionError, match="eigenvalues"):
        E.check_pairs(sp, u, lam * (1 + 1e-10), bmul)
    with pytest.raises(AssertionError, match="residual"):
        E.check_pairs(sp, u, lam, lambda x: (1 + 1e-10) * (b @ x))
    swapped = u.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    with pytest.raises(AssertionError, match="residual|vector"):
        E.check_pairs(sp, swapped, lam, bmul)
    with pytest.raises(AssertionError, match="sign rule"):
        E.check_pairs(sp, u * np.array([1.0, -1.0, 1.0]), lam, bmul)


def test_lanczos_bars_of_every_case_stay_below_the_parity_bar():
    """The Lanczos bars (E.lanczos_bars) are derived from the path's acceptance rule, residual <= 8e-11 ||B||, and grow with
    1 / gap.  Every case of tests/test_gpu_lanczos_bands.py keeps the solver's share of its vector and subspace bar,
    VEC_BAR + 2e-10 ||B|| / gap, below the project's 1e-6 parity bar (REL_GAP = 1e-3 bounds it by 2.1e-7), and so the whole
    bar wherever the reference is exact (vec_tol = 0; the Davis-Kahan term of the perturbed family is the reference's own
    uncertainty).  The schedule helper is held to the constants of lanczos_single."""
    import test_gpu_lanczos_bands as LB
    for case in LB.CASES:
        sp = LB.spectrum(case)
        bars = E.lanczos_bars(sp)
        assert bars["eig"] == bars["res"] == 1e-10 and bars["orth"] == E.ORTH_BAR
        assert sp.gap.shape == (sp.k,) and np.all(sp.gap >= E.REL_GAP * sp.norm), (case, sp.gap / sp.norm)
        for members, whole in sp.groups:
            if not whole or np.isnan(sp.vecs[:, members]).any():
                continue
            share = max(E.VEC_BAR, E.SUB_BAR) + max(bars["vec"][t] for t in members)
            assert share <= 2.1e-7, (case, members, share)
            if not sp.lam_tol:
                assert share + max(sp.vec_tol[t] for t in members) < 1e-6, (case, members)
    assert sorted(LB.schedule(4100, 2)) == [12, 16, 20, 24, 32, 40, 48, 56, 64, 96, 144, 216, 324, 486, 512]
    assert sorted(LB.schedule(33, 2)) == [12, 16, 20, 24, 32, 33] and min(LB.schedule(600, 15)) == 17


def test_check_pairs_takes_other_bars(O):
    """bars= replaces the dense bars: a residual of 5e-11 ||B|| fails the dense bar and passes the Lanczos one; one
    of 2e-10 ||B|| fails both."""
    sp = E.shifted_low_rank(300, 3, v=8)
    b, _, u, lam = _lapack(O, sp)
    off = lambda x: (1 + 5e-11 * sp.norm / np.abs(lam).min()) * (b @ x)   # noqa: E731
    with pytest.raises(AssertionError, match="residual"):
        E.check_pairs(sp, u, lam, off)
    E.check_pairs(sp, u, lam, off, bars=E.lanczos_bars(sp))
    with pytest.raises(AssertionError, match="residual"):
        E.check_pairs(sp, u, lam, lambda x: (1 + 2e-10 * sp.norm / np.abs(lam).min()) * (b @ x), bars=E.lanczos_bars(sp))

"""GPU tests of the least-squares projection of sparsely called samples on a GRM engine (pcoa_grm_project_lsq,
--grm-project-lsq): on cohorts where every sum is exact the normal equations equal the numpy twin's bit for bit, at every shape
at which the kernels of grm_lsq.hip take another path and at every chunk tail; a pair's sum has the same bits whatever chunk it
rode in; P is pcoa_grm_project's numerator; the solve is held against the exact rational solution inside the forward-error bound
of a Cholesky solve; real vectors stay inside the summation bound; sparsely called samples land where their full data puts
them; undetermined samples are flagged; nothing writes a store; both hosts print the same rows.  The twin is
test_grm_lsq_cpu.py's."""
import ctypes
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT, align_sign, load_golden, load_pkg, write_golden_plink
from test_grm_cpu import _run_driver, _run_python, dosage, exact_cohort, pack_bed, random_codes, spec_grm_counts, spec_grm_weights
from test_grm_project_cpu import panel_and_held_out, read_fileset, spec_grm_project, split_fileset, top_eigenpairs, write_fileset
from test_grm_lsq_cpu import lsq_solve, mask_calls, nearest_centroid, slopes, spec_grm_lsq, undetermined_cohort
from test_gpu_grm import SEGMENT_KNOB, product

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def P():
    return load_pkg()


def feed(eng, codes, ref_is_a1, cuts=None):
    rows = pack_bed(codes)
    cuts = cuts or [0, codes.shape[0]]
    for a, b in zip(cuts[:-1], cuts[1:]):
        eng.accumulate_plink_bed(np.ascontiguousarray(rows[a:b]), ref_is_a1=ref_is_a1)
    eng.sync()


def split_normal(nrm, k):
    """out_normal [K (K + 1) / 2 + K][Nq] -> (H [Nq][pairs], P [Nq][K])."""
    pairs = k * (k + 1) // 2
    return np.ascontiguousarray(nrm[:pairs].T), np.ascontiguousarray(nrm[pairs:].T)


def full_h(hq, k):
    a = np.zeros((k, k))
    for c in range(k):
        for c2 in range(c + 1):
            a[c, c2] = a[c2, c] = hq[c * (c + 1) // 2 + c2]
    return a


def exact_pair(seed, n, nq, v, ref_p, ref_s, k):
    """Panel and study from exact_cohort (M' the largest power of two below V, the unused rows among the used), half of the
    study's slots set to 01, integer components."""
    rng = np.random.default_rng(seed)
    vu = 1 << ((v - 1).bit_length() - 1)
    panel = exact_cohort(rng, n, vu, v - vu, ref_p)
    study = mask_calls(exact_cohort(rng, max(nq, 2), v, 0, ref_s)[:, :nq], 0.5, seed + 1)
    comps = rng.integers(-8, 9, size=(n, k)).astype(np.float64)
    return panel, study, comps, vu


# ---- exact cohorts ----------------------------------------------------------------------------------------------------------
# (panel N, N_study, V, num_pc, ref_is_a1 of the panel, of the study).  N_study: one sample, a partly live word (15), a whole
# word (16), two words (17), three (33), a second wave and a second workgroup row (1,025).  V: the row unroll of 4 and a range of
# 512 rows minus one, exact, plus one, and 2,049 = four ranges + 1.  num_pc 1, 2, 3, 4, 5, 8, 16: 1, 3, 6, 10, 15, 36 and 136
# pairs, every tail of the chunks of 4, 2 and 1.
EXACT = [
    (32, 1, 31, 1, False, False),
    (33, 15, 32, 2, True, False),
    (65, 16, 33, 3, False, True),
    (1025, 17, 511, 4, True, True),
    (65, 33, 512, 5, False, False),
    (33, 1025, 513, 8, True, False),
    (1025, 1025, 2049, 16, False, True),
]


@pytest.mark.parametrize("n,nq,v,k,ref_p,ref_s", EXACT)
def test_the_normal_equations_equal_the_twin_bit_for_bit_on_exact_cohorts(P, n, nq, v, k, ref_p, ref_s):
    """mu_v = 1, d_v = 2 and integer components: t is an even integer vector, p = t t' / 2 an integer, and every partial sum of H
    and P an integer far below 2^53 (at most 2,049 x (2 x 1,025 x 8)^2 / 2 < 2^39), so H and P must equal the twin's whatever the
    order of the additions; the solve then runs on identical inputs in the header's sequence and has the twin's bits too."""
    panel, study, comps, vu = exact_pair(1000 * n + v, n, nq, v, ref_p, ref_s, k)
    solve = nq * k <= 33 * 8
    want_h, want_p, want_x, want_det = spec_grm_lsq(panel, ref_p, study, ref_s, comps, solve=solve)
    assert spec_grm_weights(spec_grm_counts(panel, ref_p))[3] == vu and want_h.any() and want_p.any()
    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(nq, grm_study=True) as st:
        feed(eng, panel, ref_p)
        feed(st, study, ref_s, cuts=[0, v // 3, v])
        x, called, det, nrm = eng.grm_project_lsq(st, comps, normal=True)
        assert x.shape == (nq, k) and det.shape == (nq,) and nrm.shape == (k * (k + 1) // 2 + k, nq)
        h, p = split_normal(nrm, k)
        assert np.array_equal(h, want_h) and np.array_equal(p, want_p)
        lam = 2.0 ** np.arange(k).astype(np.float64)
        xy, called_mean = eng.grm_project(st, comps, lam)
        assert np.array_equal(called, called_mean) and called.dtype == np.int32
        if solve:
            assert np.array_equal(det, want_det) and np.array_equal(x[det], want_x[want_det]) and np.isnan(x[~det]).all()
        else:
            x2, det2 = lsq_solve(h[:40], p[:40])
            assert np.array_equal(det[:40], det2) and np.array_equal(x[:40][det2], x2[det2])
        assert eng.grm_lsq_stats()["grm_lsq_undetermined"] == int((~det).sum())
        # the same call without the optional outputs
        assert eng.grm_project_lsq(st, comps)[0].tobytes() == x.tobytes()


# ---- rounded cohorts --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rounded():
    rng = np.random.default_rng(2460)
    n, nq, v = 260, 37, 1000
    panel = random_codes(rng, v, n, missing=0.05)
    study = random_codes(rng, v, nq, missing=0.4)
    return {"n": n, "nq": nq, "v": v, "panel": panel, "study": study, "comps": rng.standard_normal((n, 16)),
            "lam": rng.uniform(0.5, 3.0, size=16)}


def test_a_pair_sum_has_the_same_bits_whatever_chunk_it_rode_in(P, rounded):
    """Every H column of a num_pc = 16 call (34 chunks of four pairs) equals the column of a two-component call on that pair
    alone (a chunk of two and one of one), and so does every P column."""
    r = rounded
    with P.PcoaEngine(r["n"], grm=True) as eng, P.PcoaEngine(r["nq"], grm_study=True) as st:
        feed(eng, r["panel"], False)
        feed(st, r["study"], False)
        h16, p16 = split_normal(eng.grm_project_lsq(st, r["comps"], normal=True)[3], 16)
        assert np.isfinite(h16).all() and h16.any()
        for c in range(16):
            for c2 in range(c):
                h2, p2 = split_normal(eng.grm_project_lsq(st, r["comps"][:, [c2, c]], normal=True)[3], 2)
                assert h2[:, 1].tobytes() == h16[:, c * (c + 1) // 2 + c2].tobytes(), (c, c2)
                assert h2[:, 0].tobytes() == h16[:, c2 * (c2 + 1) // 2 + c2].tobytes(), (c, c2)
                assert h2[:, 2].tobytes() == h16[:, c * (c + 1) // 2 + c].tobytes(), (c, c2)
                assert p2[:, 1].tobytes() == p16[:, c].tobytes() and p2[:, 0].tobytes() == p16[:, c2].tobytes(), (c, c2)
        st5 = eng.grm_lsq_stats()
        assert st5["grm_lsq_calls"] == 121 and st5["grm_lsq_pair_vectors"] == 136 + 120 * 3
        assert st5["grm_lsq_pairs_seconds"] > 0 and st5["grm_lsq_solve_seconds"] > 0


def test_p_is_the_numerator_of_grm_project_and_call_cuts_do_not_enter(P, rounded):
    r = rounded
    v = r["v"]
    for k in (1, 2, 3, 8):
        comps, lam = r["comps"][:, :k], r["lam"][:k]
        outs = []
        for cuts_p, cuts_s in (([0, v], [0, v]), ([0, 1, 33, 513, v], [0, 250, 999, v])):
            with P.PcoaEngine(r["n"], grm=True) as eng, P.PcoaEngine(r["nq"], grm_study=True) as st:
                feed(eng, r["panel"], False, cuts=cuts_p)
                feed(st, r["study"], False, cuts=cuts_s)
                x, called, det, nrm = eng.grm_project_lsq(st, comps, normal=True)
                xy, called_mean = eng.grm_project(st, comps, lam)
                m = eng.grm_info()[1]
                h, p = split_normal(nrm, k)
                assert (p / float(m) / lam[None, :]).tobytes() == xy.tobytes() and np.array_equal(called, called_mean)
                outs.append((x.tobytes(), nrm.tobytes(), det.tobytes()))
        assert outs[0] == outs[1], k


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(tests)r)
from conftest import load_pkg
from test_grm_cpu import pack_bed, random_codes
from test_grm_lsq_cpu import spec_grm_lsq
from test_gpu_grm_lsq import exact_pair, split_normal
P = load_pkg()
n, nq, v, k = 130, 37, 1000, 5
panel, study, comps, vu = exact_pair(96, n, nq, v, False, True, k)
want_h, want_p, want_x, want_det = spec_grm_lsq(panel, False, study, True, comps)
rng = np.random.default_rng(97)
rpanel, rstudy = random_codes(rng, v, n), random_codes(rng, v, nq, missing=0.4)
rcomps, lam = rng.standard_normal((n, 3)), rng.uniform(0.5, 2.0, size=3)
with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(nq, grm_study=True) as st:
    rows_p, rows_s = pack_bed(panel), pack_bed(study)
    for r0 in range(0, v, 250):
        eng.accumulate_plink_bed(rows_p[r0:r0 + 250], ref_is_a1=False)
    for r0 in range(0, v, 333):
        st.accumulate_plink_bed(rows_s[r0:r0 + 333], ref_is_a1=True)
    assert eng.grm_info()[2] == 11 * 96 * 48 and st.grm_info()[2] == 11 * 96 * 16, (eng.grm_info(), st.grm_info())
    x, called, det, nrm = eng.grm_project_lsq(st, comps, normal=True)
    h, p = split_normal(nrm, k)
    assert np.array_equal(h, want_h) and np.array_equal(p, want_p) and np.array_equal(det, want_det)
    assert np.array_equal(x[det], want_x[want_det])
    eng.reset(); st.reset()
    rows_p, rows_s = pack_bed(rpanel), pack_bed(rstudy)
    for r0 in range(0, v, 250):
        eng.accumulate_plink_bed(rows_p[r0:r0 + 250])
    for r0 in range(0, v, 333):
        st.accumulate_plink_bed(rows_s[r0:r0 + 333])
    x, called, det, nrm = eng.grm_project_lsq(st, rcomps, normal=True)
    xy, called_mean = eng.grm_project(st, rcomps, lam)
    h, p = split_normal(nrm, 3)
    assert (p / float(eng.grm_info()[1]) / lam[None, :]).tobytes() == xy.tobytes() and np.array_equal(called, called_mean)
    assert det.all() and np.isfinite(x).all()
print("SEGMENTS-OK")
"""


def test_the_bits_hold_across_segment_boundaries():
    """Both stores in segments of 96 rows (the knob is read once per process: a fresh child): the exact cohort still gives the
    twin's integers, and P is still pcoa_grm_project's numerator."""
    env = dict(os.environ)
    env[SEGMENT_KNOB] = "96"
    res = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests")}], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0 and "SEGMENTS-OK" in res.stdout, res.stdout[-3000:]


# ---- the solve --------------------------------------------------------------------------------------------------------------
def rational_solve(hq, pq, k):
    """The exact solution of the integer system, by Gaussian elimination over the rationals."""
    a = [[Fraction(int(hq[max(i, j) * (max(i, j) + 1) // 2 + min(i, j)])) for j in range(k)] + [Fraction(int(pq[i]))] for i in range(k)]
    for i in range(k):
        piv = next(r for r in range(i, k) if a[r][i] != 0)
        a[i], a[piv] = a[piv], a[i]
        for r in range(k):
            if r != i and a[r][i] != 0:
                f = a[r][i] / a[i][i]
                a[r] = [x - f * y for x, y in zip(a[r], a[i])]
    return np.array([float(a[i][k] / a[i][i]) for i in range(k)])


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_the_solve_against_the_exact_rational_solution(P, k):
    """num_pc = 1: x = P / H bit for bit.  num_pc 2, 3, 5: ||x - x*||_2 <= 8 K^2 2^-53 kappa_2(H_q) ||x*||_2 with x* the exact
    rational solution of the integer H_q, P_q and kappa_2 numpy's on the integer H_q, on cohorts with kappa_2 <= 10^6 (asserted).
    Largest observed fraction of the bound on an MI355X: 0.030 (K = 2), 0.0061 (K = 3), 0.0023 (K = 5)."""
    n, nq, v = 65, 33, 64
    panel, study, comps, vu = exact_pair(700 + k, n, nq, v, False, False, k)
    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(nq, grm_study=True) as st:
        feed(eng, panel, False)
        feed(st, study, False)
        x, called, det, nrm = eng.grm_project_lsq(st, comps, normal=True)
    h, p = split_normal(nrm, k)
    assert np.array_equal(h, np.round(h)) and np.array_equal(p, np.round(p)) and det.all()
    if k == 1:
        assert x[:, 0].tobytes() == (p[:, 0] / h[:, 0]).tobytes()
        return
    worst = 0.0
    for q in range(nq):
        kappa = np.linalg.cond(full_h(h[q], k), 2)
        assert kappa <= 1e6, (q, kappa)
        want = rational_solve(h[q], p[q], k)
        bound = 8 * k * k * U * kappa * np.linalg.norm(want)
        err = np.linalg.norm(x[q] - want)
        worst = max(worst, err / bound)
        assert err <= bound, (q, err, bound)
    print("K = %d: largest ||x - x*|| / bound = %.3g" % (k, worst))


# ---- real vectors -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bn():
    panel, study, pop_p, pop_s = panel_and_held_out()
    comps, lam, lam_all = top_eigenpairs(panel, False, 3)
    return {"panel": panel, "study": study, "masked": mask_calls(study, 0.5, 0), "comps": comps, "lam": lam, "lam_all": lam_all,
            "pop_p": pop_p, "pop_s": pop_s}


def test_real_vectors_stay_inside_the_summation_and_solve_bounds(P, bn):
    """compute(3) on the device, the study masked at 0.5.  Against the twin evaluated on the device's own t:
    |H - twin| <= (V + 16) 2^-52 sum_v c_vq |t_vc t_vc'| / d_v entry by entry, |P - twin| <= (V + 16) 2^-52 sum_v (g + mu c)_vq |t_vc|,
    and ||x - twin|| <= 8 K^2 2^-53 kappa ||x*|| + kappa (||dP|| + ||dH||_F ||x*||) / ||H||_2 / (1 - kappa ||dH||_F / ||H||_2): the
    solve's forward-error bound plus those perturbations carried through kappa_2.  End to end x is within 1e-6 of the twin on
    numpy's eigenvectors, and the placement keeps the slope and the centroids of the CPU claim."""
    panel, masked = bn["panel"], bn["masked"]
    v, k = panel.shape[0], 3
    with P.PcoaEngine(260, grm=True) as eng, P.PcoaEngine(40, grm_study=True) as st:
        feed(eng, panel, False)
        feed(st, masked, False)
        comps, lam, _ = eng.compute(k)
        x, called, det, nrm = eng.grm_project_lsq(st, comps, normal=True)
        t = eng.grm_weights(comps, lam, scaled=False)
    h, p = split_normal(nrm, k)
    th, tp, tx, tdet = spec_grm_lsq(panel, False, masked, False, comps, t=t)
    assert det.all() and tdet.all()
    mu, d, used, m = spec_grm_weights(spec_grm_counts(panel, False))
    g, c = dosage(masked, False)
    cf = c.astype(np.float64)
    eps = (v + 16) * 2.0 ** -52
    with np.errstate(divide="ignore", invalid="ignore"):
        hb = np.stack([eps * (cf.T @ np.where(used, np.abs(t[:, a] * t[:, b]) / d, 0.0)) for a in range(k) for b in range(a + 1)], axis=1)
    pb = eps * ((g.astype(np.float64) + mu[:, None] * cf).T @ np.abs(t))
    print("largest |H - twin| / bound = %.3g, |P - twin| / bound = %.3g" % ((np.abs(h - th) / hb).max(), (np.abs(p - tp) / pb).max()))
    assert np.all(np.abs(h - th) <= hb) and np.all(np.abs(p - tp) <= pb)
    worst = 0.0
    for q in range(40):
        a = full_h(th[q], k)
        kappa, norm = np.linalg.cond(a, 2), np.linalg.norm(a, 2)
        dh = np.linalg.norm(full_h(hb[q], k))
        bound = 8 * k * k * U * kappa * np.linalg.norm(tx[q]) \
            + kappa * (np.linalg.norm(pb[q]) + dh * np.linalg.norm(tx[q])) / norm / (1.0 - kappa * dh / norm)
        worst = max(worst, np.linalg.norm(x[q] - tx[q]) / bound)
        assert np.linalg.norm(x[q] - tx[q]) <= bound, q
    print("largest ||x - twin|| / bound = %.3g" % worst)
    # end to end, on numpy's eigenvectors
    want = spec_grm_lsq(panel, False, masked, False, bn["comps"])[2]
    assert np.abs(align_sign(x, want) - want).max() < 1e-6
    assert np.array_equal(called, spec_grm_project(panel, False, masked, False, bn["comps"], bn["lam"])[1])
    # the claim, on the first two axes of the device output
    full, _ = spec_grm_project(panel, False, bn["study"], False, comps[:, :2], lam[:2])
    with P.PcoaEngine(260, grm=True) as eng, P.PcoaEngine(40, grm_study=True) as st:
        feed(eng, panel, False)
        feed(st, masked, False)
        x2, _, det2 = eng.grm_project_lsq(st, comps[:, :2])
        shrunk, _ = eng.grm_project(st, comps[:, :2], lam[:2])
    s = slopes(x2, full)
    print("slopes: least squares %s, mean-imputed %s" % (s, slopes(shrunk, full)))
    assert det2.all() and np.all(s >= 0.9) and np.all(s <= 1.15)
    assert np.array_equal(nearest_centroid(x2, comps[:, :2], bn["pop_p"]), bn["pop_s"])
    assert np.all(slopes(shrunk, full) < 0.6)      # mean imputation at a call share of about 0.5


# ---- undetermined samples ---------------------------------------------------------------------------------------------------
def test_undetermined_samples_get_nan_a_zero_flag_and_are_counted(P):
    panel, study, comps, expect = undetermined_cohort()
    want = spec_grm_lsq(panel, False, study, False, comps)
    with P.PcoaEngine(panel.shape[1], grm=True) as eng, P.PcoaEngine(study.shape[1], grm_study=True) as st:
        feed(eng, panel, False)
        feed(st, study, False)
        x, called, det, nrm = eng.grm_project_lsq(st, comps, normal=True)
        assert np.array_equal(det, expect) and np.isnan(x[~expect]).all() and np.array_equal(x[expect], want[2][expect])
        assert eng.grm_lsq_stats()["grm_lsq_undetermined"] == 3
        assert called[1] == 1 and called[3] == 0 and called[5] == 2
        # the count is the last call's
        good = np.nonzero(expect)[0]
        with P.PcoaEngine(good.size, grm_study=True) as st2:
            feed(st2, np.ascontiguousarray(study[:, good]), False)
            x2, _, det2 = eng.grm_project_lsq(st2, comps)
            assert det2.all() and np.array_equal(x2, want[2][expect]) and eng.grm_lsq_stats()["grm_lsq_undetermined"] == 0


# ---- state ------------------------------------------------------------------------------------------------------------------
def test_nothing_writes_a_store_settings_are_honoured_and_refusals_leave_both_ctxs_usable(P, rounded):
    L = P._lib
    r = rounded
    n, nq, v = r["n"], r["nq"], r["v"]
    comps, lam = r["comps"][:, :3], r["lam"][:3]
    xv, xs = r["comps"][:, 8], r["comps"][:nq, 9]
    eps = (v + 16) * 2.0 ** -52

    def refused(code, call, *words):
        with pytest.raises(P.PcoaError) as ei:
            call()
        assert ei.value.code == code and len(str(ei.value)) > 30, str(ei.value)
        for word in words:
            assert word in str(ei.value), (word, str(ei.value))

    def state(eng, other):
        return (product(eng, xv).tobytes(), eng.grm_counts().tobytes(), other.grm_counts().tobytes(),
                eng.grm_project(other, comps, lam)[0].tobytes(), eng.grm_project(eng, comps, lam)[0].tobytes())

    def check_against_twin(eng, st, min_maf=0.0):
        """The call under the engine's current settings: P is grm_project's numerator, H the twin's on the device's t."""
        x, called, det, nrm = eng.grm_project_lsq(st, comps, normal=True)
        xy, called_mean = eng.grm_project(st, comps, lam)
        h, p = split_normal(nrm, 3)
        assert (p / float(eng.grm_info()[1]) / lam[None, :]).tobytes() == xy.tobytes() and np.array_equal(called, called_mean)
        t = eng.grm_weights(comps, lam, scaled=False)
        th = spec_grm_lsq(r["panel"], False, r["study"], False, comps, min_maf, t=t, solve=False)[0]
        mu, d, used, m = spec_grm_weights(spec_grm_counts(r["panel"], False), min_maf)
        cf = dosage(r["study"], False)[1].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            hb = np.stack([eps * (cf.T @ np.where(used, np.abs(t[:, a] * t[:, b]) / d, 0.0)) for a in range(3) for b in range(a + 1)], axis=1)
        assert np.all(np.abs(h - th) <= hb) and det.all()
        return nrm.tobytes()

    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(nq, grm_study=True) as st, P.PcoaEngine(nq, grm_study=True) as short:
        feed(eng, r["panel"], False)
        feed(st, r["study"], False)
        feed(short, r["study"][:v - 1], False)
        s0 = state(eng, st)
        n0 = check_against_twin(eng, st)
        own = eng.grm_project_lsq(eng, comps)        # the panel as its own study
        assert own[2].all() and own[0].shape == (n, 3)
        assert state(eng, st) == s0
        # refusals
        refused(L.PCOA_ERR_STATE, lambda: st.grm_project_lsq(st, comps[:nq]), "pcoa_create_grm")
        refused(L.PCOA_ERR_STATE, lambda: eng.grm_project_lsq(short, comps), str(v - 1), str(v))
        refused(L.PCOA_ERR_INVALID_ARG, lambda: eng.grm_project_lsq(st, comps[:, :0]), "num_pc")
        refused(L.PCOA_ERR_INVALID_ARG, lambda: eng.grm_project_lsq(st, np.zeros((n, 17))), "num_pc", "16")
        u = np.ascontiguousarray(comps.T)
        refused(L.PCOA_ERR_INVALID_ARG, lambda: eng._check(eng._lib.pcoa_grm_project_lsq(
            eng._ctx, st._ctx, 3, ctypes.c_void_p(u.ctypes.data), None, None, None, None)), "out_coords")
        assert state(eng, st) == s0 and check_against_twin(eng, st) == n0
        # a changed min_maf, a changed variant filter and an installed LD mask are honoured, and undone
        m0 = eng.grm_info()[1]
        eng.grm_set_min_maf(0.05)
        m1 = eng.grm_info()[1]
        n1 = check_against_twin(eng, st, 0.05)
        assert 0 < m1 < m0 and n1 != n0
        eng.grm_set_min_maf(0.0)
        assert check_against_twin(eng, st) == n0
        eng.grm_set_variant_filters(max_missing=0.05)
        m2 = eng.grm_info()[1]
        n2 = check_against_twin(eng, st)
        assert 0 < m2 < m0 and n2 != n0
        eng.grm_set_variant_filters()
        assert check_against_twin(eng, st) == n0
        cand, kept = eng.grm_ld_prune(50, 0.001)
        assert 0 < kept < cand == m0 and eng.grm_info()[1] == kept
        n3 = check_against_twin(eng, st)
        assert n3 != n0
        eng.grm_ld_clear()
        assert check_against_twin(eng, st) == n0 and state(eng, st) == s0
        # M' = 0
        eng.reset()
        st.reset()
        feed(eng, np.full((5, n), 3, np.uint8), False)
        feed(st, np.full((5, nq), 3, np.uint8), False)
        refused(L.PCOA_ERR_INVALID_ARG, lambda: eng.grm_project_lsq(st, comps), "M' = 0")
        eng.reset()
        st.reset()
        feed(eng, r["panel"], False)
        feed(st, r["study"], False)
        assert check_against_twin(eng, st) == n0 and state(eng, st) == s0


# ---- hosts ------------------------------------------------------------------------------------------------------------------
def table(text):
    rows = [ln.split("\t") for ln in text.splitlines() if ln.count("\t") == 3]
    return [(r[0], r[1]) for r in rows], np.array([[float(r[2]), float(r[3])] for r in rows])


def test_both_hosts_place_sparse_and_mind_removed_samples_by_least_squares(tmp_path):
    """The tile260 golden split into a panel of 240 and a study of 20; 60 % of the study's calls and 90 % of five panel samples'
    calls are masked, and --grm-mind 0.5 takes those five out.  With --grm-project-lsq both hosts print the same bytes, the study's
    and the five samples' rows (sorted by name behind the kept samples') within 1e-6 of the twin on numpy's eigenvectors of the 235; without it the five are absent and the
    study's rows are the mean-imputed ones."""
    g = load_golden("tile260")
    n = write_golden_plink(g, str(tmp_path / "tile260"))
    study_cols = np.arange(7, n, 13)[:20]
    split_fileset(str(tmp_path / "tile260"), str(tmp_path / "panel0"), str(tmp_path / "cohortB0"), study_cols)
    panel, bim, fam = read_fileset(str(tmp_path / "panel0"))
    study, _, sfam = read_fileset(str(tmp_path / "cohortB0"))
    five = np.array([3, 50, 51, 120, 239])
    panel[:, five] = mask_calls(np.ascontiguousarray(panel[:, five]), 0.9, 5)
    study = mask_calls(study, 0.6, 6)
    write_fileset(str(tmp_path / "panel"), panel, bim, fam)
    write_fileset(str(tmp_path / "cohortB"), study, bim, sfam)
    stay = np.setdiff1d(np.arange(panel.shape[1]), five)
    assert np.array_equal(np.nonzero((panel == 1).mean(axis=0) > 0.5)[0], five)
    kept = np.ascontiguousarray(panel[:, stay])
    comps, lam, lam_all = top_eigenpairs(kept, False, 2)
    assert (lam_all[0] - lam_all[1]) / lam_all[0] >= 0.01 and (lam_all[1] - lam_all[2]) / lam_all[0] >= 0.01
    want_study = spec_grm_lsq(kept, False, study, False, comps)
    want_five = spec_grm_lsq(kept, False, np.ascontiguousarray(panel[:, five]), False, comps)
    assert want_study[3].all() and want_five[3].all()
    mean_study, called = spec_grm_project(kept, False, study, False, comps, lam)
    m = spec_grm_weights(spec_grm_counts(kept, False))[3]
    base = ["--input-path", str(tmp_path / "panel.bed"), "--grm", "--grm-mind", "0.5", "--grm-project-path", str(tmp_path / "cohortB.bed"),
            "--grm-project-removed"]
    outs = []
    for run in (_run_driver, _run_python):
        lsq = run(base + ["--grm-project-lsq"])
        plain = run(base)
        assert lsq.returncode == 0 and plain.returncode == 0, lsq.stderr[-2000:]
        assert "Projected 20 samples over %d used variants (mean call share %.4f, least squares, 0 undetermined)" \
            % (m, float(called.mean()) / m) in lsq.stderr, lsq.stderr[-1500:]
        assert "Projected 5 removed samples over %d used variants" % m in lsq.stderr and "least squares, 0 undetermined" in lsq.stderr
        assert "Projected 20 samples over %d used variants (mean call share %.4f)\n" % (m, float(called.mean()) / m) in plain.stderr
        assert "removed samples" not in plain.stderr and "least squares" not in plain.stderr
        ids, xy = table(lsq.stdout)
        ids_p, xy_p = table(plain.stdout)
        # the placed samples follow the kept ones, sorted by name among themselves
        tail = sorted([(ln.split()[1], "cohortB", want_study[2][q]) for q, ln in enumerate(sfam)]
                      + [(fam[i].split()[1], "panel", want_five[2][j]) for j, i in enumerate(five)], key=lambda t: t[0])
        tail_p = sorted([(ln.split()[1], "cohortB", mean_study[q]) for q, ln in enumerate(sfam)], key=lambda t: t[0])
        assert len(ids) == 235 + 20 + 5 and ids[235:] == [(t[0], t[1]) for t in tail]
        assert len(ids_p) == 235 + 20 and ids_p[235:] == [(t[0], t[1]) for t in tail_p] and ids_p[:235] == ids[:235]
        lsq_rows = [ln for ln in lsq.stdout.splitlines() if ln.count("\t") == 3]
        assert lsq_rows[:235] == [ln for ln in plain.stdout.splitlines() if ln.count("\t") == 3][:235]
        signs = np.sign((xy[:235] * comps).sum(axis=0))
        assert np.abs(xy[:235] * signs - comps).max() < 1e-6
        assert np.abs(xy[235:] * signs - np.stack([t[2] for t in tail])).max() < 1e-6
        assert np.abs(xy_p[235:] * signs - np.stack([t[2] for t in tail_p])).max() < 1e-6
        outs.append((lsq.stdout, plain.stdout))
    assert outs[0] == outs[1]

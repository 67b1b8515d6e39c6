"""GPU tests of the SNP weights and the projection of new samples on a GRM engine (pcoa_create_grm_study, pcoa_grm_weights,
pcoa_grm_project): on cohorts where every sum is exact both equal the numpy twins bit for bit, at every shape at which the
kernels of grm_multi.hip take another path; a component has the same bits whatever num_pc is; a study store that holds the
panel's own rows gives the existing product over lambda bit for bit, across segments and call cuts; real vectors stay inside
the summation bound; compute + project reproduces numpy's eigenvectors and their projection; what cannot be served says so and
writes nothing; both hosts emit the same weights file and projected rows.  The twins are test_grm_project_cpu.py's."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, align_sign, load_golden, load_pkg, write_golden_plink
from test_grm_cpu import _run_driver, _run_python, dosage, exact_cohort, pack_bed, random_codes, spec_grm_counts, spec_grm_weights
from test_grm_project_cpu import panel_and_held_out, scale_weights, spec_grm_project, spec_grm_project_bound, spec_grm_t, \
    spec_grm_weights_vectors, split_fileset, top_eigenpairs
from test_gpu_grm import SEGMENT_KNOB, product, store_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return load_pkg()


def feed(eng, codes, ref_is_a1, cuts=None):
    rows = pack_bed(codes)
    cuts = cuts or [0, codes.shape[0]]
    for a, b in zip(cuts[:-1], cuts[1:]):
        eng.accumulate_plink_bed(np.ascontiguousarray(rows[a:b]), ref_is_a1=ref_is_a1)
    eng.sync()


def t_bound(codes, ref_is_a1, comps, min_maf=0.0):
    """(N + 16) 2^-52 d_v (W |u_c|)_v with W = g + mu c: the first pass's share of test_grm_cpu.spec_grm_bound."""
    mu, d, used, m = spec_grm_weights(spec_grm_counts(codes, ref_is_a1), min_maf)
    g, c = dosage(codes, ref_is_a1)
    w = g.astype(np.float64) + mu[:, None] * c.astype(np.float64)
    return (codes.shape[1] + 16) * 2.0 ** -52 * d[:, None] * (w @ np.abs(comps))


FOUR_ROUNDINGS = 4 * 2.0 ** -53   # (double)M' * lambda, d * that, the square root, the quotient


# ---- exact cohorts ----------------------------------------------------------------------------------------------------------
# (panel N, N_study, V, num_pc, ref_is_a1 of the panel, of the study).  N: a ctx's smallest, one sample into the third word, one
# into the second wave's... the sample-direction constants of grm_bits.hip plus one (65: 4 words + 1, 1,025: a wave's 64 words + 1,
# 4,097: a workgroup's group + 1).  N_study: one sample, one partly live word (15), one whole word (16), two words (17, 31), three
# (33), a second wave (1,025).  V: a butterfly block of 16 / 32 rows and a range of 512 rows minus one, exact, plus one, and
# 2,049 = four ranges + 1.  num_pc: a chunk of 1, of 2, 2 + 1, four chunks of 2, four + 1.  The used rows are the largest power
# of two below V, the others (monomorphic, all missing) lie among them.
EXACT = [
    (32, 1, 31, 1, False, False),
    (33, 15, 32, 2, True, False),
    (65, 16, 33, 3, False, True),
    (1025, 17, 511, 8, True, True),
    (4097, 31, 512, 9, False, True),
    (65, 33, 513, 2, True, False),
    (1025, 1025, 2049, 3, False, False),
]


@pytest.mark.parametrize("n,nq,v,k,ref_p,ref_s", EXACT)
def test_weights_and_projection_equal_the_twins_bit_for_bit_on_exact_cohorts(P, n, nq, v, k, ref_p, ref_s):
    """mu_v = 1, d_v = 2, integer-valued "components", eigenvalues that are powers of two: t is an integer vector and every partial
    sum of the projection an integer far below 2^53 (at most 2,049 x 3 x 12 x 4,097 x 8 < 2^32), so the unscaled weights and the
    coordinates must equal the twins whatever the order of the additions."""
    rng = np.random.default_rng(1000 * n + v)
    vu = 1 << ((v - 1).bit_length() - 1)
    panel = exact_cohort(rng, n, vu, v - vu, ref_p)
    study = random_codes(rng, v, nq, missing=0.1)
    comps = rng.integers(-8, 9, size=(n, k)).astype(np.float64)
    lam = 2.0 ** rng.integers(-3, 4, size=k).astype(np.float64)
    want_t = spec_grm_t(panel, ref_p, comps)
    want_xy, want_called = spec_grm_project(panel, ref_p, study, ref_s, comps, lam)
    assert want_t.any() and want_xy.any()
    mu, d, used, m = spec_grm_weights(spec_grm_counts(panel, ref_p))
    assert m == vu and not want_t[~used].any()
    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(nq, grm_study=True) as st:
        feed(eng, panel, ref_p)
        feed(st, study, ref_s, cuts=[0, v // 3, v])
        assert st.grm_info() == (v, 0, store_bytes(nq, v))
        assert np.array_equal(st.grm_counts(), spec_grm_counts(study, ref_s))
        t = eng.grm_weights(comps, lam, scaled=False)
        assert t.shape == (v, k) and np.array_equal(t, want_t)
        # a window that starts and ends inside a block of rows
        assert np.array_equal(eng.grm_weights(comps, lam, scaled=False, first_variant=5, n_variants=v - 11), want_t[5:v - 6])
        assert eng.grm_weights(comps, lam, first_variant=v, n_variants=0).shape == (0, k)
        w = eng.grm_weights(comps, lam, scaled=True)
        want_w = scale_weights(t, d, used, m, lam)
        assert np.all(np.abs(w - want_w) <= FOUR_ROUNDINGS * np.abs(want_w)) and not w[~used].any() and w[used].any()
        xy, called = eng.grm_project(st, comps, lam)
        assert xy.shape == (nq, k) and np.array_equal(xy, want_xy)
        assert called.dtype == np.int32 and np.array_equal(called, want_called)
        # the panel as its own study
        own, own_called = eng.grm_project(eng, comps, lam)
        want_own = spec_grm_project(panel, ref_p, panel, ref_p, comps, lam)
        assert np.array_equal(own, want_own[0]) and np.array_equal(own_called, want_own[1])


# ---- rounded cohorts --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rounded():
    rng = np.random.default_rng(1260)
    n, nq, v = 260, 37, 1000
    panel = random_codes(rng, v, n, missing=0.05)
    study = random_codes(rng, v, nq, missing=0.08)
    return {"n": n, "nq": nq, "v": v, "panel": panel, "study": study, "comps": rng.standard_normal((n, 9)),
            "lam": rng.uniform(0.5, 3.0, size=9)}


def test_a_component_has_the_same_bits_whatever_num_pc_is(P, rounded):
    r = rounded
    with P.PcoaEngine(r["n"], grm=True) as eng, P.PcoaEngine(r["nq"], grm_study=True) as st:
        feed(eng, r["panel"], False)
        feed(st, r["study"], False)
        t9 = eng.grm_weights(r["comps"], r["lam"], scaled=False)
        w9 = eng.grm_weights(r["comps"], r["lam"], scaled=True)
        xy9, called9 = eng.grm_project(st, r["comps"], r["lam"])
        for c in range(9):
            one = (r["comps"][:, c:c + 1], r["lam"][c:c + 1])
            assert eng.grm_weights(*one, scaled=False)[:, 0].tobytes() == t9[:, c].tobytes(), c
            assert eng.grm_weights(*one, scaled=True)[:, 0].tobytes() == w9[:, c].tobytes(), c
            xy1, called1 = eng.grm_project(st, *one)
            assert xy1[:, 0].tobytes() == xy9[:, c].tobytes() and np.array_equal(called1, called9), c
        xy2, _ = eng.grm_project(st, r["comps"][:, 3:5], r["lam"][3:5])          # a pair that is no chunk of the nine
        assert xy2.tobytes() == np.ascontiguousarray(xy9[:, 3:5]).tobytes()


@pytest.mark.parametrize("study_kind", ["grm_study", "grm"])
def test_a_store_of_the_panels_own_rows_gives_the_product_over_lambda(P, rounded, study_kind):
    """coords[:, c] == grm_matvec_device(u_c) / lambda_c bit for bit: the order of additions is the one-vector product's, whatever
    the chunk, and the call cuts of either side do not enter it."""
    r = rounded
    v = r["v"]
    with P.PcoaEngine(r["n"], grm=True) as eng, P.PcoaEngine(r["n"], **{study_kind: True}) as st:
        feed(eng, r["panel"], False, cuts=[0, 1, 33, 513, v])
        feed(st, r["panel"], False, cuts=[0, 250, 999, v])
        for k in (1, 2, 3):
            xy, called = eng.grm_project(st, r["comps"][:, :k], r["lam"][:k])
            for c in range(k):
                want = product(eng, r["comps"][:, c]) / r["lam"][c]
                assert xy[:, c].tobytes() == want.tobytes(), (k, c)
        used = spec_grm_weights(spec_grm_counts(r["panel"], False))[2]
        assert np.array_equal(called, (r["panel"][used] != 1).sum(axis=0))


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(tests)r)
from conftest import load_pkg
from test_grm_cpu import pack_bed, random_codes
import torch
P = load_pkg()
rng = np.random.default_rng(96)
n, v = 130, 1000
codes = random_codes(rng, v, n)
rows = pack_bed(codes)
comps, lam = rng.standard_normal((n, 3)), rng.uniform(0.5, 2.0, size=3)
with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(n, grm_study=True) as st:
    for r0 in range(0, v, 250):
        eng.accumulate_plink_bed(rows[r0:r0 + 250])
    for r0 in range(0, v, 333):
        st.accumulate_plink_bed(rows[r0:r0 + 333])
    assert eng.grm_info()[2] == 11 * 96 * 48 and st.grm_info() == (1000, 0, 11 * 96 * 48), (eng.grm_info(), st.grm_info())
    xy, called = eng.grm_project(st, comps, lam)
    for c in range(3):
        y = eng.grm_matvec_device(torch.from_numpy(np.ascontiguousarray(comps[:, c])).cuda()).cpu().numpy()
        assert xy[:, c].tobytes() == (y / lam[c]).tobytes(), c
print("SEGMENTS-OK")
"""


def test_the_tie_to_the_product_holds_across_segment_boundaries():
    """Both stores in segments of 96 rows (the knob is read once per process: a fresh child)."""
    env = dict(os.environ)
    env[SEGMENT_KNOB] = "96"
    res = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests")}], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0 and "SEGMENTS-OK" in res.stdout, res.stdout[-3000:]


def test_real_vectors_stay_inside_the_summation_bound(P, rounded):
    """|coords - twin| <= (N_panel + V + 16) 2^-52 (W_study^T diag(d) (W_panel |u_c|))_q / (M' lambda_c), the bound of one product
    carried through both passes; the scaled weights are the numpy expression on the device's own t up to its four roundings."""
    r = rounded
    comps, lam = r["comps"][:, :3], r["lam"][:3]
    want, want_called = spec_grm_project(r["panel"], False, r["study"], True, comps, lam)
    bound = spec_grm_project_bound(r["panel"], False, r["study"], True, comps, lam)
    mu, d, used, m = spec_grm_weights(spec_grm_counts(r["panel"], False))
    with P.PcoaEngine(r["n"], grm=True) as eng, P.PcoaEngine(r["nq"], grm_study=True) as st:
        feed(eng, r["panel"], False)
        feed(st, r["study"], True)
        xy, called = eng.grm_project(st, comps, lam)
        t = eng.grm_weights(comps, lam, scaled=False)
        w = eng.grm_weights(comps, lam, scaled=True)
    share = float(np.max(np.abs(xy - want) / bound))
    print("N = %d, N_study = %d, V = %d: largest |coords - twin| / bound = %.3g" % (r["n"], r["nq"], r["v"], share))
    assert np.all(np.abs(xy - want) <= bound) and np.array_equal(called, want_called)
    want_t = spec_grm_t(r["panel"], False, comps)
    assert want_t.any() and np.all(np.abs(t - want_t) <= t_bound(r["panel"], False, comps))
    want_w = scale_weights(t, d, used, m, lam)
    rel = np.abs(w - want_w) / np.where(want_w != 0, np.abs(want_w), 1.0)
    print("scaled weights: largest relative distance to the numpy expression = %.3g (allowed %.3g)" % (rel.max(), FOUR_ROUNDINGS))
    assert np.all(np.abs(w - want_w) <= FOUR_ROUNDINGS * np.abs(want_w))


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bn():
    panel, study, pop_p, pop_s = panel_and_held_out()
    comps, lam, lam_all = top_eigenpairs(panel, False, 3)
    return {"panel": panel, "study": study, "comps": comps, "lam": lam, "lam_all": lam_all, "pop_p": pop_p, "pop_s": pop_s}


def test_compute_then_project_gives_numpys_eigenvectors_and_their_projection(P, bn):
    panel, study = bn["panel"], bn["study"]
    la = bn["lam_all"]
    assert panel.shape == (1000, 260) and study.shape == (1000, 40)
    assert (la[0] - la[1]) / la[0] >= 0.01 and (la[1] - la[2]) / la[0] >= 0.01
    want_xy, want_called = spec_grm_project(panel, False, study, False, bn["comps"][:, :2], bn["lam"][:2])
    with P.PcoaEngine(260, grm=True) as eng, P.PcoaEngine(40, grm_study=True) as st:
        feed(eng, panel, False)
        feed(st, study, False)
        comps, lam, nz = eng.compute(2)
        xy, called = eng.grm_project(st, comps, lam)
        assert np.max(np.abs(lam - bn["lam"][:2]) / bn["lam"][:2]) < 1e-6
        assert np.abs(align_sign(comps, bn["comps"][:, :2]) - bn["comps"][:, :2]).max() < 1e-6
        assert np.abs(align_sign(xy, want_xy) - want_xy).max() < 1e-6
        assert np.array_equal(called, want_called)
        # the held-out samples land nearest their own population's centroid
        centroids = np.stack([comps[bn["pop_p"] == p].mean(axis=0) for p in range(3)])
        nearest = np.argmin(((xy[:, None, :] - centroids[None, :, :]) ** 2).sum(axis=2), axis=1)
        assert np.array_equal(nearest, bn["pop_s"])
        # the weights of three axes are orthonormal, and give the panel's own coordinates back
        comps3, lam3, _ = eng.compute(3)
        w = eng.grm_weights(comps3, lam3)
        gram = w.T @ w
        print("W^T W - I: largest entry %.3g" % np.abs(gram - np.eye(3)).max())
        assert np.abs(gram - np.eye(3)).max() <= 1e-12
        want_w = spec_grm_weights_vectors(panel, False, bn["comps"][:, :2], bn["lam"][:2])   # (three populations: two axes with a gap)
        assert np.abs(align_sign(w[:, :2], want_w) - want_w).max() < 1e-6
        own, _ = eng.grm_project(eng, comps3, lam3)
        assert np.abs(own - comps3).max() < 1e-9


# ---- state ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_stores_untouched(P, rounded):
    import torch
    L = P._lib
    r = rounded
    n, nq, v = r["n"], r["nq"], r["v"]
    comps, lam = r["comps"][:, :2], r["lam"][:2]
    x = r["comps"][:, 8]

    def refused(code, call, *words):
        with pytest.raises(P.PcoaError) as ei:
            call()
        assert ei.value.code == code and len(str(ei.value)) > 30, str(ei.value)
        for word in words:
            assert word in str(ei.value), (word, str(ei.value))
        return str(ei.value)

    with pytest.raises(P.PcoaError) as ei:
        P.PcoaEngine(16, grm=True)
    assert ei.value.code == L.PCOA_ERR_INVALID_ARG and "32" in str(ei.value)
    with P.PcoaEngine(16, grm_study=True) as tiny:
        assert tiny.grm_info() == (0, 0, 0) and tiny.n == 16
    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(nq, grm_study=True) as st, P.PcoaEngine(n) as full, \
            P.PcoaEngine(n, operator=True) as op, P.PcoaEngine(nq, grm_study=True) as short:
        feed(eng, r["panel"], False)
        feed(st, r["study"], False)
        feed(short, r["study"][:v - 1], False)
        y0, c0, s0 = product(eng, x).tobytes(), eng.grm_counts().tobytes(), st.grm_counts().tobytes()
        e0 = eng.compute(2)
        xy0, called0 = eng.grm_project(st, comps, lam)
        t0 = eng.grm_weights(comps, lam, scaled=False)
        xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        # a study ctx has no weights of its own
        messages = set()
        for call in (lambda: st.compute(2), lambda: st.grm_set_min_maf(0.1),
                     lambda: st.grm_matvec_device(torch.zeros(nq, dtype=torch.float64, device="cuda"))):
            messages.add(refused(L.PCOA_ERR_STATE, call, "pcoa_create_grm_study"))
        assert len(messages) == 3
        # the panel must be a GRM ctx with weights of its own; the study a GRM store of as many rows
        for other in (full, op, st):
            refused(L.PCOA_ERR_STATE, lambda: other.grm_project(st, comps[:other.n], lam), "pcoa_create_grm")
            refused(L.PCOA_ERR_STATE, lambda: other.grm_weights(comps[:other.n], lam), "pcoa_create_grm")
        refused(L.PCOA_ERR_STATE, lambda: eng.grm_project(full, comps, lam))
        refused(L.PCOA_ERR_STATE, lambda: eng.grm_project(op, comps, lam))
        refused(L.PCOA_ERR_STATE, lambda: eng.grm_project(short, comps, lam), str(v - 1), str(v))
        # what stays refused on a GRM ctx of either kind
        refused(L.PCOA_ERR_STATE, lambda: eng.loadings(e0[0], e0[1]))
        refused(L.PCOA_ERR_STATE, lambda: eng.project(full, e0[0], e0[1]))
        refused(L.PCOA_ERR_STATE, lambda: st._check(st._lib.pcoa_loadings_begin(st._ctx, 1, None, None, 0)))
        # bad arguments
        refused(L.PCOA_ERR_INVALID_ARG, lambda: eng.grm_project(st, comps, np.array([1.0, 0.0])), "eigenvalue 1")
        refused(L.PCOA_ERR_INVALID_ARG, lambda: eng.grm_project(st, comps, np.array([-1.0, 1.0])), "eigenvalue 0")
        refused(L.PCOA_ERR_INVALID_ARG, lambda: eng.grm_weights(comps, np.array([1.0, float("nan")])), "eigenvalue 1")
        refused(L.PCOA_ERR_INVALID_ARG, lambda: eng.grm_project(st, comps[:, :0], lam[:0]), "num_pc")
        refused(L.PCOA_ERR_INVALID_ARG, lambda: eng.grm_weights(comps[:, :0], lam[:0]), "num_pc")
        refused(L.PCOA_ERR_INVALID_ARG, lambda: eng.grm_weights(comps, lam, first_variant=v - 3, n_variants=4), str(v))
        refused(L.PCOA_ERR_INVALID_ARG, lambda: eng.grm_weights(comps, lam, first_variant=-1, n_variants=2))
        # nothing wrote either store, and both ctxs still serve
        assert product(eng, x).tobytes() == y0 and eng.grm_counts().tobytes() == c0 and st.grm_counts().tobytes() == s0
        e1 = eng.compute(2)
        assert e1[0].tobytes() == e0[0].tobytes() and e1[1].tobytes() == e0[1].tobytes()
        xy1, called1 = eng.grm_project(st, comps, lam)
        assert xy1.tobytes() == xy0.tobytes() and np.array_equal(called1, called0)
        assert eng.grm_weights(comps, lam, scaled=False).tobytes() == t0.tobytes()
        # min_maf changed between two calls: the weights are recomputed as pcoa_compute would
        eng.grm_set_min_maf(0.05)
        want_t = spec_grm_t(r["panel"], False, comps, 0.05)
        used5 = spec_grm_weights(spec_grm_counts(r["panel"], False), 0.05)[2]
        t5 = eng.grm_weights(comps, lam, scaled=False)
        assert 0 < used5.sum() < spec_grm_weights(spec_grm_counts(r["panel"], False))[3]
        assert not t5[~used5].any() and np.all(np.abs(t5 - want_t) <= t_bound(r["panel"], False, comps, 0.05))
        assert t5.tobytes() != t0.tobytes()
        xy5, called5 = eng.grm_project(st, comps, lam)
        want5 = spec_grm_project(r["panel"], False, r["study"], False, comps, lam, 0.05)
        assert np.all(np.abs(xy5 - want5[0]) <= spec_grm_project_bound(r["panel"], False, r["study"], False, comps, lam, 0.05))
        assert np.array_equal(called5, want5[1])
        eng.grm_set_min_maf(0.0)
        assert eng.grm_weights(comps, lam, scaled=False).tobytes() == t0.tobytes()
        # M' = 0
        eng.reset()
        st.reset()
        feed(eng, np.full((5, n), 3, np.uint8), False)
        feed(st, np.full((5, nq), 3, np.uint8), False)
        refused(L.PCOA_ERR_INVALID_ARG, lambda: eng.grm_project(st, comps, lam), "M' = 0")
        refused(L.PCOA_ERR_INVALID_ARG, lambda: eng.grm_weights(comps, lam), "M' = 0")
        eng.reset()
        st.reset()
        feed(eng, r["panel"], False)
        feed(st, r["study"], False)
        assert eng.grm_project(st, comps, lam)[0].tobytes() == xy0.tobytes()


# ---- hosts ------------------------------------------------------------------------------------------------------------------
def table(text):
    rows = [ln.split("\t") for ln in text.splitlines() if ln.count("\t") == 3]
    return [(r[0], r[1]) for r in rows], np.array([[float(r[2]), float(r[3])] for r in rows])


def test_both_hosts_write_the_weights_and_place_the_study_on_the_panels_axes(tmp_path):
    """The tile260 golden as a PLINK fileset, split into a panel of 240 samples and a study of 20: both hosts emit the same
    weights file and the same rows line for line, within 1e-6 of the twins on numpy's eigenvectors; the study's rows follow the
    panel's; without the new flags the panel's output is what --grm alone prints."""
    g = load_golden("tile260")
    n = write_golden_plink(g, str(tmp_path / "tile260"))
    study_cols = np.arange(7, n, 13)[:20]
    panel, study = split_fileset(str(tmp_path / "tile260"), str(tmp_path / "panel"), str(tmp_path / "cohortB"), study_cols)
    assert panel.shape[1] == n - 20 and study.shape[1] == 20
    comps, lam, lam_all = top_eigenpairs(panel, False, 2)
    assert (lam_all[0] - lam_all[1]) / lam_all[0] >= 0.01 and (lam_all[1] - lam_all[2]) / lam_all[0] >= 0.01
    want_w = spec_grm_weights_vectors(panel, False, comps, lam)
    want_xy, want_called = spec_grm_project(panel, False, study, False, comps, lam)
    mu, d, used, m = spec_grm_weights(spec_grm_counts(panel, False))
    line = "Projected 20 samples over %d used variants (mean call share %.4f)" % (m, float(want_called.mean()) / m)
    outs = []
    for k, run in enumerate((_run_driver, _run_python)):
        wpath = str(tmp_path / ("weights%d.tsv" % k))
        plain = run(["--input-path", str(tmp_path / "panel.bed"), "--grm"])
        both = run(["--input-path", str(tmp_path / "panel.bed"), "--grm", "--grm-weights-output-path", wpath,
                    "--grm-project-path", str(tmp_path / "cohortB.bed")])
        assert plain.returncode == 0 and both.returncode == 0, both.stderr[-2000:]
        assert line in both.stderr and "Projected" not in plain.stderr, both.stderr[-1500:]
        ids, xy = table(both.stdout)
        ids_p, xy_p = table(plain.stdout)
        assert len(ids) == n and ids[:n - 20] == ids_p and [i[1] for i in ids[n - 20:]] == ["cohortB"] * 20
        assert [i[0] for i in ids[n - 20:]] == ["S%04d" % c for c in study_cols]
        # the panel's part is what --grm alone prints, byte for byte
        plain_rows = [ln for ln in plain.stdout.splitlines() if ln.count("\t") == 3]
        assert [ln for ln in both.stdout.splitlines() if ln.count("\t") == 3][:n - 20] == plain_rows
        signs = np.sign((xy[:n - 20] * comps).sum(axis=0))
        assert np.abs(xy[:n - 20] * signs - comps).max() < 1e-6
        assert np.abs(xy[n - 20:] * signs - want_xy).max() < 1e-6
        wlines = open(wpath).read().splitlines()
        assert len(wlines) == panel.shape[0]
        cols = [ln.split("\t") for ln in wlines]
        assert [c[:4] for c in cols[:2]] == [["0", "17", "41196312", "rs0"], ["1", "17", "41196319", "rs1"]]
        w = np.array([[float(c[4]), float(c[5])] for c in cols])
        assert np.abs(w * signs - want_w).max() < 1e-6
        assert all(c[4] == "0.0" and c[5] == "0.0" for c, u in zip(cols, used) if not u) and not used.all()
        outs.append((both.stdout, wlines))
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1]

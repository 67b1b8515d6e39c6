"""GPU tests of PC-Relate kinship on the 2-bit store of a GRM engine (pcoa_grm_pcrelate_fit / _beta / _isaf / _block / _pairs):
on cohorts where every partial sum is exact the fit, the individual-specific frequencies, phi and n equal the numpy statements
bit for bit (which pins the lane map of the fp64 instruction, the per-sample masks and every padded instantiation of the kernel);
on rounded cohorts the read-out equals the rule bit for bit, phi is exactly symmetric, independent of how it was cut, and inside
the summation bound of the rule fed the device's own fit; the pair screen reports the rule's records; the admixed cohort's
planted relatives come out and nobody else; the calls refuse what they must, the fit is dropped by what changes the store, and a
ctx answers every existing call with the same bits whether it holds a fit or not."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pcrelate_cohort as C
from conftest import ROOT, load_pkg
from test_gpu_grm_dense import EXACT_V, fill, rectangles, same_bits
from test_grm_cpu import balding_nichols, edge_rows, exact_cohort, random_codes

pytestmark = pytest.mark.gpu

U = 2.0 ** -52


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def vp():
    return load_pkg("variants_pca")


# ---- 1. exact cohorts -------------------------------------------------------------------------------------------------------
def exact_fit_cohort(rng, n, vu, vx, ref_is_a1):
    """exact_cohort (mu_v = 1 on the used rows) with, in every used row, sample 0 heterozygous and sample 1 called: codes are
    swapped inside the row -- or a homozygote of each kind is turned into two heterozygotes -- so the row's counts stay.  With
    hat[0] = e_0, basis[0] = 1, hat[1] = e_1 and basis[1] in {0, 1, -1} (0 at samples 0 and 1): beta_v0 = 1, beta_v1 = g_1v,
    mu_iv in {-0.5, 0, 0.5, 1, 1.5}; a surviving operand has mu = 0.5, a in {-1, 0, 1}, b = 0.5: num is an integer, den = n / 4,
    phi is one division, and the masks differ per sample."""
    hom, ref = (3, 0) if ref_is_a1 else (0, 3)
    codes = exact_cohort(rng, n, vu, vx, ref_is_a1)
    for r in range(codes.shape[0]):
        row = codes[r]
        counts = [(row == q).sum() for q in (hom, ref)]
        if not (counts[0] == counts[1] and counts[0] > 0):
            continue                                          # an unused row (monomorphic or all missing)
        if not (row == 2).any():
            row[np.flatnonzero(row == hom)[0]] = 2
            row[np.flatnonzero(row == ref)[0]] = 2
        if row[0] != 2:
            j = np.flatnonzero(row == 2)[-1]
            row[0], row[j] = row[j], row[0]
        if row[1] == 1:
            j = 2 + np.flatnonzero(row[2:] != 1)[-1]
            row[1], row[j] = row[j], row[1]
        assert row[0] == 2 and row[1] != 1
    basis = np.zeros((2, n))
    basis[0] = 1.0
    basis[1, 2:] = rng.integers(-1, 2, size=n - 2)
    hat = np.zeros((2, n))
    hat[0, 0] = hat[1, 1] = 1.0
    return codes, basis, hat


def padded(m, n_cov):
    out = np.zeros((n_cov, m.shape[1]))
    out[:m.shape[0]] = m
    return out


def block(eng, rect, t, device=False):
    k, n = eng.grm_pcrelate_block(rect[0], rect[1], rect[2], rect[3], t, pairs=True, device=device)
    return (k.cpu().numpy(), n.cpu().numpy()) if device else (k, n)


@pytest.mark.parametrize("n", [32, 33, 47, 63, 64, 65, 130, 1025])
def test_fit_isaf_and_blocks_equal_the_rule_bit_for_bit_on_exact_cohorts(P, vp, n):
    rng = np.random.default_rng(7000 + n)
    with P.PcoaEngine(n, grm=True) as eng:
        for k, (vu, vx) in enumerate(EXACT_V):
            for ref_is_a1 in ((False, True) if (vu, vx) == (64, 2) else (bool((k + n) & 1),)):
                codes, basis, hat = exact_fit_cohort(rng, n, vu, vx, ref_is_a1)
                v = vu + vx
                eng.reset()
                fill(eng, codes, ref_is_a1)
                assert eng.grm_info()[:2] == (v, vu)
                eng.grm_pcrelate_fit(basis, hat)
                want_beta = vp.grm_pcrelate_beta_rule(codes, ref_is_a1, hat)
                beta = eng.grm_pcrelate_beta()
                assert same_bits(beta, want_beta), (n, vu, vx)
                hom = 3 if ref_is_a1 else 0
                g1 = (codes[:, 1] == 2) + 2.0 * (codes[:, 1] == hom)
                used = np.array([(codes[r] == hom).sum() == (codes[r] == (3 - hom)).sum() > 0 for r in range(v)])
                assert np.all(beta[used, 0] == 1.0) and np.array_equal(beta[used, 1], g1[used])
                want_mu = vp.grm_pcrelate_isaf_rule(beta, basis)
                assert same_bits(eng.grm_pcrelate_isaf(0, v), want_mu)
                assert set(np.unique(want_mu[used])) <= {-0.5, 0.0, 0.5, 1.0, 1.5}
                want_phi, want_n, num, den = vp.grm_pcrelate_rule(codes, ref_is_a1, beta, basis, 0.01)
                assert np.array_equal(num, np.rint(num)) and np.array_equal(den, want_n / 4.0)
                assert len(set(np.diagonal(want_n).tolist())) > 1 or vu < 8       # the masks differ per sample
                for q, (r0, r, c0, c) in enumerate(rectangles(n)):
                    got_phi, got_n = block(eng, (r0, r, c0, c), 0.01, device=bool((q + k) & 1))
                    where = (n, vu, vx, ref_is_a1, (r0, r, c0, c))
                    assert same_bits(got_n, want_n[r0:r0 + r, c0:c0 + c].astype(np.int32)), where
                    assert same_bits(got_phi, np.ascontiguousarray(want_phi[r0:r0 + r, c0:c0 + c])), where
                assert eng.grm_pcrelate_stats()["grm_pcrelate_n_cov"] == 2
                if (vu, vx) in ((4, 3), (64, 2)):
                    # the padded instantiations: zero rows change no bit
                    for n_cov in (3, 5, 9):
                        eng.grm_pcrelate_fit(padded(basis, n_cov), padded(hat, n_cov))
                        got_phi, got_n = block(eng, (0, n, 0, n), 0.01)
                        assert same_bits(got_phi, want_phi) and same_bits(got_n, want_n.astype(np.int32)), (n, vu, n_cov)
                        assert same_bits(eng.grm_pcrelate_isaf(0, v), want_mu)
                    # one covariate: mu = 0.5 everywhere, the mask is used and called
                    eng.grm_pcrelate_fit(basis[:1], hat[:1])
                    b1 = eng.grm_pcrelate_beta()
                    assert b1.shape == (v, 1) and same_bits(b1, np.ascontiguousarray(want_beta[:, :1]))
                    w1 = vp.grm_pcrelate_rule(codes, ref_is_a1, b1, basis[:1], 0.01)
                    got_phi, got_n = block(eng, (0, n, 0, n), 0.01, device=True)
                    assert same_bits(got_phi, w1[0]) and same_bits(got_n, w1[1].astype(np.int32))
                    assert np.array_equal(w1[1], vp.grm_dense_rule(codes, ref_is_a1)[1])


# ---- 2. segments ------------------------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(tests)r)
from conftest import load_pkg
from test_gpu_grm_pcrelate import exact_fit_cohort
from test_grm_cpu import pack_bed
P = load_pkg()
vp = load_pkg("variants_pca")
rng = np.random.default_rng(65)
n = 65
with P.PcoaEngine(n, grm=True) as eng:
    for vu, vx in ((64, 31), (64, 32), (64, 33), (128, 72)):
        codes, basis, hat = exact_fit_cohort(rng, n, vu, vx, False)
        rows = pack_bed(codes)
        eng.reset()
        cuts = [0] + sorted(set(int(c) for c in rng.integers(1, vu + vx, size=4))) + [vu + vx]
        for a, b in zip(cuts[:-1], cuts[1:]):
            eng.accumulate_plink_bed(np.ascontiguousarray(rows[a:b]))
        info = eng.grm_info()
        assert info[:2] == (vu + vx, vu) and info[2] == -(-(vu + vx) // 96) * 96 * 32, info   # segments of 96 rows of 32 bytes
        eng.grm_pcrelate_fit(basis, hat)
        beta = eng.grm_pcrelate_beta()
        assert beta.tobytes() == vp.grm_pcrelate_beta_rule(codes, False, hat).tobytes()
        assert eng.grm_pcrelate_isaf(3, vu + vx - 3).tobytes() == vp.grm_pcrelate_isaf_rule(beta, basis)[3:].tobytes()
        want_phi, want_n, _, _ = vp.grm_pcrelate_rule(codes, False, beta, basis, 0.01)
        for rect in ((0, n, 0, n), (17, 30, 3, 45), (n - 1, 1, 0, n)):
            r0, r, c0, c = rect
            for device in (False, True):
                k, m = eng.grm_pcrelate_block(r0, r, c0, c, 0.01, pairs=True, device=device)
                if device:
                    k, m = k.cpu().numpy(), m.cpu().numpy()
                assert k.tobytes() == np.ascontiguousarray(want_phi[r0:r0 + r, c0:c0 + c]).tobytes(), (vu, vx, rect)
                assert np.array_equal(m, want_n[r0:r0 + r, c0:c0 + c]), (vu, vx, rect)
        pairs, found = eng.grm_pcrelate_pairs(0.1, 0.01, band_rows=64)
        assert pairs.tobytes() == vp.grm_pairs_rule(want_phi, 0.1, want_n).tobytes() and found == pairs.size
print("SEGMENTS-OK")
"""


def test_fit_and_blocks_across_segment_boundaries():
    """V = 95, 96, 97 and 200 at N = 65 with segments of 96 rows, fed in ragged calls (the knob is read once per process)."""
    env = dict(os.environ)
    env["PCOA_GRM_SEGMENT_ROWS"] = "96"
    res = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests")}], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0 and "SEGMENTS-OK" in res.stdout, res.stdout[-3000:]


# ---- 3. rounded cohorts -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rounded():
    rng = np.random.default_rng(2600)
    return {"bn": balding_nichols(rng, 260, 1000), "edge": edge_rows(random_codes(rng, 300, 130))}


def orthonormal_covariates(rng, n, n_cov):
    """[n_cov][n]: an orthonormal basis of span{1, n_cov - 1 random vectors}, the first row along the ones"""
    m = rng.standard_normal((n, n_cov))
    m[:, 0] = 1.0
    q, r = np.linalg.qr(m)
    return np.ascontiguousarray((q * np.sign(np.diagonal(r))[None, :]).T)


def phi_bound(v, a, b, num, den, phi):
    """What separates two evaluations of phi(i, j) that share their operands bit for bit and differ in the order of the V
    additions: each sum of V terms carries at most (V - 1) 2^-53 sum|term|, so two orders differ by at most
    g_x = (V + 16) 2^-52 sum_v |x_i x_j| (the 16 leaves room for the products' own roundings being added in other places of
    the tree).  phi = num / (4 den) then moves by at most (g_num + 4 |phi| g_den) / (4 (den - g_den)) plus the roundings of
    the product 4 den (exact), the division and its operand errors' second order: 4 * 2^-52 |phi|."""
    gam = (v + 16) * U
    g_num = gam * (np.abs(a).T @ np.abs(a))
    g_den = gam * (b.T @ b)
    lo = np.maximum(den - g_den, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(lo > 0, (g_num + 4.0 * np.abs(phi) * g_den) / (4.0 * lo), 0.0) + 4.0 * U * np.abs(phi)
    return out


def operands(vp, codes, beta, basis, t):
    mu = vp.grm_pcrelate_isaf_rule(beta, basis)
    c = codes != 1
    g = (codes == 2) + 2.0 * (codes == 0)
    nv = c.sum(axis=1)
    av = g.sum(axis=1)
    used = (nv > 0) & (av > 0) & (av < 2 * nv)
    m = used[:, None] & c & (mu > t) & (mu < 1.0 - t)
    a = np.where(m, g - (mu + mu), 0.0)
    b = np.where(m, np.sqrt(np.where(m, mu * (1.0 - mu), 0.0)), 0.0)
    return a, b


def tiled(eng, n, t, bh, bw, r_first=0, c_first=0):
    out = np.full((n, n), np.nan)
    r_edges = ([0, r_first] if r_first else [0]) + list(range((r_first or 0) + bh, n, bh)) + [n]
    c_edges = ([0, c_first] if c_first else [0]) + list(range((c_first or 0) + bw, n, bw)) + [n]
    for ra, rb in zip(r_edges[:-1], r_edges[1:]):
        for ca, cb in zip(c_edges[:-1], c_edges[1:]):
            out[ra:rb, ca:cb] = eng.grm_pcrelate_block(ra, rb - ra, ca, cb - ca, t)
    return out


@pytest.mark.parametrize("n_cov", [1, 3, 9])
@pytest.mark.parametrize("name", ["bn", "edge"])
def test_fit_read_out_symmetry_cuts_and_accuracy_on_rounded_cohorts(P, vp, rounded, name, n_cov):
    codes = rounded[name]
    v, n = codes.shape
    rng = np.random.default_rng(31 * n_cov + n)
    basis = orthonormal_covariates(rng, n, n_cov)
    hat = P.pcrelate_hat(basis)
    assert same_bits(hat, vp.pcrelate_hat_rule(basis))
    t = 0.01
    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(n, grm=True) as other:
        fill(eng, codes)
        fill(other, codes, cuts=[1, 7, 130, 131])
        eng.grm_pcrelate_fit(basis)                               # hat=None: the helper
        other.grm_pcrelate_fit(basis, hat)
        beta = eng.grm_pcrelate_beta()
        assert same_bits(other.grm_pcrelate_beta(), beta)
        assert same_bits(eng.grm_pcrelate_beta(5, 17), np.ascontiguousarray(beta[5:22]))
        want_beta = vp.grm_pcrelate_beta_rule(codes, False, hat)
        tol = (n + 16) * U * 2.0 * np.abs(hat).sum(axis=1)        # dosages are at most 2
        err = np.abs(beta - want_beta)
        print("%s n_cov %d: beta error / bound %.3g" % (name, n_cov, float((err / tol[None, :]).max())))
        assert np.all(err <= tol[None, :])
        want_mu = vp.grm_pcrelate_isaf_rule(beta, basis)
        assert same_bits(eng.grm_pcrelate_isaf(0, v), want_mu)
        assert same_bits(eng.grm_pcrelate_isaf(v - 3, 3), np.ascontiguousarray(want_mu[v - 3:]))
        want_phi, want_n, num, den = vp.grm_pcrelate_rule(codes, False, beta, basis, t)
        phi, cnt = block(eng, (0, n, 0, n), t)
        assert np.array_equal(cnt, want_n)
        assert same_bits(phi, np.ascontiguousarray(phi.T))                                  # exact symmetry
        assert same_bits(block(eng, (0, n, 0, n), t, device=True)[0], phi)                  # two runs, either pointer kind
        assert same_bits(tiled(eng, n, t, 64, 64), phi)
        assert same_bits(tiled(eng, n, t, 50, 70, r_first=7, c_first=13), phi)              # blocks at odd offsets
        assert same_bits(block(other, (0, n, 0, n), t)[0], phi)                             # other accumulate call sizes
        assert same_bits(eng.grm_pcrelate_dense(t, block=100), phi)
        a, b = operands(vp, codes, beta, basis, t)
        bound = phi_bound(v, a, b, num, den, want_phi)
        err = np.abs(phi - want_phi)
        share = float((err[bound > 0] / bound[bound > 0]).max())
        print("%s n_cov %d: largest share of the phi bound %.3g" % (name, n_cov, share))
        assert np.all(err <= bound), share
        if name == "edge":   # sample 1 is never called
            assert not phi[1].any() and not phi[:, 1].any() and not cnt[1].any()
        # the threshold and min_maf enter as the rule says; the fit does not move
        w2 = vp.grm_pcrelate_rule(codes, False, beta, basis, 0.1)
        phi2, cnt2 = block(eng, (0, n, 0, n), 0.1)
        a2, b2 = operands(vp, codes, beta, basis, 0.1)
        assert np.array_equal(cnt2, w2[1]) and np.all(np.abs(phi2 - w2[0]) <= phi_bound(v, a2, b2, w2[2], w2[3], w2[0]))
        assert (cnt2 <= cnt).all() and (cnt2 < cnt).any()
        eng.grm_set_min_maf(0.2)
        w3 = vp.grm_pcrelate_rule(codes, False, beta, basis, t, min_maf=0.2)
        phi3, cnt3 = block(eng, (0, n, 0, n), t)
        assert np.array_equal(cnt3, w3[1]) and (cnt3 <= cnt).all() and (cnt3 < cnt).any()
        assert same_bits(eng.grm_pcrelate_beta(), beta)
        eng.grm_set_min_maf(0.0)
        assert same_bits(block(eng, (0, n, 0, n), t)[0], phi)
        # the screen: the rule on the very bits of the block call, whatever the band
        cutoff = float(np.sort(phi[np.triu_indices(n, 1)])[-40])
        want_pairs = vp.grm_pairs_rule(phi, cutoff, cnt)
        assert want_pairs.size >= 40
        for band in (0, 64, 128):
            pairs, found, diag = eng.grm_pcrelate_pairs(cutoff, t, band_rows=band, diag=True)
            assert found == want_pairs.size and pairs.tobytes() == want_pairs.tobytes(), band
            assert same_bits(diag, np.ascontiguousarray(np.diagonal(phi)))
        pairs, found = eng.grm_pcrelate_pairs(cutoff, t, capacity=7)
        assert found == want_pairs.size and pairs.tobytes() == want_pairs[:7].tobytes()
        pairs, found = eng.grm_pcrelate_pairs(cutoff, t, capacity=0)
        assert found == want_pairs.size and pairs.size == 0


@pytest.mark.parametrize("n", [32, 33, 1025])
def test_the_read_out_at_five_rows_and_any_hat(P, vp, n):
    """hat need not be a pseudo-inverse: any finite matrix is a fit, and the read-out is the rule on the device's beta"""
    rng = np.random.default_rng(n)
    codes = random_codes(rng, 5, n)
    for n_cov in (2, 9):
        basis, hat = rng.standard_normal((n_cov, n)), rng.standard_normal((n_cov, n)) / n
        with P.PcoaEngine(n, grm=True) as eng:
            fill(eng, codes)
            eng.grm_pcrelate_fit(basis, hat)
            beta = eng.grm_pcrelate_beta()
            want = vp.grm_pcrelate_beta_rule(codes, False, hat)
            assert np.all(np.abs(beta - want) <= (n + 16) * U * 2.0 * np.abs(hat).sum(axis=1)[None, :])
            assert same_bits(eng.grm_pcrelate_isaf(0, 5), vp.grm_pcrelate_isaf_rule(beta, basis))
            assert same_bits(eng.grm_pcrelate_isaf(2, 2), np.ascontiguousarray(vp.grm_pcrelate_isaf_rule(beta, basis)[2:4]))


# ---- 4. the admixed cohort --------------------------------------------------------------------------------------------------
def test_the_screen_finds_the_planted_relatives_of_the_admixed_cohort(P, vp):
    n, v, seed = C.SIZES[0]
    code = C.codes(n, v, seed)
    basis = C.covariates(vp, code)
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, code)
        eng.grm_pcrelate_fit(basis)
        pairs, found, diag = eng.grm_pcrelate_pairs(C.CUTOFF, C.THRESHOLD, diag=True)
        phi = eng.grm_pcrelate_dense(C.THRESHOLD)
    assert found == pairs.size and [(int(p["i"]), int(p["j"])) for p in pairs] == C.planted_pairs()
    lo, other = C.extremes(phi)
    print("admixed cohort on the device: smallest planted phi %.4f, largest other %.4f" % (lo, other))
    assert (round(lo, 3), round(other, 3)) == C.KNOWN[(n, v)]["phi"]
    assert np.all(np.abs(2.0 * diag - 1.0) < 0.2)                      # inbreeding coefficients of an outbred cohort


# ---- 5. state ---------------------------------------------------------------------------------------------------------------
def test_refusals_state_and_statistics(P, vp):
    import torch
    L = P._lib
    lib = L.load()
    n, v = 130, 300
    rng = np.random.default_rng(61)
    codes = random_codes(rng, v, n)
    basis = orthonormal_covariates(rng, n, 3)
    hat = P.pcrelate_hat(basis)
    x = torch.from_numpy(rng.standard_normal(n)).cuda()
    cvp = ctypes.c_void_p
    out = np.zeros((n, n))
    found = ctypes.c_int64(0)
    ptr = lambda a: cvp(a.ctypes.data)

    for rc in (lib.pcoa_grm_pcrelate_fit(None, 3, ptr(basis), ptr(hat)), lib.pcoa_grm_pcrelate_beta(None, 0, 1, ptr(out)),
               lib.pcoa_grm_pcrelate_isaf(None, 0, 1, ptr(out)), lib.pcoa_grm_pcrelate_block(None, 0, 1, 0, 1, 0.01, ptr(out), None, 0),
               lib.pcoa_grm_pcrelate_pairs(None, 0.1, 0.01, 0, None, 0, ctypes.byref(found), None)):
        assert rc == L.PCOA_ERR_INVALID_ARG and b"pcoa_grm_pcrelate" in lib.pcoa_last_error(None)
    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(n) as full, P.PcoaEngine(n, operator=True) as op, \
            P.PcoaEngine(n, grm_study=True) as study:
        def refused(code, word, fn, *args):
            with pytest.raises(P.PcoaError) as ei:
                fn(*args)
            assert ei.value.code == code and word in str(ei.value), str(ei.value)

        # an empty store, and no fit yet
        refused(L.PCOA_ERR_STATE, "empty", eng.grm_pcrelate_fit, basis, hat)
        fill(eng, codes)
        fill(study, codes)
        for fn, args in ((eng.grm_pcrelate_beta, (0, 1)), (eng.grm_pcrelate_isaf, (0, 1)), (eng.grm_pcrelate_block, (0, 1, 0, 1)),
                         (eng.grm_pcrelate_pairs, (0.1,))):
            refused(L.PCOA_ERR_STATE, "no fit", fn, *args)
        # a ctx without a fit and one with it answer the existing calls with the same bits
        k0, y0, c0 = eng.grm_block(0, n, 0, n), eng.grm_matvec_device(x).cpu().numpy(), eng.compute(2)
        g0 = eng.grm_pairs(0.05)
        eng.reset_timings()
        # the fit's refusals
        for other, word in ((full, "full engine"), (op, "operator"), (study, "no weights of its own")):
            refused(L.PCOA_ERR_STATE, word, other.grm_pcrelate_fit, basis, hat)
        bad = basis.copy()
        bad[1, 5] = np.nan
        refused(L.PCOA_ERR_INVALID_ARG, "basis[1][5]", eng.grm_pcrelate_fit, bad, hat)
        bad = hat.copy()
        bad[2, 7] = np.inf
        refused(L.PCOA_ERR_INVALID_ARG, "hat[2][7]", eng.grm_pcrelate_fit, basis, bad)
        assert lib.pcoa_grm_pcrelate_fit(eng._ctx, 0, ptr(basis), ptr(hat)) == L.PCOA_ERR_INVALID_ARG
        assert lib.pcoa_grm_pcrelate_fit(eng._ctx, 10, ptr(basis), ptr(hat)) == L.PCOA_ERR_INVALID_ARG
        assert b"n_cov = 10" in lib.pcoa_last_error(eng._ctx)
        assert lib.pcoa_grm_pcrelate_fit(eng._ctx, 3, None, ptr(hat)) == L.PCOA_ERR_INVALID_ARG
        assert lib.pcoa_grm_pcrelate_fit(eng._ctx, 3, ptr(basis), None) == L.PCOA_ERR_INVALID_ARG
        assert eng.grm_pcrelate_stats()["grm_pcrelate_fits"] == 0
        eng.grm_pcrelate_fit(basis, hat)
        beta = eng.grm_pcrelate_beta()
        # windows, rectangles, thresholds, the pairs call's arguments
        for first, cnt in ((-1, 1), (0, v + 1), (v, 1), (5, -1)):
            assert lib.pcoa_grm_pcrelate_beta(eng._ctx, first, cnt, ptr(out)) == L.PCOA_ERR_INVALID_ARG
            assert lib.pcoa_grm_pcrelate_isaf(eng._ctx, first, cnt, ptr(out)) == L.PCOA_ERR_INVALID_ARG
            assert b"pcoa_grm_pcrelate_isaf" in lib.pcoa_last_error(eng._ctx)
        assert lib.pcoa_grm_pcrelate_beta(eng._ctx, 0, 1, None) == L.PCOA_ERR_INVALID_ARG
        assert lib.pcoa_grm_pcrelate_isaf(eng._ctx, 0, 1, None) == L.PCOA_ERR_INVALID_ARG
        for args in ((0, 0, 0, 1), (0, 1, 0, -1), (-1, 2, 0, 1), (0, n + 1, 0, 1), (n - 1, 2, 0, 1), (0, 1, 5, n - 4)):
            assert lib.pcoa_grm_pcrelate_block(eng._ctx, *args, 0.01, ptr(out), None, 0) == L.PCOA_ERR_INVALID_ARG, args
            assert b"pcoa_grm_pcrelate_block" in lib.pcoa_last_error(eng._ctx)
        assert lib.pcoa_grm_pcrelate_block(eng._ctx, 0, 1, 0, 1, 0.01, None, None, 0) == L.PCOA_ERR_INVALID_ARG
        assert b"NULL" in lib.pcoa_last_error(eng._ctx)
        for t in (-0.01, 0.5, float("nan"), float("inf")):
            refused(L.PCOA_ERR_INVALID_ARG, "maf_threshold", eng.grm_pcrelate_block, 0, 1, 0, 1, t)
            refused(L.PCOA_ERR_INVALID_ARG, "maf_threshold", eng.grm_pcrelate_pairs, 0.1, t)
        refused(L.PCOA_ERR_INVALID_ARG, "cutoff", eng.grm_pcrelate_pairs, float("nan"))
        refused(L.PCOA_ERR_INVALID_ARG, "band_rows", eng.grm_pcrelate_pairs, 0.1, 0.01, 65)
        refused(L.PCOA_ERR_INVALID_ARG, "band_rows", eng.grm_pcrelate_pairs, 0.1, 0.01, -64)
        refused(L.PCOA_ERR_INVALID_ARG, "capacity", eng.grm_pcrelate_pairs, 0.1, 0.01, 0, -1)
        assert lib.pcoa_grm_pcrelate_pairs(eng._ctx, 0.1, 0.01, 0, None, 5, ctypes.byref(found), None) == L.PCOA_ERR_INVALID_ARG
        assert lib.pcoa_grm_pcrelate_pairs(eng._ctx, 0.1, 0.01, 0, None, 0, None, None) == L.PCOA_ERR_INVALID_ARG
        for other, word in ((full, "full engine"), (op, "operator"), (study, "no weights of its own")):
            refused(L.PCOA_ERR_STATE, word, other.grm_pcrelate_block, 0, 1, 0, 1)
            refused(L.PCOA_ERR_STATE, word, other.grm_pcrelate_pairs, 0.1)
        # statistics
        st = eng.grm_pcrelate_stats()
        assert st["grm_pcrelate_fits"] == 1 and st["grm_pcrelate_block_calls"] == 0 and st["grm_pcrelate_fit_seconds"] > 0
        eng.grm_pcrelate_block(3, 40, 0, 50)
        eng.grm_pcrelate_block(3, 40, 0, 50, pairs=True)
        eng.grm_pcrelate_pairs(0.1, band_rows=64)
        st = eng.grm_pcrelate_stats()
        band_flops = sum(2.0 * min(64, n - r0) * (192 - r0 // 64 * 64) * v * 3 for r0 in range(0, n, 64))
        assert st["grm_pcrelate_block_calls"] == 2 and st["grm_pcrelate_pairs_calls"] == 1 and st["grm_pcrelate_bands"] == 3
        assert st["grm_pcrelate_flops"] == 2.0 * 40 * 50 * v * 5 + band_flops
        assert st["grm_pcrelate_dense_seconds"] > 0 and st["grm_pcrelate_screen_seconds"] > 0 and st["grm_pcrelate_bytes"] > 0
        # nothing of the ctx moved
        assert same_bits(eng.grm_block(0, n, 0, n), k0) and same_bits(eng.grm_matvec_device(x).cpu().numpy(), y0)
        c1 = eng.compute(2)
        assert same_bits(c1[0], c0[0]) and same_bits(c1[1], c0[1]) and c1[2] == c0[2]
        g1 = eng.grm_pairs(0.05)
        assert g1[0].tobytes() == g0[0].tobytes() and g1[1] == g0[1]
        # a subset does not inherit the fit
        with eng.grm_subset(np.arange(0, n, 2)) as sub:
            refused(L.PCOA_ERR_STATE, "no fit", sub.grm_pcrelate_block, 0, 1, 0, 1)
        phi = eng.grm_pcrelate_block(0, n, 0, n)
        # an append drops the fit and says so; a second fit replaces it; reset drops it and says so
        eng.accumulate_plink_bed(np.ascontiguousarray(np.zeros((1, (n + 3) // 4), dtype=np.uint8)))
        refused(L.PCOA_ERR_STATE, "pcoa_accumulate_plink_bed", eng.grm_pcrelate_block, 0, 1, 0, 1)
        refused(L.PCOA_ERR_STATE, "pcoa_accumulate_plink_bed", eng.grm_pcrelate_beta, 0, 1)
        eng.grm_pcrelate_fit(basis[:2], hat[:2])
        assert eng.grm_pcrelate_beta().shape == (v + 1, 2)
        eng.reset()
        refused(L.PCOA_ERR_STATE, "pcoa_reset", eng.grm_pcrelate_pairs, 0.1)
        # M' = 0
        eng.accumulate_plink_bed(np.ascontiguousarray(np.full((5, (n + 3) // 4), 0xFF, dtype=np.uint8)))
        eng.grm_pcrelate_fit(basis, hat)
        refused(L.PCOA_ERR_STATE, "M' = 0", eng.grm_pcrelate_block, 0, 1, 0, 1)
        refused(L.PCOA_ERR_STATE, "M' = 0", eng.grm_pcrelate_pairs, 0.1)
        assert eng.grm_pcrelate_beta().shape == (5, 3)                   # the fit itself is defined for every row
        eng.reset()
        fill(eng, codes)
        eng.grm_pcrelate_fit(basis, hat)
        assert same_bits(eng.grm_pcrelate_beta(), beta) and same_bits(eng.grm_pcrelate_block(0, n, 0, n), phi)
        assert same_bits(eng.grm_matvec_device(x).cpu().numpy(), y0)


# ---- 6. hosts ---------------------------------------------------------------------------------------------------------------
def test_both_hosts_write_the_same_files_and_find_the_planted_relatives(P, vp, tmp_path):
    """--grm-pcrelate-output-path in both hosts, on the admixed cohort as a PLINK fileset: over the whole cohort on the final
    engine, and as the step behind PC-AiR -- the six children listed out, placed by --grm-project-removed, the cohort's engine a
    panel subset of the whole fileset's -- where the planted relatives come out and nobody else."""
    from king_cohort import write_plink
    from test_grm_cpu import _run_driver, _run_python
    n, v, seed = C.SIZES[0]
    code = C.codes(n, v, seed)
    names = ["S%04d" % i for i in range(n)]
    prefix = str(tmp_path / "admixed")
    write_plink(code, prefix, names)
    listed = str(tmp_path / "children.txt")
    with open(listed, "w") as f:
        f.write("".join("%s\n" % names[i] for i in C.PLACED))
    x = vp.java_double_to_string(C.CUTOFF)
    runs = {}
    for tag, run in (("cpp", _run_driver), ("py", _run_python)):
        plain = run(["--input-path", prefix + ".bed", "--grm"])
        assert plain.returncode == 0 and "GRM PC-Relate" not in plain.stderr, plain.stderr[-2000:]
        for case, extra in (("all", []), ("pcair", ["--grm-remove-samples", listed, "--grm-project-removed"])):
            pairs_path, inb_path = str(tmp_path / ("%s_%s_pairs.tsv" % (tag, case))), str(tmp_path / ("%s_%s_f.tsv" % (tag, case)))
            res = run(["--input-path", prefix + ".bed", "--grm"] + extra +
                      ["--grm-pcrelate-output-path", pairs_path, "--grm-pcrelate-cutoff", repr(C.CUTOFF),
                       "--grm-pcrelate-inbreeding-output-path", inb_path])
            assert res.returncode == 0, res.stderr[-2000:]
            if case == "all":
                assert res.stdout == plain.stdout                                  # the coordinates do not move
            line = [ln for ln in res.stderr.splitlines() if ln.startswith("GRM PC-Relate: ")]
            assert len(line) == 1 and (" pair(s) with kinship >= %s among %d sample(s), 2 axes, " % (x, n)) in line[0], res.stderr[-2000:]
            assert line[0].endswith(" used variant(s), threshold 0.01")
            runs[tag, case] = (open(pairs_path, "rb").read(), open(inb_path, "rb").read(), line[0], res.stdout)
    for case in ("all", "pcair"):
        assert runs["cpp", case] == runs["py", case], case
    # behind PC-AiR: the planted relatives and nobody else, in (i, j) order
    rows = runs["cpp", "pcair"][0].decode().splitlines()
    assert rows[0] == "name_i\tname_j\tkinship\tn"
    assert [tuple(r.split("\t")[:2]) for r in rows[1:]] == [(names[a], names[b]) for a, b in C.planted_pairs()]
    assert runs["cpp", "pcair"][2].startswith("GRM PC-Relate: %d pair(s)" % len(C.planted_pairs()))
    frows = runs["cpp", "pcair"][1].decode().splitlines()
    assert frows[0] == "name\tf\tn" and [r.split("\t")[0] for r in frows[1:]] == names
    assert all(abs(float(r.split("\t")[1])) < 0.2 and 0 < int(r.split("\t")[2]) <= v for r in frows[1:])
    # over the whole cohort: the engine's own answer through the Python API, byte for byte
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, code)
        comps, _, _ = eng.compute(2)
        basis = np.ascontiguousarray(np.vstack([np.ones((1, n)), comps[:, :2].T]))
        eng.grm_pcrelate_fit(basis)
        pairs, found, diag = eng.grm_pcrelate_pairs(C.CUTOFF, 0.01, diag=True)
        n_diag = np.diagonal(eng.grm_pcrelate_block(0, n, 0, n, 0.01, pairs=True)[1])
    vp.write_pcrelate_pairs(str(tmp_path / "api_pairs.tsv"), pairs, names)
    vp.write_pcrelate_inbreeding(str(tmp_path / "api_f.tsv"), names, diag, n_diag)
    assert open(str(tmp_path / "api_pairs.tsv"), "rb").read() == runs["cpp", "all"][0]
    assert open(str(tmp_path / "api_f.tsv"), "rb").read() == runs["cpp", "all"][1]

"""The cohort of the PC-Relate tests (test_grm_pcrelate_cpu.py, test_gpu_grm_pcrelate.py): an ADMIXED cohort -- every sample draws
its alleles from two ancestral populations at a share alpha_i ~ Beta(0.5, 0.5) of its own -- with six children planted into it, two
of them with parents of different ancestry and one a grandchild.  K / 2 inflates every pair that shares ancestry and KING-robust
deflates relatives whose ancestry differs, so neither separates the 17 planted pairs (second degree and closer) from the rest at
(260, 6000); PC-Relate kinship on two axes does, by a margin.  A fixture that does not discriminate fails loudly instead of
testing nothing."""
import numpy as np

FST = 0.2
SIZES = [(130, 6000, 1), (260, 6000, 2)]      # (n, v, seed)
CUTOFF = 2.0 ** -3.5                           # between second (1 / 8) and third (1 / 16) degree
MIN_MARGIN = 0.05                              # every pair's phi / CUTOFF stays at least this far from 1, or the fixture is invalid
NUM_PC = 2
THRESHOLD = 0.01
CHILDREN = [(20, 0, 1), (21, 0, 1), (22, 2, 3), (23, 2, 4), (24, 20, 5), (25, 6, 7)]    # (child, parent, parent), in this order
PLACED = [c for c, _, _ in CHILDREN]           # not in the reference set of the axes: placed by the projection formula
FIRST_DEGREE = [(0, 20), (1, 20), (0, 21), (1, 21), (20, 21), (2, 22), (3, 22), (2, 23), (4, 23), (20, 24), (5, 24), (6, 25), (7, 25)]
SECOND_DEGREE = [(22, 23), (0, 24), (1, 24), (21, 24)]
CODE_OF_DOSAGE = np.array([3, 2, 0], dtype=np.uint8)   # copies of A1 -> .bed code: A2 is the reference (ref_is_a1 = False)
# (smallest planted value, largest other value) to three decimals, per (n, v): PC-Relate phi, K / 2, KING-robust kinship
KNOWN = {
    (130, 6000): {"phi": (0.098, 0.040), "k_half": (0.092, 0.105), "king": (0.113, 0.066)},
    (260, 6000): {"phi": (0.105, 0.033), "k_half": (0.073, 0.114), "king": (0.055, 0.080)},
}


def planted_pairs():
    return sorted(FIRST_DEGREE + SECOND_DEGREE)


def codes(n, v, seed):
    """uint8 [v][n] of PLINK .bed codes (0 hom A1, 1 missing, 2 het, 3 hom A2); KNOWN depends on the order of the
    RNG calls below."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, size=v)
    f = rng.beta(p[:, None] * (1 - FST) / FST, (1 - p[:, None]) * (1 - FST) / FST, size=(v, 2))
    alpha = rng.beta(0.5, 0.5, size=n)
    hap = rng.random((2, v, n)) < (f[:, 0:1] * alpha[None, :] + f[:, 1:2] * (1.0 - alpha[None, :]))[None, :, :]
    for child, pa, pb in CHILDREN:
        for k, parent in enumerate((pa, pb)):
            pick = rng.integers(0, 2, v)
            hap[k, :, child] = np.where(pick == 0, hap[0, :, parent], hap[1, :, parent])
    code = CODE_OF_DOSAGE[hap[0].astype(np.int64) + hap[1]]
    rate = rng.uniform(0.0, 0.1, size=n)
    code[rng.random((v, n)) < rate[None, :]] = 1
    return code


def covariates(vp, code, num_pc=NUM_PC):
    """basis [1 + num_pc][n]: a row of ones, then the leading axes of the dense K of the samples other than PLACED (u_c, from
    numpy's eigh) with the PLACED samples at coord(q, c) = sum_v c_vq (g_vq - mu_v) t_vc / M' / lambda_c, t_c = D A u_c: the
    mean-imputed projection of pcoa_grm_project."""
    v, n = code.shape
    ref = np.array([i for i in range(n) if i not in PLACED])
    k, _ = vp.grm_dense_rule(code[:, ref], False, 0.0, "used")
    w, vec = np.linalg.eigh(k)
    lam, u = w[::-1][:num_pc], vec[:, ::-1][:, :num_pc]
    c = code[:, ref] != 1
    g = (code[:, ref] == 2) + 2.0 * (code[:, ref] == 0)
    nv, av = c.sum(axis=1), g.sum(axis=1)
    mu = np.where(nv > 0, av / np.maximum(nv, 1), 0.0)
    used = (nv > 0) & (av > 0) & (av < 2 * nv)
    d = np.where(used, 1.0 / np.where(used, mu * (1.0 - 0.5 * mu), 1.0), 0.0)
    t = d[:, None] * (np.where(c, g - mu[:, None], 0.0) @ u)                  # [v][num_pc]
    cq = code[:, PLACED] != 1
    gq = (code[:, PLACED] == 2) + 2.0 * (code[:, PLACED] == 0)
    coords = (np.where(cq, gq - mu[:, None], 0.0).T @ t) / float(used.sum()) / lam[None, :]
    basis = np.ones((1 + num_pc, n))
    basis[1:, ref] = u.T
    basis[1:, PLACED] = coords.T
    return basis


def phi_matrix(vp, code, num_pc=NUM_PC, t=THRESHOLD):
    """phi of the whole cohort by the numpy rules: covariates, their hat matrix, the fit, grm_pcrelate_rule."""
    basis = covariates(vp, code, num_pc)
    beta = vp.grm_pcrelate_beta_rule(code, False, vp.pcrelate_hat_rule(basis))
    return vp.grm_pcrelate_rule(code, False, beta, basis, t)[0]


def extremes(m):
    """(smallest planted entry, largest entry of any other pair i < j) of a symmetric matrix"""
    n = m.shape[0]
    planted = planted_pairs()
    lo = min(float(m[a, b]) for a, b in planted)
    rest = np.array(m, dtype=np.float64)
    rest[np.tril_indices(n)] = -np.inf
    for a, b in planted:
        rest[a, b] = -np.inf
    return lo, float(rest.max())


def margins(vp, code, cutoff=CUTOFF):
    """(smallest planted phi, largest phi of any other pair), after ASSERTING that every planted pair has phi / cutoff >=
    1 + MIN_MARGIN and every other pair <= 1 - MIN_MARGIN."""
    lo, other = extremes(phi_matrix(vp, code))
    assert lo / cutoff >= 1.0 + MIN_MARGIN, "fixture invalid: a planted pair at phi %.4f, cutoff %.4f" % (lo, cutoff)
    assert other / cutoff <= 1.0 - MIN_MARGIN, "fixture invalid: an unplanted pair at phi %.4f, cutoff %.4f" % (other, cutoff)
    return lo, other


def k_half_extremes(vp, code):
    """the same two numbers for K / 2 of the whole cohort (pcoa_grm_pairs' matrix as a kinship)"""
    return extremes(vp.grm_dense_rule(code, False, 0.0, "used")[0] / 2.0)


def king_extremes(vp, code):
    """and for the KING-robust kinship (hethet - 2 ibs0) / het_sum over all rows"""
    hethet, ibs0, het_sum = vp.grm_king_rule(code)
    return extremes(np.where(het_sum > 0, (hethet - 2 * ibs0) / np.maximum(het_sum, 1), 0.0))

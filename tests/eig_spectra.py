"""Integer similarity matrices S whose centred matrix B = J S J has a known spectrum, a high-precision reference for it, and
the checks that hold the dense eigensolver (csrc/eig.hip) and, with bars of its own (`lanczos_bars`), the Lanczos path
(csrc/eig_lanczos.hip) to that reference; and `integer_centred`, an S whose centred matrix is an integer matrix, the exact
reference of the centred mat-vec.  Test infrastructure: imported by tests only.

Every builder returns a Spectrum for the top k pairs of B, ranked by |lambda| with ties to the larger value (the order of
pcoa_compute and of MLlib).  Most families have the form

    S = c I + Y^T C Y        (Y a small V x N integer matrix, C a V x V integer matrix)

so that B = c J + Z^T C Z with Z = Y J.  The second term lies in range(J) and commutes with the first, so spec(B) is
{c + m_i} (the eigenvalues m_i of Z^T C Z on range(Z^T)), then c with multiplicity N - 1 - V, then 0 (the constant vector).
The m_i are those of R^T C R, where R R^T = Z Z^T = (N Y Y^T - r r^T) / N is an exact rational V x V matrix (r = Y 1); they
are solved in mpmath at DPS digits and their eigenvectors are Z^T R^-T b.  The `planted` family is referenced by LAPACK
(float64) on the oracle's B instead.
"""
import mpmath
import numpy as np

from conftest import int_gram, load_oracle, planted_callsets

DPS = 40             # mpmath digits of the reduced problems
REL_GAP = 1e-3       # eigenvalues of B closer than REL_GAP ||B||_2 form one cluster: its subspace is checked, not its vectors
EIG_BAR = 1e-11      # |lambda - lambda_ref| <= EIG_BAR ||B||_2 (+ the Weyl bound of a perturbed family)
RES_BAR = 1e-11      # ||B u - lambda u|| <= RES_BAR ||B||_2
ORTH_BAR = 1e-11     # max |U^T U - I|
VEC_BAR = 1e-8       # ||u - u_ref|| of an isolated eigenvalue (+ the Davis-Kahan bound of a perturbed family)
SUB_BAR = 1e-8       # ||U U^T - U_ref U_ref^T||_2 of a cluster returned whole


class Spectrum(object):
    """s: int64 S [N, N].  lam: the top-k eigenvalues of B (signed, ranked by |lambda|).  vecs: [N, k] reference vectors,
    NaN where only the eigenvalue is known (the bulk c, the null space); the columns of a cluster span its eigenspace.
    groups: (indices into the top k, whole) per cluster of the whole spectrum that the top k touch; whole = every
    eigenvalue of the cluster is among the top k.  norm: ||B||_2.  lam_tol: extra eigenvalue bar (Weyl bound; 0 = exact).
    vec_tol: [k] extra vector bars (Davis-Kahan; 0 = exact).  levels: [(value, multiplicity)] of the whole spectrum.
    gap: [k] distance of every selected eigenvalue to the nearest level outside its cluster (inf if there is none)."""

    def __init__(self, s, lam, vecs, groups, norm, levels, lam_tol=0.0, vec_tol=None, family="", gap=None):
        self.s, self.lam, self.vecs, self.groups, self.norm, self.levels = s, lam, vecs, groups, norm, levels
        self.gap = np.full(len(lam), np.inf) if gap is None else gap
        self.lam_tol = lam_tol
        self.vec_tol = np.zeros(len(lam)) if vec_tol is None else vec_tol
        self.family = family

    def top(self, k):
        """The same S with the reference for the top k pairs instead."""
        return _spectrum(self.s, self._levels, k, self.family, weyl=self.lam_tol)

    @property
    def n(self):
        return self.s.shape[0]

    @property
    def k(self):
        return len(self.lam)


# ------------------------------------------------------------------------------------------------- ranking and clusters
def _select(levels, k):
    """levels: [(value, multiplicity, basis [N, m] or None)] of the whole spectrum.  Returns the top-k eigenvalues, their
    vectors (NaN where the basis is unknown), the cluster groups and, per selected eigenvalue, the distance to the nearest
    level outside its cluster."""
    norm = max(abs(v) for v, _, _ in levels)
    scale = norm if norm > 0 else 1.0
    by_value = sorted(range(len(levels)), key=lambda i: levels[i][0])
    cluster = {}
    cid = 0
    for pos, i in enumerate(by_value):
        if pos > 0 and levels[i][0] - levels[by_value[pos - 1]][0] >= REL_GAP * scale:
            cid += 1
        cluster[i] = cid
    ranked = sorted(range(len(levels)), key=lambda i: (-abs(levels[i][0]), -levels[i][0]))
    n = next(b.shape[0] for _, _, b in levels if b is not None)
    lam, cols, owner, taken = [], [], [], {}
    for i in ranked:
        v, mult, basis = levels[i]
        for j in range(mult):
            if len(lam) == k:
                break
            lam.append(v)
            cols.append(basis[:, j] if basis is not None else np.full(n, np.nan))
            owner.append(i)
            taken[i] = taken.get(i, 0) + 1
    groups = []
    for c in sorted(set(cluster[i] for i in owner)):
        members = [t for t in range(k) if cluster[owner[t]] == c]
        whole = all(taken.get(i, 0) == levels[i][1] for i in cluster if cluster[i] == c)
        groups.append((members, whole))
    gap = np.array([min([abs(levels[owner[t]][0] - levels[j][0]) for j in cluster if cluster[j] != cluster[owner[t]]] or
                        [np.inf]) for t in range(k)])
    return np.array(lam), np.stack(cols, axis=1), groups, norm, gap


# ------------------------------------------------------------------------------------------------- reduced problems
def _reduced_pairs(y, cmat):
    """Eigenpairs of Z^T C Z on range(Z^T), Z = Y J: values [V] and unit vectors [N, V] (float64 of DPS-digit solves)."""
    y = np.asarray(y, dtype=np.int64)
    v, n = y.shape
    yi = [[int(t) for t in row] for row in y]
    r = [sum(row) for row in yi]
    yyt = y.astype(np.float64) @ y.T.astype(np.float64)            # exact: small integers, sums far below 2^53
    assert np.abs(yyt).max() < 2.0 ** 52
    with mpmath.workdps(DPS):
        g = mpmath.matrix(v, v)
        for a in range(v):
            for b in range(v):
                g[a, b] = mpmath.mpf(n * int(yyt[a, b]) - r[a] * r[b]) / n
        rl = mpmath.cholesky(g)
        cm = mpmath.matrix([[int(t) for t in row] for row in np.asarray(cmat, dtype=np.int64)])
        m = rl.T * cm * rl
        ev, q = mpmath.eigsy(m)
        rt = rl.T
        vals = np.array([float(ev[i]) for i in range(v)])
        coef = np.empty((v, v))
        for j in range(v):                                            # R^-T b for every eigenvector b
            a = mpmath.lu_solve(rt, q[:, j])
            coef[:, j] = [float(a[i]) for i in range(v)]
    u = y.T.astype(np.float64) @ coef
    u -= u.mean(axis=0)
    u /= np.linalg.norm(u, axis=0)
    return vals, u


def _low_rank_levels(y, cmat, c):
    """Levels of B = c J + Z^T C Z: c + m_i (vectors known), c (multiplicity N - 1 - V), 0 (the constant vector)."""
    v, n = np.asarray(y).shape
    vals, u = _reduced_pairs(y, cmat)
    levels = [(c + vals[i], 1, u[:, i:i + 1]) for i in range(v)]
    ones = np.full((n, 1), 1.0 / np.sqrt(n))
    if c == 0:
        levels.append((0.0, n - v, None))
    else:
        if n - 1 - v > 0:
            levels.append((float(c), n - 1 - v, None))
        levels.append((0.0, 1, ones))
    return levels


def _spectrum(s, levels, k, family, weyl=0.0):
    lam, vecs, groups, norm, gap = _select(levels, k)
    vec_tol = 2.0 * weyl / gap if weyl > 0 else None
    sp = Spectrum(s, lam, vecs, groups, norm, [(v, m) for v, m, _ in levels], lam_tol=weyl, vec_tol=vec_tol, family=family,
                  gap=gap)
    sp._levels = levels
    return sp


def genotypes(rng, v, n, pops=4):
    """[v, n] genotype-like values in {0, 1, 2} with population structure: samples in `pops` populations of unequal size, every
    variant with its own allele frequency per population."""
    bounds = np.sort(rng.choice(np.arange(1, n), size=pops - 1, replace=False)) if n > pops else np.arange(1, pops)
    pop = np.searchsorted(bounds, np.arange(n), side="right")
    f = rng.uniform(0.05, 0.95, size=(v, pops))
    return (rng.random((v, n)) < f[:, pop]).astype(np.int64) + (rng.random((v, n)) < f[:, pop]).astype(np.int64)


def _shifted_gram(x, c, sign=1, scale=1):
    s = int_gram(x) * (sign * scale)
    s[np.diag_indices_from(s)] += c * scale
    return s


# ------------------------------------------------------------------------------------------------- families
def planted(n, k, seed=0, v=None):
    """S = X^T X of planted carrier lists; reference: float64 LAPACK (scipy eigh, subset_by_index) on the oracle's B.
    Only for N <= 4,100 (about 1.5 s at N = 4,081 on 8 cores)."""
    import scipy.linalg
    assert n <= 4100
    rng = np.random.default_rng(1000 + n + 7 * seed)
    x = planted_callsets(rng, n, v or max(40, 3 * n // 2 if n < 100 else 600), k=4)
    s = int_gram(x)
    b = load_oracle().center_matrix(s)[0]
    lo = max(n - k - 1, 0)
    w, u = scipy.linalg.eigh(b, subset_by_index=[lo, n - 1], driver="evr")
    # B = J S J with S = X^T X is positive semidefinite: the largest |lambda| are the largest lambda.  Below the top k + 1
    # only an upper bound is known: one level of the remaining multiplicity at the (k+1)-th value stands for them.
    levels = [(float(w[i]), 1, u[:, i:i + 1]) for i in range(len(w))]
    if lo > 0:
        levels[0] = (float(w[0]), lo + 1, None)
    sp = _spectrum(s, levels, k, "planted")
    sp.b = b
    return sp


def shifted_low_rank(n, k, v=8, c=1000, seed=0, noise=False, scale=1):
    """S = c I + X^T X (times `scale`), X a [v, n] genotype matrix; c = 0 gives a rank-v B.  noise: + E + E^T with E in
    {-1, 0, 1} (a generic full-rank spectrum), referenced by the unperturbed spectrum with the Weyl bound
    1.1 ||E + E^T||_2 (power iteration) on the eigenvalues and the Davis-Kahan bound 2 ||E + E^T||_2 / gap on the vectors."""
    rng = np.random.default_rng(2000 + n + 13 * seed)
    x = genotypes(rng, v, n)
    s = _shifted_gram(x, c, scale=scale)
    levels = _low_rank_levels(x, np.eye(v, dtype=np.int64) * scale, c * scale)
    weyl = 0.0
    if noise:
        a = symmetric_noise(rng, n)
        weyl = 1.1 * norm_estimate(a)
        for r0 in range(0, n, 2048):
            s[r0:r0 + 2048] += a[r0:r0 + 2048].astype(np.int64)
        del a
    return _spectrum(s, levels, k, "shifted low rank" + (" + noise" if noise else "") + (" x%d" % scale if scale != 1 else ""),
                     weyl=weyl)


def negative_dominant(n, k, v=6, c=20, seed=0):
    """S = c I - X^T X: the eigenvalues c - m_i of largest |lambda| are negative."""
    rng = np.random.default_rng(3000 + n + 13 * seed)
    x = genotypes(rng, v, n)
    s = _shifted_gram(x, c, sign=-1)
    sp = _spectrum(s, _low_rank_levels(x, -np.eye(v, dtype=np.int64), c), k, "negative dominant")
    assert np.all(sp.lam < 0), sp.lam
    return sp


def block_constant(n, pops, within, across, c, bump=0):
    """S = c I + `_block_constant_similarity` (population 0 raised by `bump`), with the leftover samples (if any) as one more
    population whose within-value is `across`.  Equal populations give an eigenvalue of multiplicity len(pops) - 1 exactly;
    a small bump splits it into a near tie."""
    pops = list(pops)
    leftover = n - sum(pops)
    if leftover:
        pops.append(leftover)
    s, offs = _block_constant_similarity(n, pops, within, across, bump)
    d = [(within - across) + (bump if p == 0 else 0) for p in range(len(pops))]
    if leftover:
        s[offs[-2]:, offs[-2]:] = across
        d[-1] = 0
    s[np.diag_indices_from(s)] += c
    # J (sum_p d_p 1_p 1_p^T) J with the last indicator replaced by 1 - (the others): Y = the first P - 1 indicators,
    # C = diag(d_0 .. d_{P-2}) + d_{P-1} 1 1^T
    p = len(pops)
    y = np.zeros((p - 1, n), dtype=np.int64)
    for q in range(p - 1):
        y[q, offs[q]:offs[q + 1]] = 1
    cmat = np.diag(d[:p - 1]).astype(np.int64) + d[p - 1]
    return s, _low_rank_levels(y, cmat, c)


def multiplicity(n, k, mult=2, c=1000, within=900, across=100):
    """mult + 1 equal, identically built populations (plus the leftover samples): the leading eigenvalue of B has
    multiplicity `mult` exactly."""
    m = n // (mult + 2)
    s, levels = block_constant(n, [m] * (mult + 1), within, across, c)
    return _spectrum(s, levels, k, "multiplicity %d" % mult)


def near_tie(n, k, c=1000, within=1000000100, across=100, bump=1):
    """Three equal populations, the first raised by `bump`: the two leading eigenvalues are within a relative ~1e-9."""
    m = n // 4
    s, levels = block_constant(n, [m] * 3, within, across, c, bump=bump)
    return _spectrum(s, levels, k, "near tie")


# ------------------------------------------------------------------------------------------------- exactly integer B
INT_X_MAX = 8        # integer_vectors draws from [-INT_X_MAX, INT_X_MAX]


def integer_centred(n, seed, hi=1000, scale=1, zero_row=None):
    """A symmetric int64 S whose centred matrix is an INTEGER matrix, and that matrix: (S, B).  A random symmetric matrix
    with entries in [0, hi); row and column `zero_row` zeroed (a sample that carries nothing); every diagonal entry raised by
    (-rowsum) % n, so that every row sum is divisible by n; S[0, 0] raised by n ((-(total // n)) % n), so that the total is
    divisible by n^2; everything times `scale`.  rowMean, colMean and the matrix mean are then integers, B = S - r_i / n -
    r_j / n + m is an integer matrix, and for an integer x every partial sum of B x, in any order of addition, is an integer:
    asserted to stay below 2^53 for |x| <= INT_X_MAX, so every correct mat-vec equals the int64 product bit for bit."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, hi, size=(n, n), dtype=np.int64)
    s = np.triu(a) + np.triu(a, 1).T
    if zero_row is not None:
        s[zero_row, :] = 0
        s[:, zero_row] = 0
    s[np.diag_indices_from(s)] += (-s.sum(axis=1)) % n
    s[0, 0] += n * ((-(int(s.sum()) // n)) % n)
    s *= scale
    r = s.sum(axis=1)
    total = int(r.sum())
    assert np.all(r % n == 0) and total % (n * n) == 0 and np.array_equal(s, s.T)
    rm = r // n
    b = s - rm[:, None] - rm[None, :] + total // (n * n)
    assert n * int(np.abs(b).max()) * INT_X_MAX < 2 ** 53 and int(np.abs(r).max()) < 2 ** 53 and abs(total) < 2 ** 53, (
        "n = %d, seed = %d, scale = %d: a partial sum of B x may leave the integers of float64" % (n, seed, scale))
    return s, b


def integer_vectors(n, seed, count=3):
    """[count, n] float64 vectors of integers drawn per position from [-INT_X_MAX, INT_X_MAX]."""
    rng = np.random.default_rng([seed, n])
    return rng.integers(-INT_X_MAX, INT_X_MAX + 1, size=(count, n)).astype(np.float64)


# ------------------------------------------------------------------------------------------------- helpers
def symmetric_noise(rng, n, rows=2048):
    """E + E^T as float32 [n, n], E uniform in {-1, 0, 1} (generated in row blocks)."""
    a = np.empty((n, n), dtype=np.float32)
    for r0 in range(0, n, rows):
        a[r0:r0 + rows] = rng.integers(-1, 2, size=(min(rows, n - r0), n), dtype=np.int8)
    a += a.T.copy()
    return a


def norm_estimate(a, iters=40, seed=5):
    """||A||_2 of a symmetric A by power iteration (a lower bound that converges from below)."""
    x = np.random.default_rng(seed).standard_normal(a.shape[0]).astype(a.dtype)
    est = 0.0
    for _ in range(iters):
        y = a @ x
        est = float(np.linalg.norm(y.astype(np.float64)) / np.linalg.norm(x.astype(np.float64)))
        x = y / np.float32(np.linalg.norm(y))
    return est


def _block_constant_similarity(n, pops, within, across, bump):
    """S[i, j] = within (+ bump inside population 0) if i and j belong to the same population, else across: the centred matrix
    has the between-population contrasts as its only non-zero eigen-directions, (len(pops) - 1) of them in one cluster that
    `bump` splits by a relative ~ bump / (within - across)."""
    offs = np.concatenate([[0], np.cumsum(pops)])
    s = np.full((n, n), across, dtype=np.int64)
    for p in range(len(pops)):
        s[offs[p]:offs[p + 1], offs[p]:offs[p + 1]] = within + (bump if p == 0 else 0)
    return s, offs


def _reduced_eigenvalues(pops, within, across, bump):
    """Eigenvalues of B = J S J for a block-constant S from the len(pops)-dimensional problem on the normalised population
    indicators (exact structure, long double arithmetic)."""
    sz = np.asarray(pops, dtype=np.longdouble)
    nn = sz.sum()
    k = len(pops)
    sr = np.empty((k, k), dtype=np.longdouble)
    for p in range(k):
        for q in range(k):
            val = (within + (bump if p == 0 else 0)) if p == q else across
            sr[p, q] = np.longdouble(val) * np.sqrt(sz[p] * sz[q])
    root = np.sqrt(sz)
    jr = np.eye(k, dtype=np.longdouble) - np.outer(root, root) / nn
    br = (jr @ sr @ jr).astype(np.float64)
    return np.sort(np.linalg.eigvalsh(br))[::-1]


def _centred_matvec_host(sf, u):
    """B u = (S - m 1^T - 1 m^T + mm 1 1^T) u for a float64 S, without forming B."""
    n = sf.shape[0]
    rs = sf.sum(axis=1)
    mean = rs / n
    mm = rs.sum() / n / n
    return sf @ u - mean * u.sum() - (mean @ u) + mm * u.sum()


def centred_matmul_host(sf):
    """U -> B U column by column (`_centred_matvec_host`), for check_pairs."""
    return lambda u: np.column_stack([_centred_matvec_host(sf, u[:, t]) for t in range(u.shape[1])])


# ------------------------------------------------------------------------------------------------- checks
def lanczos_bars(sp):
    """The bars of the Lanczos path (csrc/eig_lanczos.hip), derived from its acceptance rule instead of the dense solver's
    accuracy: a pair is returned once its TRUE residual r on the device satisfies 0.125 r <= 1e-11 scale (`accept`, tol =
    1e-11, scale = the largest |Ritz value| <= ||B||), i.e. r <= 8e-11 ||B||.  The host's residual differs from the device's
    by the rounding of one product, O(N 2^-53 ||B||) < 1e-12 ||B|| at the N of the tests, so
        residual, eigenvalue:  1e-10 ||B||          (|lambda - lambda_ref| <= ||r|| for a symmetric B)
        isolated vector:       VEC_BAR + 2e-10 ||B|| / gap
        whole cluster:         SUB_BAR + 2e-10 ||B|| / gap_cluster
    (Davis-Kahan with the residual bar: sin of the angle <= r / gap, and ||u - u_ref|| <= sqrt(2) sin, taken as 2), with
    gap the distance to the nearest level outside the cluster (Spectrum.gap; a cluster takes its members' smallest).
    Orthogonality keeps ORTH_BAR: the returned vectors are Ritz vectors of ONE orthonormal basis."""
    scale = sp.norm if sp.norm > 0 else 1.0
    extra = 2e-10 * scale / sp.gap
    return {"eig": 1e-10, "res": 1e-10, "orth": ORTH_BAR, "vec": extra, "sub": extra}


def check_pairs(sp, comps, lam, bmul, what="", bars=None):
    """Holds computed pairs (comps [N, k], lam [k]) to the Spectrum sp.  bmul(U) = B U on the host.  Returns the observed
    maxima {eig, res, orth, vec, sub} relative to the bars' units (eigenvalue and residual as multiples of ||B||_2).
    bars: None = the dense solver's (EIG_BAR, RES_BAR, ORTH_BAR, VEC_BAR, SUB_BAR), or a dict {eig, res, orth: scalars in
    the same units; vec, sub: [k] additions to VEC_BAR / SUB_BAR per selected eigenvalue} such as `lanczos_bars`."""
    scale = sp.norm if sp.norm > 0 else 1.0
    k = sp.k
    if bars is None:
        bars = {"eig": EIG_BAR, "res": RES_BAR, "orth": ORTH_BAR, "vec": np.zeros(k), "sub": np.zeros(k)}
    eig_bar, res_bar, orth_bar = bars["eig"], bars["res"], bars["orth"]
    assert comps.shape == (sp.n, k) and lam.shape == (k,), what
    err = np.abs(lam - sp.lam)
    assert np.all(err <= eig_bar * scale + sp.lam_tol), "%s eigenvalues: |lambda - ref| = %s > %.3g ||B|| + %.3g" % (
        what, err.tolist(), eig_bar, sp.lam_tol)
    res = np.linalg.norm(bmul(comps) - comps * lam, axis=0)
    assert np.all(res <= res_bar * scale), "%s residual ||Bu - lambda u|| / ||B|| = %s" % (what, (res / scale).tolist())
    orth = float(np.abs(comps.T @ comps - np.eye(k)).max())
    assert orth <= orth_bar, "%s orthogonality |U^T U - I| = %.3g" % (what, orth)
    for t in range(k):
        u = comps[:, t]
        assert u.max() >= -u.min(), "%s sign rule: PC%d has its largest magnitude negative" % (what, t + 1)
    vec = sub = 0.0
    for members, whole in sp.groups:
        if not whole:
            continue
        if np.isnan(sp.vecs[:, members]).any():
            continue
        if len(members) == 1:
            t = members[0]
            ref = sp.vecs[:, t]
            u = comps[:, t] if comps[:, t] @ ref >= 0 else -comps[:, t]
            d = float(np.linalg.norm(u - ref))
            vec_bar = VEC_BAR + sp.vec_tol[t] + bars["vec"][t]
            assert d <= vec_bar, "%s vector PC%d: ||u - u_ref|| = %.3g > %.3g" % (what, t + 1, d, vec_bar)
            vec = max(vec, d)
        else:
            u, ref = comps[:, members], sp.vecs[:, members]
            # ||U U^T - R R^T||_2 = sin of the largest principal angle = ||(I - R R^T) U||_2 for equal dimensions
            d = float(np.linalg.norm(u - ref @ (ref.T @ u), 2))
            sub_bar = SUB_BAR + max(sp.vec_tol[t] for t in members) + max(bars["sub"][t] for t in members)
            assert d <= sub_bar, "%s cluster PC%s: ||UU^T - U_ref U_ref^T|| = %.3g > %.3g" % (
                what, [t + 1 for t in members], d, sub_bar)
            sub = max(sub, d)
    return {"eig": float((err / scale).max()), "res": float((res / scale).max()), "orth": orth, "vec": vec, "sub": sub}

"""What the tests of the GRM LD prune share (no test here): the numpy statement of the rule of pcoa_grm_ld_prune (include/pcoa.h,
DESIGN.md 4.19) as a V x V matrix and as a band, two deliberately wrong rules a plausible wrong kernel would follow, the cohort
generator, and the store's word coding for the popcount identities.

A cohort is g, [V][N] int8: the dosage 0 / 1 / 2, -1 = not called."""
import numpy as np

SHAPES = [(33, 300, 1, .5), (70, 700, 7, .2), (130, 1000, 64, .5), (260, 1000, 65, .8), (1025, 600, 50, .2)]   # N, V, W, t


def cohort(n, v, seed, miss=0.05):
    rng = np.random.default_rng(seed)
    g = np.zeros((v, n), dtype=np.int8); r = 0
    while r < v:
        f = rng.uniform(0.05, 0.5); h0 = rng.random(n) < f; h1 = rng.random(n) < f
        run = int(rng.integers(1, 13)); noise = [0, .01, .05, .1, .2][int(rng.integers(0, 5))]; chain = rng.random() < .5
        for _ in range(run):
            if r >= v: break
            a = h0 ^ (rng.random(n) < noise); b = h1 ^ (rng.random(n) < noise)
            if chain: h0, h1 = a, b
            row = a.astype(np.int8) + b.astype(np.int8)
            if rng.random() < .2: row = 2 - row
            g[r] = row; r += 1
    m = rng.random((v, n)) < miss
    for k in range(7, v, 37): m[k] |= rng.random(n) < 0.6      # rows with heavy missingness
    g[m] = -1                                                   # -1 = not called
    if v > 3: g[3][g[3] >= 0] = 0                               # monomorphic
    if v > 5: g[5] = -1                                         # never called
    if v > 9: g[9] = g[8]                                       # duplicate, missing pattern included
    return g


def to_codes(g):
    """PLINK codes with A2 the reference (ref_is_a1 False): g = 2 -> 00, not called -> 01, g = 1 -> 10, g = 0 -> 11."""
    return np.array([1, 3, 2, 0], dtype=np.uint8)[np.asarray(g, dtype=np.int64) + 1]


def candidates(g, min_maf=0.0):
    """used_v of pcoa_create_grm from the dosages."""
    c = g >= 0
    n = c.sum(axis=1).astype(np.int64)
    a = np.where(c, g, 0).astype(np.int64).sum(axis=1)
    return (n > 0) & (a > 0) & (a < 2 * n) & (np.minimum(a, 2 * n - a).astype(np.float64) >= min_maf * (2.0 * n.astype(np.float64)))


def _compare(n, su, sv, qu, qv, p, t):
    cov = n * p - su * sv
    var_u, var_v = n * qu - su * su, n * qv - sv * sv
    return cov.astype(np.float64) * cov.astype(np.float64) > t * (var_u.astype(np.float64) * var_v.astype(np.float64))


def exceeds_matrix(g, t, ignore_missing=False):
    """exceeds(u, v) for every pair, [V][V] bool, from n, s, q, p as integer matrix products.  ignore_missing: the WRONG rule that
    sums over all N samples with a missing call as 0 and n = N."""
    c = (g >= 0).astype(np.int64)
    x = np.where(g >= 0, g, 0).astype(np.int64)
    if ignore_missing:
        c = np.ones_like(c)
    n = c @ c.T
    s = x @ c.T                # s[u, v]: the dosage sum of u over the samples called at both
    q = (x * x) @ c.T
    p = x @ x.T
    return _compare(n, s, s.T, q, q.T, p, t)


def exceeds_band(g, w, t, stats=False):
    """[V][w] bool: column d - 1 = exceeds(v - d, v), False where v - d < 0; only the band is computed.  stats: also n p and
    cov^2 / (var_u var_v) (nan where a variance is 0) of every band entry."""
    v = g.shape[0]
    c = (g >= 0).astype(np.int64)
    x = np.where(g >= 0, g, 0).astype(np.int64)
    out = np.zeros((v, w), dtype=bool)
    n_p = np.zeros((v, w), dtype=np.int64)
    ratio = np.full((v, w), np.nan)
    for d in range(1, min(w, v - 1) + 1):
        cu, cv, xu, xv = c[:-d], c[d:], x[:-d], x[d:]
        j = cu * cv
        n, su, sv, qu, qv, p = j.sum(1), (xu * j).sum(1), (xv * j).sum(1), (xu * xu * j).sum(1), (xv * xv * j).sum(1), (xu * xv).sum(1)
        out[d:, d - 1] = _compare(n, su, sv, qu, qv, p, t)
        if stats:
            n_p[d:, d - 1] = n * p
            den = (n * qu - su * su).astype(np.float64) * (n * qv - sv * sv).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio[d:, d - 1] = np.where(den > 0, (n * p - su * sv).astype(np.float64) ** 2 / den, np.nan)
    return (out, n_p, ratio) if stats else out


def starts(v, breaks):
    """start[r]: the last break at or in front of row r (0 without one)."""
    out = np.zeros(v, dtype=np.int64)
    for b in breaks:
        out[int(b):] = int(b)
    return out


def greedy(ex, cand, w, breaks=(), non_greedy=False):
    """The forward greedy pass over a V x V exceeds matrix: bool keep mask.  non_greedy: the WRONG rule in which any candidate
    predecessor in the window blocks, kept or not."""
    v = ex.shape[0]
    st = starts(v, breaks)
    keep = np.zeros(v, dtype=bool)
    block = cand if non_greedy else keep
    for r in range(v):
        if not cand[r]:
            continue
        lo = max(r - w, int(st[r]))
        keep[r] = not np.any(block[lo:r] & ex[lo:r, r])
    return keep


def greedy_band(band, cand, w, breaks=()):
    """The same pass over exceeds_band's output."""
    v = band.shape[0]
    st = starts(v, breaks)
    keep = np.zeros(v, dtype=bool)
    for r in range(v):
        if not cand[r]:
            continue
        reach = min(w, r - int(st[r]))
        keep[r] = not np.any(keep[r - reach:r][::-1] & band[r, :reach])
    return keep


def rule(g, w, t, breaks=(), min_maf=0.0):
    """(keep mask, candidates, kept, in-window pairs) of pcoa_grm_ld_prune."""
    cand = candidates(g, min_maf)
    keep = greedy(exceeds_matrix(g, t), cand, w, breaks)
    return keep, int(cand.sum()), int(keep.sum()), window_pairs(g.shape[0], w, breaks)


def window_pairs(v, w, breaks=()):
    st = starts(v, breaks)
    return int(np.minimum(w, np.arange(v) - st).sum())


def window_mask(v, w, breaks=()):
    """[V][V] bool: (u, v) is an in-window pair behind the breaks."""
    st = starts(v, breaks)
    u, r = np.arange(v)[:, None], np.arange(v)[None, :]
    return (u < r) & (u >= r - w) & (u >= st[None, :])


# ---- the store's words (grm_bits.hip): 16 slots of 2 bits, 00 g = 0, 01 not called, 10 g = 1, 11 g = 2; padding slots 01 -------
K_LO = np.uint32(0x55555555)


def store_words(g, pitch_words=None):
    v, n = g.shape
    words = (n + 15) // 16
    pitch = pitch_words or (words + 3) // 4 * 4
    slots = np.full((v, pitch * 16), 1, dtype=np.uint32)
    slots[:, :n] = np.array([1, 0, 2, 3], dtype=np.uint32)[np.asarray(g, dtype=np.int64) + 1]
    sh = (2 * np.arange(16, dtype=np.uint32))[None, None, :]
    return (slots.reshape(v, pitch, 16) << sh).sum(axis=2, dtype=np.uint64).astype(np.uint32)


def popc(x):
    return np.unpackbits(np.ascontiguousarray(x, dtype=np.uint32).view(np.uint8), axis=-1).reshape(x.shape + (32,)).sum(axis=-1) \
        .astype(np.int64)


def popcount_sums(wu, wv):
    """(n, s_u, s_v, q_u, q_v, p) of two rows of store words by the seven popcounts of grm_ld.hip."""
    def masks(w):
        hi = (w >> np.uint32(1)) & K_LO
        both = hi & w
        called = (hi | ~w) & K_LO
        return hi, both, called
    hu, bu, cu = masks(wu)
    hv, bv, cv = masks(wv)
    xu, xv = hu | (bu << np.uint32(1)), hv | (bv << np.uint32(1))
    xsv = bv | (hv << np.uint32(1))
    c2u, c2v = cu | (cu << np.uint32(1)), cv | (cv << np.uint32(1))
    n = popc(cu & cv).sum()
    su, sv = popc(xu & c2v).sum(), popc(xv & c2u).sum()
    qu, qv = su + 2 * popc(bu & cv).sum(), sv + 2 * popc(bv & cu).sum()
    p = popc(xu & xv).sum() + popc(xu & xsv).sum()
    return int(n), int(su), int(sv), int(qu), int(qv), int(p)


def direct_sums(gu, gv):
    j = (gu >= 0) & (gv >= 0)
    a, b = gu[j].astype(np.int64), gv[j].astype(np.int64)
    return int(j.sum()), int(a.sum()), int(b.sum()), int((a * a).sum()), int((b * b).sum()), int((a * b).sum())

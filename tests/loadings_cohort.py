"""Helpers of the loadings tests: the numpy statement of the rule, the planted cohort, the bitset and .bed encoders.  No GPU.

The rule (include/pcoa.h): with X the V x N carrier matrix, J = I - 11^T / N and (u_c, lambda_c) an eigenpair of
B = J S J = (X J)^T (X J), the loading of variant v on axis c is w_c[v] = (sum over the carriers i of v of (u_c[i] - mean(u_c)))
/ sqrt(lambda_c)."""
import numpy as np

CENTRE, UNIT = 1, 2


def loadings_rule(x, u, lam=None, centre=True):
    """(X @ (U - mean)) / sqrt(lambda) in longdouble.  x [V, N] 0/1, u [N, k], lam [k] or None (no division)."""
    xl = np.asarray(x, dtype=np.longdouble)
    ul = np.asarray(u, dtype=np.longdouble)
    if centre:
        ul = ul - ul.mean(axis=0, keepdims=True)
    w = xl @ ul
    if lam is not None:
        w = w / np.sqrt(np.asarray(lam, dtype=np.longdouble))[None, :]
    return w


def summation_bound(x, u, lam, w):
    """The bound of test_gpu_loadings case 5 for every entry, [V, k]: with c_v the carriers of row v and u' the centred vector,
    2^-52 c_v (sum_{i carries v} |u'_i| + sum_i |u_i|) / sqrt(lambda) + 3 2^-53 |w| -- twice the first-order bound of
    any-order summation of c_v terms, plus the error of a mean of N terms, plus the square root and the division."""
    xl = np.asarray(x, dtype=np.longdouble)
    ul = np.asarray(u, dtype=np.longdouble)
    uc = ul - ul.mean(axis=0, keepdims=True)
    cv = xl.sum(axis=1)[:, None]
    carried = xl @ np.abs(uc)
    total = np.abs(ul).sum(axis=0)[None, :]
    root = np.sqrt(np.asarray(lam, dtype=np.longdouble))[None, :]
    return 2.0 ** -52 * cv * (carried + total) / root + 3 * 2.0 ** -53 * np.abs(np.asarray(w, dtype=np.longdouble))


def planted_cohort(n=200, v=4096, seed=20250917):
    """N samples in four populations dealt round-robin, V variants: a base frequency in [0.05, 0.3] per variant and a
    per-population shift of sd 0.12 around it.  Returns x [V, N] uint8."""
    rng = np.random.default_rng(seed)
    pop = np.arange(n) % 4
    base = rng.uniform(0.05, 0.3, size=(v, 1))
    freq = np.clip(base + rng.normal(0.0, 0.12, size=(v, 4)), 0.0, 1.0)
    return (rng.random((v, n)) < freq[:, pop]).astype(np.uint8)


def centred_eig(x, k):
    """The k leading eigenpairs of B = J X^T X J by numpy.linalg.eigh: (u [N, k], lam [k]), largest first."""
    xf = np.asarray(x, dtype=np.float64)
    xc = xf - xf.mean(axis=1, keepdims=True)      # X J
    lam, u = np.linalg.eigh(xc.T @ xc)
    order = np.argsort(lam)[::-1][:k]
    return u[:, order], lam[order]


def identity_defects(x, u, lam, w):
    """(max |W^T W - I|, max |(X J)^T W diag(lambda^-1/2) - U|) up to the sign of each column."""
    xf = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    xc = xf - xf.mean(axis=1, keepdims=True)
    back = (xc.T @ w) / np.sqrt(np.asarray(lam, dtype=np.float64))[None, :]
    return float(np.abs(w.T @ w - np.eye(w.shape[1])).max()), float(np.abs(back - np.asarray(u, dtype=np.float64)).max())


def pack_rows(x, n, pad_words=0, garbage=None):
    """0/1 [V, N] -> uint32 bitsets [V, ceil(N / 32) + pad_words], sample i = bit i & 31 of word i >> 5.  garbage: a Generator
    -> the bits of samples >= N and every pad word are SET (all ones), as case 1 of test_gpu_loadings demands."""
    x = np.asarray(x)
    v = x.shape[0]
    words = (n + 31) // 32
    b = np.packbits(x.astype(bool), axis=1, bitorder="little")
    out = np.zeros((v, (words + pad_words) * 4), dtype=np.uint8)
    out[:, :b.shape[1]] = b
    out = out.view("<u4").copy()
    if garbage is not None:
        out[:, words:] = 0xffffffff
        if n & 31:
            out[:, words - 1] |= np.uint32((0xffffffff << (n & 31)) & 0xffffffff)
    return out


def encode_bed(x, n, missing=None, ref_is_a1=False, rng=None):
    """Carrier matrix x [V, N] -> raw .bed rows uint8 [V, ceil(N / 4)] (sample s in bits 2 (s % 4) of byte s / 4; 00 hom A1,
    01 missing, 10 het, 11 hom A2).  A carrier becomes het or, half the time, homozygous non-reference; a non-carrier homozygous
    reference; missing [V, N] bool marks calls coded 01.  With A2 the reference allele the carrier codes are 00 / 10, with
    ref_is_a1 they are 11 / 10.  The padding genotypes of the last byte are coded as carriers: the decode must not trust them."""
    x = np.asarray(x).astype(bool)
    v = x.shape[0]
    rng = rng or np.random.default_rng(0)
    hom_alt, hom_ref = (3, 0) if ref_is_a1 else (0, 3)
    bpv = (n + 3) // 4
    codes = np.full((v, bpv * 4), 2, dtype=np.uint8)
    body = np.where(x, np.where(rng.random((v, n)) < 0.5, 2, hom_alt), hom_ref).astype(np.uint8)
    if missing is not None:
        body[np.asarray(missing, dtype=bool)] = 1
    codes[:, :n] = body
    q = codes.reshape(v, bpv, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def decode_bed(bed, n, ref_is_a1=False):
    """The rule of plink_bed_to_bits_kernel in numpy: raw rows -> carrier matrix [V, N] (a missing call carries nothing)."""
    bed = np.asarray(bed, dtype=np.uint8)
    codes = np.stack([(bed >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(bed.shape[0], -1)[:, :n]
    return ((codes == 2) | (codes == (3 if ref_is_a1 else 0))).astype(np.uint8)

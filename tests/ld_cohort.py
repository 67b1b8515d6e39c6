"""Helpers of the LD-pruning tests: the numpy statement of the rule and the cohort generator.  No GPU, no test.

The rule (include/pcoa.h).  Variants arrive in feed order; n is the sample count, a_v the carrier count of
variant v and c_uv = popcount(row_u & row_v).  For a window W (in fed variants) and a threshold t

    D = n c_uv - a_u a_v,   p = a_u (n - a_u),   q = a_v (n - a_v)                    (int64)
    exceeds(u, v)  <=>  float64(D) * float64(D)  >  t * (float64(p) * float64(q))         (three products, no sum)

and the pass is forward and greedy: a monomorphic variant (a_v = 0 or n) is removed; a polymorphic v is kept iff no KEPT u
with v - W <= u < v, behind the last break, has exceeds(u, v); a removed variant blocks nobody."""
import numpy as np

from loadings_cohort import decode_bed, encode_bed, pack_rows   # (re-exported for the tests)

__all__ = ["exceeds_matrix", "ld_rule", "ld_rule_banded", "ld_rule_nongreedy", "ld_pairs", "ld_cohort", "write_plink",
           "decode_bed", "encode_bed", "pack_rows"]


def exceeds_matrix(x, t):
    """exceeds(u, v) for every pair, [V, V] bool, by the three-product expression (int64 up to the casts)."""
    x = np.asarray(x)
    n = np.int64(x.shape[1])
    xf = x.astype(np.float64)
    c = np.rint(xf @ xf.T).astype(np.int64)       # counts <= n: exact in float64
    a = x.sum(axis=1, dtype=np.int64)
    d = n * c - a[:, None] * a[None, :]
    p = a * (n - a)
    df = d.astype(np.float64)
    pf = p.astype(np.float64)
    return (df * df) > (np.float64(t) * (pf[:, None] * pf[None, :]))


def _window_start(v, window, breaks):
    start = max(0, v - window)
    for b in breaks:
        if b <= v:
            start = max(start, b)
    return start


def ld_rule(x, window, t, breaks=()):
    """The keep mask [V] bool.  breaks: indices b such that a break lies in front of row b."""
    x = np.asarray(x)
    v_total, n = x.shape
    ex = exceeds_matrix(x, t)
    a = x.sum(axis=1, dtype=np.int64)
    keep = np.zeros(v_total, dtype=bool)
    breaks = sorted(int(b) for b in breaks)
    for v in range(v_total):
        if a[v] == 0 or a[v] == n:
            continue
        s = _window_start(v, window, breaks)
        keep[v] = not (ex[v, s:v] & keep[s:v]).any()
    return keep


def ld_rule_banded(x, window, t, breaks=()):
    """ld_rule without the V x V matrix, for cohorts of 10^5 rows: exceeds(v - d, v) is evaluated for d = 1 .. window only,
    by the same three-product expression in the same dtypes, and the same greedy pass runs over the band."""
    x = np.asarray(x)
    v_total, n = x.shape
    n64 = np.int64(n)
    a = x.sum(axis=1, dtype=np.int64)
    pf = (a * (n64 - a)).astype(np.float64)
    ex = np.zeros((v_total, window), dtype=bool)        # ex[v, d - 1] = exceeds(v - d, v)
    for d in range(1, min(window, v_total - 1) + 1):
        c = (x[d:] & x[:-d]).sum(axis=1, dtype=np.int64)      # 0 / 1 rows: the AND is the product
        df = (n64 * c - a[d:] * a[:-d]).astype(np.float64)
        ex[d:, d - 1] = (df * df) > (np.float64(t) * (pf[d:] * pf[:-d]))
    keep = np.zeros(v_total, dtype=bool)
    breaks = sorted(int(b) for b in breaks)
    for v in range(v_total):
        if a[v] == 0 or a[v] == n:
            continue
        s = _window_start(v, window, breaks)
        keep[v] = not (ex[v, :v - s] & keep[s:v][::-1]).any()
    return keep


def ld_rule_nongreedy(x, window, t, breaks=()):
    """The shortcut that is NOT the rule: v is removed when ANY polymorphic in-window predecessor exceeds, kept or not."""
    x = np.asarray(x)
    v_total, n = x.shape
    ex = exceeds_matrix(x, t)
    a = x.sum(axis=1, dtype=np.int64)
    keep = np.zeros(v_total, dtype=bool)
    breaks = sorted(int(b) for b in breaks)
    for v in range(v_total):
        if a[v] == 0 or a[v] == n:
            continue
        s = _window_start(v, window, breaks)
        keep[v] = not ex[v, s:v].any()
    return keep


def ld_pairs(v_total, window, breaks=()):
    """(earlier row, row) pairs inside the windows: what pcoa_ld_stats.ld_pairs counts."""
    breaks = sorted(int(b) for b in breaks)
    return sum(v - _window_start(v, window, breaks) for v in range(v_total))


def ld_cohort(n, v, seed):
    """[V, N] uint8: runs of 1..12 rows behind a founder of carrier frequency 0.05..0.5 -- noisy copies (each genotype flipped
    with probability 0, 0.01, 0.05, 0.1 or 0.2) of the founder or, in every other run, of the ROW BEFORE (a drifting chain: a row
    exceeds against its neighbour and no longer against the neighbour's neighbour), complements of such copies, exact duplicates
    -- so that rows exceed at every threshold and many an exceeding pair has an earlier member that was itself removed.  Row 3
    is all zero, row 5 all ones and row 9 a duplicate of row 8 (where there are that many)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((v, n), dtype=np.uint8)
    r = 0
    while r < v:
        founder = (rng.random(n) < rng.uniform(0.05, 0.5)).astype(np.uint8)
        run = int(rng.integers(1, 13))
        noise = [0.0, 0.01, 0.05, 0.1, 0.2][int(rng.integers(0, 5))]
        chain = rng.random() < 0.5
        for _ in range(run):
            if r >= v:
                break
            founder_or_last = founder ^ (rng.random(n) < noise).astype(np.uint8)
            if chain:
                founder = founder_or_last
            row = founder_or_last
            if rng.random() < 0.2:
                row = 1 - row
            x[r] = row
            r += 1
    if v > 3:
        x[3] = 0
    if v > 5:
        x[5] = 1
    if v > 9:
        x[9] = x[8]
    return x


def write_plink(prefix, x, contigs, seed=0):
    """x [V, N] as a PLINK 1 fileset <prefix>.bed/.bim/.fam (A2 the reference allele, no missing calls); contigs: one name per
    variant.  Returns the (contig, position, id) of every variant as the hosts record them."""
    x = np.asarray(x)
    v, n = x.shape
    with open(prefix + ".fam", "w") as f:
        for i in range(n):
            f.write("FAM%d S%04d 0 0 0 -9\n" % (i, i))
    meta = [(str(contigs[k]), 1000 + 13 * k, "rs%d" % k) for k in range(v)]
    with open(prefix + ".bim", "w") as f:
        for contig, pos, vid in meta:
            f.write("%s\t%s\t0\t%d\tC\tA\n" % (contig, vid, pos))
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6c, 0x1b, 0x01]))
        f.write(encode_bed(x, n, rng=np.random.default_rng(seed)).tobytes())
    return meta

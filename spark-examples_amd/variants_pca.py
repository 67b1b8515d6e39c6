"""Host-side mirror of the reference's PCoA driver, on top of the HIP engine.

Same names, argument meaning and error behaviour as the reference interface for this path:

  reference (Scala, VariantsPca.scala)                     here
  ---------------------------------------------------------------------------------------------
  VariantsPcaDriver.extractCallInfo            :56-60      extract_call_info
  VariantsPcaDriver.getCallsRdd                :153-168    VariantsPcaDriver.getCallsRdd / prepare_call_data
  VariantsPcaDriver.getSimilarityMatrix        :182-191    VariantsPcaDriver.getSimilarityMatrix / calculate_similarity_matrix
  VariantsPcaDriver.computePca                 :198-231    VariantsPcaDriver.computePca / center_matrix + perform_pca
  VariantsPcaDriver.emitResult                 :233-246    VariantsPcaDriver.emitResult
  VariantsPcaDriver.main                       :38-50      main
  PcaConf / GenomicsConf flags                 GenomicsConf.scala:31-101   PcaConf

and of the Python twin src/main/python/variants_pca.py (prepare_call_data :19-52,
calculate_similarity_matrix :54-82, center_matrix :84-121, perform_pca :123-152).

An "RDD" here is a plain Python list (of variant dicts, or of per-variant index lists); the
distributed part of the reference (partitions + reduceByKey) is the GPU Gram kernel + all-reduce.
Nothing in this module computes on the CPU: every matrix operation goes through libpcoa_hip.so.
"""
from __future__ import print_function

import argparse
import os
import sys

import numpy as np

if __name__ == "__main__" and not __package__:
    # started by path (`python spark-examples_amd/variants_pca.py ...`; torch.distributed.run starts a rank this way): load the
    # module inside its package -- the relative imports below need one
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.exit(importlib.import_module("spark-examples_amd.variants_pca").main(sys.argv[1:]))

from .engine import PcoaEngine

PLINK_BLOCK_ROWS = 1 << 16   # raw .bed rows handed to pcoa_accumulate_plink_bed per call (41 MB at N = 2504)


# --------------------------------------------------------------------------------------------- a1/a2
def extract_call_info(variant, mapping):
    """VariantsPcaDriver.extractCallInfo (VariantsPca.scala:56-60).

    variant: dict with optional 'calls' -> list of {'callSetId'|'callsetId': str, 'genotype': [int]}.
    Returns [(hasVariation, callsetIndex)]; hasVariation = genotype.exists(_ > 0) -- a missing
    allele (-1) or hom-ref (0) does not vary.  An unknown callset id raises KeyError, as
    mapping(call.callsetId) throws NoSuchElementException in the reference."""
    out = []
    for call in (variant.get("calls") or []):
        cid = call["callSetId"] if "callSetId" in call else call["callsetId"]
        has_variation = False
        for allele in call.get("genotype", []):
            has_variation = has_variation or allele > 0
        out.append((has_variation, mapping[cid]))
    return out


def variant_meta_of(variant):
    """(contig, 1-based position, id) of a variant record: a line's first columns in the --loadings-output-path file."""
    return (variant["contig"], int(variant["start"]) + 1, variant.get("id", "."))


def prepare_call_data(py_rdd, py_id_to_index, meta=None):
    """prepare_call_data (variants_pca.py:19-52) == getCallsRdd for one variant set
    (VariantsPca.scala:153-157,163-167): keep calls with variation, drop variants with none,
    map callset ids to indices.  Returns a list of index lists (RDD[Seq[Int]]).

    Note: the Python twin tests any(genotype) (non-zero, so -1 counts) where the Scala driver tests
    _ > 0; this mirror follows the Scala driver."""
    call_rdd = []
    for variant in py_rdd:
        calls = [idx for (has_variation, idx) in extract_call_info(variant, py_id_to_index) if has_variation]
        if len(calls) > 0:
            call_rdd.append(calls)
            if meta is not None:
                meta.append(variant_meta_of(variant))
    return call_rdd


# --------------------------------------------------------------------------------------------- join / merge
_M64 = 0xFFFFFFFFFFFFFFFF


def _rotl64(x, r):
    return ((x << r) | (x >> (64 - r))) & _M64


def _fmix64(k):
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & _M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & _M64
    k ^= k >> 33
    return k


def murmur3_128_hex(data, seed=0):
    """Guava Hashing.murmur3_128(seed).hashBytes(data).toString(): MurmurHash3_x64_128, the two 64-bit
    halves printed as little-endian bytes (the reference keys variants with it, VariantsPca.scala:69-77)."""
    c1, c2 = 0x87C37B91114253D5, 0x4CF5AD432745937F
    h1 = h2 = seed & _M64
    n = len(data)
    nblocks = n // 16
    for i in range(nblocks):
        k1 = int.from_bytes(data[16 * i:16 * i + 8], "little")
        k2 = int.from_bytes(data[16 * i + 8:16 * i + 16], "little")
        k1 = (k1 * c1) & _M64; k1 = _rotl64(k1, 31); k1 = (k1 * c2) & _M64; h1 ^= k1
        h1 = _rotl64(h1, 27); h1 = (h1 + h2) & _M64; h1 = (h1 * 5 + 0x52DCE729) & _M64
        k2 = (k2 * c2) & _M64; k2 = _rotl64(k2, 33); k2 = (k2 * c1) & _M64; h2 ^= k2
        h2 = _rotl64(h2, 31); h2 = (h2 + h1) & _M64; h2 = (h2 * 5 + 0x38495AB5) & _M64
    tail = data[16 * nblocks:]
    k1 = k2 = 0
    if len(tail) > 8:
        k2 = int.from_bytes(tail[8:], "little")
        k2 = (k2 * c2) & _M64; k2 = _rotl64(k2, 33); k2 = (k2 * c1) & _M64; h2 ^= k2
    if len(tail) > 0:
        k1 = int.from_bytes(tail[:8], "little")
        k1 = (k1 * c1) & _M64; k1 = _rotl64(k1, 31); k1 = (k1 * c2) & _M64; h1 ^= k1
    h1 ^= n; h2 ^= n
    h1 = (h1 + h2) & _M64; h2 = (h2 + h1) & _M64
    h1 = _fmix64(h1); h2 = _fmix64(h2)
    h1 = (h1 + h2) & _M64; h2 = (h2 + h1) & _M64
    return (h1.to_bytes(8, "little") + h2.to_bytes(8, "little")).hex()


def get_variant_key(variant, debug=False):
    """VariantsPcaDriver.getVariantKey (VariantsPca.scala:62-78): murmur3_128 over
    contig, start, end, referenceBases, alternateBases.mkString("") as a Guava Hasher sees them
    (putString = UTF-8 bytes, putLong = 8 little-endian bytes)."""
    alternate = "".join(variant.get("alternateBases") or [])
    reference = variant.get("referenceBases") or ""
    if debug:
        print("%s: (%d, %d) ref=%s alt=%s" % (variant["contig"], variant["start"], variant["end"], reference, alternate))
    buf = (variant["contig"].encode("utf-8") + int(variant["start"]).to_bytes(8, "little", signed=True) +
           int(variant["end"]).to_bytes(8, "little", signed=True) + reference.encode("utf-8") +
           alternate.encode("utf-8"))
    return murmur3_128_hex(buf)


def join_datasets(datasets, indexes, debug=False, meta=None):
    """VariantsPcaDriver.joinDatasets (VariantsPca.scala:115-128): two-way INNER join on the variant
    key; the joined record is calls1 ++ calls2 (cross product if a key repeats, as RDD.join does).
    meta: a list that receives variant_meta_of the FIRST set's record of every joined row."""
    keyed = []
    for data in datasets[:2]:
        d = {}
        for variant in data:
            d.setdefault(get_variant_key(variant, debug), []).append((extract_call_info(variant, indexes), variant))
        keyed.append(d)
    out = []
    for key, calls1 in keyed[0].items():
        for c1, v1 in calls1:
            for c2, _ in keyed[1].get(key, []):
                out.append(c1 + c2)
                if meta is not None:
                    meta.append(variant_meta_of(v1))
    return out


def merge_datasets(datasets, variant_set_count, indexes, meta=None):
    """VariantsPcaDriver.mergeDatasets (VariantsPca.scala:136-148): union, group by variant key, keep
    the groups with exactly variantSetCount members, concatenate their calls.
    meta: a list that receives variant_meta_of the first record of every kept group."""
    groups, first = {}, {}
    for data in datasets:
        for variant in data:
            key = get_variant_key(variant)
            groups.setdefault(key, []).append(extract_call_info(variant, indexes))
            first.setdefault(key, variant)
    if meta is not None:
        meta.extend(variant_meta_of(first[k]) for k, g in groups.items() if len(g) == variant_set_count)
    return [[c for calls in g for c in calls] for g in groups.values() if len(g) == variant_set_count]


# --------------------------------------------------------------------------------------------- a3
def calculate_similarity_matrix(call_rdd, matrix_size, engine=None, device=0):
    """calculate_similarity_matrix (variants_pca.py:54-82) == getSimilarityMatrix
    (VariantsPca.scala:182-191).  call_rdd: list of index lists, or a (sample_idx, row_offsets) CSR
    pair.  Returns the PcoaEngine holding S in HBM (use .gram() for the N^2 entries)."""
    eng = engine if engine is not None else PcoaEngine(matrix_size, device=device)
    if isinstance(call_rdd, tuple) and isinstance(call_rdd[0], str) and call_rdd[0] == "bed":
        # a PLINK fileset as it lies in the file: blocks of raw 2-bit rows, decoded on the device (pcoa_accumulate_plink_bed);
        # rows outside --references are squeezed out of a block before it is handed over
        _, geno, keep, ref_is_a1 = call_rdd
        all_kept = bool(keep.all())
        for v0 in range(0, geno.shape[0], PLINK_BLOCK_ROWS):
            rows = geno[v0:v0 + PLINK_BLOCK_ROWS]
            if not all_kept:
                k = keep[v0:v0 + PLINK_BLOCK_ROWS]
                if not k.any():
                    continue
                rows = rows[k]
            eng.accumulate_plink_bed(np.ascontiguousarray(rows), ref_is_a1=ref_is_a1)
    elif isinstance(call_rdd, tuple) and isinstance(call_rdd[0], str) and call_rdd[0] == "bits":
        bits = call_rdd[1]                          # carrier bitsets [variants][ceil(N / 32)] (a PLINK fileset)
        for v0 in range(0, bits.shape[0], 1 << 20):
            eng.accumulate_bits(bits[v0:v0 + (1 << 20)])
    elif isinstance(call_rdd, tuple):
        eng.accumulate_calls(call_rdd[0], call_rdd[1])
    else:
        eng.accumulate_callsets(call_rdd)
    eng.finalize()
    return eng


def calculate_similarity_matrix_calls(call_rdd, matrix_size, device=0):
    """--missing-calls pairwise: getSimilarityMatrix over a PLINK fileset with the companion beside it.  Every block of raw
    .bed rows crosses the link once and is decoded once into the carrier bitsets (the engine) and the missing-call bitsets
    (the companion): pcoa_accumulate_plink_bed_calls.  Returns (engine, companion, variants fed)."""
    _, geno, keep, ref_is_a1 = call_rdd
    eng = PcoaEngine(matrix_size, device=device)
    companion = PcoaEngine(matrix_size, device=device)
    fed = 0
    all_kept = bool(keep.all())
    for v0 in range(0, geno.shape[0], PLINK_BLOCK_ROWS):
        rows = geno[v0:v0 + PLINK_BLOCK_ROWS]
        if not all_kept:
            k = keep[v0:v0 + PLINK_BLOCK_ROWS]
            if not k.any():
                continue
            rows = rows[k]
        eng.accumulate_plink_bed_calls(np.ascontiguousarray(rows), companion, ref_is_a1=ref_is_a1)
        fed += int(rows.shape[0])
    eng.finalize()
    companion.finalize()
    return eng, companion, fed


def shard_calls(call_rdd, rank, world):
    """Rank `rank`'s partition of an RDD[Seq[Int]] in any of the forms getCallsRdd returns -- the contiguous range
    dist.shard_range(rank, world, rows), as the reference's partitions are contiguous ranges of the variant stream
    (VariantsPca.scala:184; numReducePartitions, GenomicsConf.scala:42-45).  The shards of all ranks concatenate to the
    input; S = sum over variants, so the all-reduce of the ranks' partial matrices is the reference's reduceByKey (:190)."""
    from . import dist
    if isinstance(call_rdd, tuple) and isinstance(call_rdd[0], str) and call_rdd[0] == "bed":
        _, geno, keep, ref_is_a1 = call_rdd
        a, b = dist.shard_range(rank, world, geno.shape[0])
        return ("bed", geno[a:b], keep[a:b], ref_is_a1)
    if isinstance(call_rdd, tuple) and isinstance(call_rdd[0], str) and call_rdd[0] == "bits":
        a, b = dist.shard_range(rank, world, call_rdd[1].shape[0])
        return ("bits", call_rdd[1][a:b])
    if isinstance(call_rdd, tuple):
        idx, offs = np.asarray(call_rdd[0]), np.asarray(call_rdd[1])
        a, b = dist.shard_range(rank, world, offs.size - 1)
        return (idx[offs[a]:offs[b]], offs[a:b + 1] - offs[a])
    a, b = dist.shard_range(rank, world, len(call_rdd))
    return call_rdd[a:b]


# --------------------------------------------------------------------------------------------- a5/a6
def center_matrix(sim_matrix, row_count):
    """center_matrix (variants_pca.py:84-121; VariantsPca.scala:199-223).
    sim_matrix: PcoaEngine (as returned above) or an N x N integer array.  Returns B (N x N fp64)."""
    eng = _as_engine(sim_matrix, row_count)
    b, _, _, _ = eng.center()
    return b


# --------------------------------------------------------------------------------------------- a7
def perform_pca(matrix, row_count, nr_principal_components=2):
    """perform_pca (variants_pca.py:123-152; VariantsPca.scala:224-227).  `matrix` is the engine
    holding S (centring is part of computePca on the device) or an N x N similarity array.
    Returns an N x k numpy array (unit-norm columns, sign-normalised)."""
    eng = _as_engine(matrix, row_count)
    comps, _, _ = eng.compute(nr_principal_components)
    return comps


def _as_engine(obj, row_count):
    if isinstance(obj, PcoaEngine):
        if obj.n != row_count:
            raise ValueError("row_count %d does not match the engine's N = %d" % (row_count, obj.n))
        return obj
    eng = PcoaEngine(row_count)
    eng.load_gram(np.asarray(obj))
    return eng


# --------------------------------------------------------------------------------------------- outlier rounds
def outlier_rule(components, sigma):
    """The outlier rule of --outlier-iterations (the compiled host restates it): `components` is [num_pc][n], the principal
    components of the current cohort.  Per axis c: mean_c = (sum of the n entries) / n and sd_c = sqrt((sum of the squared
    deviations from mean_c) / n), the POPULATION standard deviation, both sums added left to right in double (cumsum adds in
    order; numpy's sum adds pairwise).  Sample i is removed if |u_c[i] - mean_c| > sigma * sd_c on any axis with sd_c > 0.
    Returns a bool array of n entries, True = removed."""
    u = np.asarray(components, dtype=np.float64)
    if u.ndim != 2:
        raise ValueError("components must be [num_pc][n]")
    n = u.shape[1]
    removed = np.zeros(n, dtype=bool)
    for c in range(u.shape[0]):
        mean = np.cumsum(u[c])[-1] / n
        dev = u[c] - mean
        sd = np.sqrt(np.cumsum(dev * dev)[-1] / n)
        if sd > 0:
            removed |= np.abs(dev) > sigma * sd
    return removed


def min_cohort(num_pc):
    """The smallest cohort an outlier round may leave behind."""
    return max(3, int(num_pc) + 1)


# --------------------------------------------------------------------------------------------- related pairs
PAIR_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("shared", np.int64)])   # pcoa_pair (include/pcoa.h)


def related_pairs_rule(s, x):
    """The rule of --related-min-jaccard and of pcoa_similar_pairs (the library and the compiled host restate it): `s` is the
    N x N similarity matrix, d_i = s[i, i] the number of variants sample i carries, s[i, j] the number two samples share and
    U = d_i + d_j - s[i, j] the number either carries.  The pair (i, j), i < j, is reported iff U > 0 and
    float64(s[i, j]) >= x * float64(U): one multiplication and one comparison in double, every integer below 2^53 -- the
    Jaccard index of the carrier sets against the threshold x without a division.  Returns the reported pairs in increasing
    (i, j) order as a structured array with the fields i, j, shared."""
    s = np.asarray(s, dtype=np.int64)
    if s.ndim != 2 or s.shape[0] != s.shape[1]:
        raise ValueError("s must be N x N")
    d = np.diagonal(s)
    u = d[:, None] + d[None, :] - s
    hit = (u > 0) & (s.astype(np.float64) >= np.float64(x) * u.astype(np.float64))
    hit &= np.triu(np.ones(s.shape, dtype=bool), 1)
    i, j = np.nonzero(hit)                      # row-major: increasing (i, j)
    out = np.zeros(i.size, dtype=PAIR_DTYPE)
    out["i"], out["j"], out["shared"] = i, j, s[i, j]
    return out


def related_removal(pairs, n):
    """The removal rule of --remove-related (the compiled host restates it): `pairs` are the reported pairs (a structured
    array with the fields i and j, or any sequence of (i, j)) among n samples.  While any pair has both samples still kept,
    the kept sample with the most kept partners is removed; a tie goes to the highest index; the partners' counts are
    updated and the step repeats.  Returns the removed samples as a sorted int64 array; it depends on the set of pairs only,
    not on their order."""
    if isinstance(pairs, np.ndarray) and pairs.dtype.names:
        edges = zip(pairs["i"].tolist(), pairs["j"].tolist())
    else:
        edges = [(int(a), int(b)) for a, b in pairs]
    partners = [set() for _ in range(n)]
    for a, b in edges:
        if not (0 <= a < n and 0 <= b < n) or a == b:
            raise ValueError("a pair names a sample outside [0, %d) or the same sample twice" % n)
        partners[a].add(b)
        partners[b].add(a)
    degree = np.array([len(p) for p in partners], dtype=np.int64)
    removed = []
    while n > 0 and degree.max() > 0:
        v = int(np.nonzero(degree == degree.max())[0][-1])
        removed.append(v)
        for w in partners[v]:
            partners[w].discard(v)
            degree[w] -= 1
        partners[v] = set()
        degree[v] = 0
    return np.array(sorted(removed), dtype=np.int64)


# --------------------------------------------------------------------------------------------- KING-robust kinship
KING_PLANES = ("het", "missing", "het_or_missing", "hom_a1", "hom_a2")   # PCOA_KING_HET .. PCOA_KING_HOM_A2 = 0 .. 4 (include/pcoa.h)
KING_PAIR_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("hethet", np.int64), ("ibs0", np.int64),
                            ("het_sum", np.int64)])                      # pcoa_king_pair


def king_planes(code):
    """The five genotype-class planes of --king-cutoff and of pcoa_accumulate_plink_bed_king (csrc/king.hip restates the decode
    on the device): `code` is [V][N] uint8 of PLINK .bed codes, 0 = 00 hom A1 (R), 1 = 01 missing (M), 2 = 10 het (H),
    3 = 11 hom A2 (A).  Returns five bool arrays [V][N] in the order of KING_PLANES: H, M, H u M, R, A."""
    code = np.asarray(code, dtype=np.uint8)
    if code.ndim != 2 or code.size and int(code.max()) > 3:
        raise ValueError("code must be [V][N] with values 0 .. 3")
    het, mis = code == 2, code == 1
    return het, mis, het | mis, code == 0, code == 3


def king_counts(grams):
    """The integer counts of the KING-robust rule from the five N x N Gram matrices of the planes, G_p = X_p^T X_p in the order
    of KING_PLANES; lower-case letters are diagonals (h_i = G_H[i, i], ...):
      V        = r_i + a_i + hm_i                                   the same for every i
      hethet   = G_H[i, j]                                          both heterozygous
      s_hm     = G_HM[i, j] - G_H[i, j] - G_M[i, j]                 one het, the other missing (H and M are disjoint)
      het_sum  = h_i + h_j - s_hm                                   hets of i where j is called + hets of j where i is called
      ibs0     = (V - hm_i - hm_j + G_HM[i, j]) - G_R[i, j] - G_A[i, j]     opposite homozygotes
    Returns (V, h, hethet, ibs0, het_sum), all int64.  The planes were not built from the same codes if V differs between the
    samples or some ibs0, het_sum or s_hm off the diagonal is negative: ValueError naming the check (pcoa_king_pairs reports
    the same four as PCOA_ERR_INVALID_ARG)."""
    g = [np.asarray(m, dtype=np.int64) for m in grams]
    if len(g) != len(KING_PLANES) or g[0].ndim != 2 or g[0].shape[0] != g[0].shape[1] or any(m.shape != g[0].shape for m in g):
        raise ValueError("grams must be five N x N matrices")
    gh, gm, ghm, gr, ga = g
    h, hm = np.diagonal(gh), np.diagonal(ghm)
    vs = np.diagonal(gr) + np.diagonal(ga) + hm
    if vs.size and (vs != vs[0]).any():
        raise ValueError("the planes were not fed the same rows: V = r_i + a_i + hm_i is not the same for every sample")
    v = int(vs[0]) if vs.size else 0
    s_hm = ghm - gh - gm
    het_sum = h[:, None] + h[None, :] - s_hm
    ibs0 = (v - hm[:, None] - hm[None, :] + ghm) - gr - ga
    off = ~np.eye(gh.shape[0], dtype=bool)
    for name, m in (("ibs0", ibs0), ("het_sum", het_sum), ("s_hm", s_hm)):
        if (m[off] < 0).any():
            raise ValueError("the planes were not fed the same rows: %s < 0 for some pair" % name)
    return v, h.copy(), gh.copy(), ibs0, het_sum


def king_pairs_rule(grams, x):
    """The rule of --king-cutoff and of pcoa_king_pairs (the library and the compiled host restate it): with the counts of
    king_counts and num = hethet - 2 ibs0 (int64, may be negative), the pair (i, j), i < j, is reported iff het_sum > 0 and
    float64(num) >= x * float64(het_sum): one multiplication and one comparison in double, every integer below 2^53 -- the
    KING-robust kinship num / het_sum over the jointly called sites against the threshold x without a division.  Returns the
    reported pairs in increasing (i, j) order as a structured array KING_PAIR_DTYPE."""
    _, _, hethet, ibs0, het_sum = king_counts(grams)
    num = hethet - 2 * ibs0
    hit = (het_sum > 0) & (num.astype(np.float64) >= np.float64(x) * het_sum.astype(np.float64))
    hit &= np.triu(np.ones(hethet.shape, dtype=bool), 1)
    i, j = np.nonzero(hit)                      # row-major: increasing (i, j)
    out = np.zeros(i.size, dtype=KING_PAIR_DTYPE)
    out["i"], out["j"], out["hethet"], out["ibs0"], out["het_sum"] = i, j, hethet[i, j], ibs0[i, j], het_sum[i, j]
    return out


def king_kinship(pairs):
    """float64(hethet - 2 ibs0) / float64(het_sum) of reported pairs: what the hosts print."""
    return (pairs["hethet"] - 2 * pairs["ibs0"]).astype(np.float64) / pairs["het_sum"].astype(np.float64)


def grm_king_rule(codes, counted=None):
    """The counts of pcoa_grm_king_block (include/pcoa.h; csrc/grm_king.hip restates them on the matrix cores): `codes` is
    [V][N] of 2-bit codes, 1 = not called (M), 2 = heterozygous (H), 0 and 3 the two homozygotes (R, A) -- .bed codes or the
    store's, the rule is symmetric in the homozygotes -- and `counted` a [V] mask of the counted rows (None: all).  With
    C = R u H u A, over the counted rows:
      hethet[i, j]  = sum_v H_vi H_vj
      ibs0[i, j]    = sum_v (R_vi A_vj + A_vi R_vj)
      het_sum[i, j] = sum_v (H_vi C_vj + C_vi H_vj)
    Returns (hethet, ibs0, het_sum), int64 [N][N], diagonal included (h_i, 0, 2 h_i).  Off the diagonal they are king_counts'
    integers from the five plane Grams of the same codes."""
    codes = np.asarray(codes, dtype=np.uint8)
    if codes.ndim != 2 or codes.size and int(codes.max()) > 3:
        raise ValueError("codes must be [V][N] with values 0 .. 3")
    if counted is not None:
        counted = np.asarray(counted).astype(bool)
        if counted.shape != (codes.shape[0],):
            raise ValueError("counted must be one flag per row of codes")
        codes = codes[counted]
    h = (codes == 2).astype(np.float64)            # 0 / 1 sums in float64: exact far beyond any V, and BLAS does them
    r = (codes == 0).astype(np.float64)
    a = (codes == 3).astype(np.float64)
    c = h + r + a
    hc = (h.T @ c).astype(np.int64)
    ra = (r.T @ a).astype(np.int64)
    return (h.T @ h).astype(np.int64), ra + ra.T, hc + hc.T


def grm_king_pairs_rule(codes, x, counted=None):
    """The rule of --grm-king-cutoff and of pcoa_grm_king_pairs: with the counts of grm_king_rule and num = hethet - 2 ibs0, the
    pair (i, j), i < j, is reported iff het_sum > 0 and float64(num) >= x * float64(het_sum) -- king_pairs_rule's comparison on
    the same integers.  Returns the reported pairs in increasing (i, j) order as KING_PAIR_DTYPE."""
    hethet, ibs0, het_sum = grm_king_rule(codes, counted)
    num = hethet - 2 * ibs0
    hit = (het_sum > 0) & (num.astype(np.float64) >= np.float64(x) * het_sum.astype(np.float64))
    hit &= np.triu(np.ones(hethet.shape, dtype=bool), 1)
    i, j = np.nonzero(hit)                      # row-major: increasing (i, j)
    out = np.zeros(i.size, dtype=KING_PAIR_DTYPE)
    out["i"], out["j"], out["hethet"], out["ibs0"], out["het_sum"] = i, j, hethet[i, j], ibs0[i, j], het_sum[i, j]
    return out


# --------------------------------------------------------------------------------------------- similarity measures
SIMILARITY_MEASURES =("shared", "jaccard", "cosine")   # PCOA_SIMILARITY_SHARED / _JACCARD / _COSINE = 0 / 1 / 2 (include/pcoa.h)


def similarity_measure(s, kind):
    """The rule of --similarity-measure and of pcoa_set_similarity (csrc/measure.hip restates it on the device): `s` is the
    N x N integer matrix of TOTAL entries (the int32 matrix plus the int64 part where the engine has one), d = diag(s) the
    number of variants each sample carries.  Returns K as float64:
      shared   K = float64(s)
      jaccard  U = d_i + d_j - s_ij as an integer;  K_ij = float64(s_ij) / float64(U) where U > 0, else 0.0 -- one division.
               The diagonal follows from the formula: 1 where d_i > 0, 0 for a sample that carries nothing.  (With carrier
               multiplicities s_ij <= (d_i + d_j) / 2 by Cauchy-Schwarz, so U >= 0, and U = 0 only when both samples are empty.)
      cosine   q_i = 1.0 / sqrt(float64(d_i)) where d_i > 0, else 0.0;  K_ij = (float64(s_ij) * q_i) * q_j, in this order
               (Ochiai): no division or square root per entry.
    Every operation is one IEEE fp64 operation (numpy fuses nothing)."""
    s = np.asarray(s, dtype=np.int64)
    if s.ndim != 2 or s.shape[0] != s.shape[1]:
        raise ValueError("s must be N x N")
    if kind not in SIMILARITY_MEASURES:
        raise ValueError("kind must be one of %s, not %r" % (", ".join(SIMILARITY_MEASURES), kind))
    sd = s.astype(np.float64)
    if kind == "shared":
        return sd
    d = np.diagonal(s)
    if kind == "jaccard":
        u = d[:, None] + d[None, :] - s
        k = np.zeros(s.shape, dtype=np.float64)
        np.divide(sd, u.astype(np.float64), out=k, where=u > 0)
        return k
    q = np.zeros(d.shape, dtype=np.float64)
    np.divide(1.0, np.sqrt(d.astype(np.float64), where=d > 0, out=np.ones(d.shape, dtype=np.float64)), out=q, where=d > 0)
    return (sd * q[:, None]) * q[None, :]


MISSING_CALLS = ("ignore", "pairwise")   # --missing-calls


def call_complete_measure(s, q, n_variants):
    """The rule of --missing-calls pairwise and of pcoa_set_call_companion (csrc/complete.hip restates it on the device): `s`
    is the N x N integer matrix of TOTAL entries of the carrier engine, `q` the Gram matrix of the missing-call bitsets (the
    companion's S), n_variants = V the number of variants fed.  With c_i = V - q_ii the variants at which sample i is called
    and M_ij = c_i + c_j - V + q_ij the variants at which both are (integers), K_ij = float64(s_ij) / float64(M_ij) where
    M_ij > 0, else 0.0 -- one IEEE fp64 division.  Returns K as float64.  K need not be positive semi-definite."""
    s = np.asarray(s, dtype=np.int64)
    q = np.asarray(q, dtype=np.int64)
    if s.ndim != 2 or s.shape[0] != s.shape[1] or q.shape != s.shape:
        raise ValueError("s and q must be N x N")
    v = int(n_variants)
    c = v - np.diagonal(q)
    if v < 0 or (c < 0).any():
        raise ValueError("n_variants is smaller than a sample's missing count")
    m = c[:, None] + c[None, :] - v + q
    k = np.zeros(s.shape, dtype=np.float64)
    np.divide(s.astype(np.float64), m.astype(np.float64), out=k, where=m > 0)
    return k


def centred_measure(k):
    """computePca's centring (VariantsPca.scala:206-221) of a similarity K in float64: r_i = sum_j K_ij, rowmean_i = r_i / N,
    mm = (sum_i r_i) / N / N (the two divisions the device's stats kernel performs), B_ij = ((K_ij - rowmean_i) - rowmean_j)
    + mm.  Returns (B, r, mm, nonzero_rows) with nonzero_rows = #{i : r_i > 0} -- for the Jaccard and cosine measures the
    count of d_i > 0, the number the shared measure prints.  The dtype of k is kept (float64, or longdouble for a reference)."""
    k = np.asarray(k)
    if k.dtype not in (np.float64, np.longdouble):
        k = k.astype(np.float64)
    n = k.shape[0]
    r = k.sum(axis=1)
    nn = k.dtype.type(n)
    rowmean = r / nn
    mm = r.sum() / nn / nn
    b = ((k - rowmean[:, None]) - rowmean[None, :]) + mm
    return b, r, mm, int(np.count_nonzero(r > 0))


# --------------------------------------------------------------------------------------------- conf
class PcaConf(object):
    """Flags of PcaConf / GenomicsConf (GenomicsConf.scala:31-101), same names and defaults.
    Spark- and cloud-specific flags are accepted and ignored; --input-path names a local dataset
    (the Genomics API the reference streamed from no longer exists)."""

    def __init__(self, arguments):
        p = argparse.ArgumentParser(prog="VariantsPcaDriver", description=self.__doc__)
        p.add_argument("--bases-per-partition", type=int, default=1000000)
        p.add_argument("--client-secrets", type=str, default=None)
        p.add_argument("--input-path", type=str, nargs="*", default=None,
                       help="one local dataset per variant set: .npz (callset_ids, [callset_names], sample_idx, "
                            "row_offsets) or .vcf[.gz]; two files are joined, three or more merged "
                            "(VariantsPca.scala:153-162)")
        p.add_argument("--num-reduce-partitions", type=int, default=10)
        p.add_argument("--output-path", type=str, default=None)
        p.add_argument("--references", type=str, nargs="*", default=["chr17:41196311:41277499"])
        p.add_argument("--spark-master", type=str, default=None)
        p.add_argument("--variant-set-id", type=str, nargs="*", default=["3049512673186936334"])
        p.add_argument("--all-references", action="store_true")
        p.add_argument("--debug-datasets", action="store_true")
        p.add_argument("--min-allele-frequency", type=float, default=None)
        p.add_argument("--num-pc", type=int, default=2)
        # additions of this engine
        p.add_argument("--synthetic", type=str, default=None, help="V,N,seed: synthetic Balding-Nichols input")
        p.add_argument("--gpu", type=int, default=0)
        p.add_argument("--gpus", type=int, default=1,
                       help="K > 1: one process per GPU (started here through torch.distributed.run unless a launcher already "
                            "did), the variants partitioned into K contiguous shards, one RCCL all-reduce of the partial "
                            "similarity matrices (reduceByKey, VariantsPca.scala:190), computePca and the output on rank 0")
        p.add_argument("--dist-backend", choices=["nccl", "gloo"], default="nccl",
                       help="--gpus K: torch.distributed backend of the rendezvous (nccl = RCCL; gloo = CPU wire, for boxes where "
                            "several ranks have to share one GPU -- it implies --allreduce torch)")
        p.add_argument("--rank-devices", type=str, default=None,
                       help="--gpus K: device ordinal of each rank, comma-separated (default: rank r on GPU r); ordinals may repeat "
                            "with --dist-backend gloo (how the path is tested on a one-GPU box)")
        p.add_argument("--allreduce", choices=["native", "torch"], default="native",
                       help="--gpus K: native = the library's RCCL communicator (in place on the int32 partial), torch = "
                            "export -> torch.distributed.all_reduce -> import")
        p.add_argument("--plink-ref-allele", choices=["a1", "a2"], default="a2",
                       help="PLINK filesets: which .bim allele column is the reference allele (a2: written with "
                            "--keep-allele-order / plink2 --make-bed; a1: the other way round)")
        p.add_argument("--spark-output-layout", action="store_true",
                       help="write <output-path>-pca.tsv as the DIRECTORY Spark's saveAsTextFile leaves (part-00000 + _SUCCESS, "
                            "VariantsPca.scala:241-245) instead of one file of that name")
        p.add_argument("--layout", choices=["auto", "full", "strips"], default="auto",
                       help="full: every rank a whole partial S over its share of the variants, then the all-reduce; strips: "
                            "rank r owns the columns strip_ranges(N, K)[r] of S and reads every variant, nothing is reduced; "
                            "auto: strips only when K > 1 and S does not fit (pcoa_plan_layout)")
        p.add_argument("--gram", choices=["stored", "implicit"], default="stored",
                       help="stored: the N x N similarity matrix is accumulated and decomposed; implicit: one operator engine "
                            "(pcoa_create_operator) keeps the carrier bitsets and computePca runs over the products "
                            "S v = X^T (X v), no N x N matrix exists.  One GPU, full layout; there is no auto: which form is "
                            "faster at which N has not been measured")
        p.add_argument("--grm", action="store_true",
                       help="standardised-genotype PCA: one GRM engine (pcoa_create_grm) keeps the 2-bit genotypes of ONE PLINK "
                            "fileset and computePca decomposes K = Z^T Z / M over allele-frequency-standardised dosages, missing "
                            "calls mean-imputed (the matrix of smartpca, plink --pca, GCTA, flashpca), through the products K x; "
                            "no N x N matrix exists.  One GPU")
        p.add_argument("--grm-min-maf", type=float, default=None,
                       help="--grm: use only variants whose minor-allele frequency among the called samples is at least this, "
                            "in [0, 0.5) (default 0)")
        p.add_argument("--grm-geno", type=float, default=None,
                       help="--grm: use only variants whose share of missing calls among the samples is at most this, in [0, 1] "
                            "(plink --geno; pcoa_grm_set_variant_filters; default 1 = off)")
        p.add_argument("--grm-hwe", type=float, default=None,
                       help="--grm: use only variants whose Hardy-Weinberg exact-test p-value (Wigginton et al. 2005, no mid-p) is at "
                            "least this, in [0, 1) (plink --hwe; default 0 = off)")
        p.add_argument("--grm-mind", type=float, default=None,
                       help="--grm: take out, before anything else, the samples whose share of missing calls over the fileset's "
                            "variants exceeds this, in [0, 1] (plink --mind; pcoa_grm_sample_counts, pcoa_create_grm_subset); they "
                            "are not placed by --grm-project-removed, unless --grm-project-lsq is given")
        p.add_argument("--grm-variant-qc-output-path", type=str, default=None,
                       help="--grm: one line per variant of the fileset: index, contig, position, id, called, het, hom-alt, missing "
                            "share, HWE p, 1 (used under --grm-min-maf / --grm-geno / --grm-hwe) or 0")
        p.add_argument("--grm-sample-qc-output-path", type=str, default=None,
                       help="--grm: one line per sample of the fileset, before --grm-mind removes anyone: name, called, het, hom-alt, "
                            "call rate, het share of called, 1 (kept) or 0")
        p.add_argument("--grm-weights-output-path", type=str, default=None,
                       help="--grm: write the SNP weight of every variant of the fileset on each of the --num-pc axes of K "
                            "(pcoa_grm_weights: the left singular vectors of the standardised genotype matrix; smartpca's "
                            "snpweightoutname, plink2's --pca var-wts) to this file, in the format of --loadings-output-path; a "
                            "variant that is not used (monomorphic, never called, below --grm-min-maf) prints 0.0")
        p.add_argument("--grm-project-path", type=str, default=None,
                       help="--grm: a second PLINK fileset (the study) whose samples are placed onto the axes of the --input-path "
                            "panel without moving them (pcoa_grm_project): the panel's allele frequencies standardise the "
                            "study's genotypes, a missing call contributes nothing.  Its .bim must equal the panel's line by "
                            "line (contig, id, position, both alleles); its rows are emitted after the panel's")
        p.add_argument("--grm-output-path", type=str, default=None,
                       help="--grm: write the matrix computePca decomposed, read out of the engine band by band "
                            "(pcoa_grm_block), as PREFIX.grm.bin (float32, lower triangle with the diagonal, row by row), "
                            "PREFIX.grm.N.bin (the jointly called used variants of each pair, float32, same order) and "
                            "PREFIX.grm.id (set id <tab> sample name per row): the layout GCTA and PLINK read")
        p.add_argument("--grm-ld-window", type=int, default=0,
                       help="--grm: LD-prune the resident genotype store before computePca (pcoa_grm_ld_prune): forward and "
                            "greedy in feed order, a used variant is removed when a KEPT variant among the W rows before it, on "
                            "the same contig, has r^2 of the DOSAGES over the jointly called samples (the pair statistic of "
                            "plink --indep-pairwise; the earlier kept variant wins, there is no step and no MAF order) above "
                            "--grm-ld-r2.  0: off; at most %d" % LD_MAX_WINDOW)
        p.add_argument("--grm-ld-r2", type=float, default=None,
                       help="the r^2 threshold of --grm-ld-window, in [0, 1] (default %g, as --ld-r2)" % LD_DEFAULT_R2)
        p.add_argument("--grm-ld-output-path", type=str, default=None,
                       help="--grm-ld-window: one line per variant of the store in feed order -- 0-based index, contig, "
                            "position, variant id, 1 (kept) or 0, tab-separated (the columns of --ld-output-path)")
        p.add_argument("--grm-keep-samples", type=str, default=None,
                       help="--grm: a file with one sample name per line (the names of PREFIX.grm.id's second column): the "
                            "fileset is streamed once into the engine and the PCA runs on these samples only, on the engine's "
                            "subset over them (pcoa_create_grm_subset: one gather of the 2-bit store; the allele frequencies are "
                            "those of the kept samples).  Excludes --grm-remove-samples")
        p.add_argument("--grm-remove-samples", type=str, default=None,
                       help="--grm: as --grm-keep-samples, the file names the samples that are taken out")
        p.add_argument("--grm-outlier-iterations", type=int, default=0,
                       help="--grm: K > 0: up to K rounds of outlier removal around computePca (smartpca's loop, the rule of "
                            "--outlier-iterations): the engine is replaced by its subset over the kept samples, whose allele "
                            "frequencies standardise the next round; --grm-ld-window prunes every round's engine again.  Rows "
                            "go out for the kept samples only")
        p.add_argument("--grm-outlier-sigma", type=float, default=None,
                       help="--grm-outlier-iterations: the threshold, in population standard deviations of an axis (default %g)"
                            % GRM_OUTLIER_SIGMA)
        p.add_argument("--grm-project-removed", action="store_true",
                       help="--grm: every sample a list or an outlier round removed is placed on the final axes "
                            "(pcoa_grm_project over a study subset of the whole fileset's engine); its rows follow the kept samples'")
        p.add_argument("--grm-project-lsq", action="store_true",
                       help="--grm-project-path / --grm-project-removed: place every sample by least squares over the used "
                            "variants it is called at (pcoa_grm_project_lsq, smartpca's lsqproject), not by mean imputation, "
                            "which shrinks a sparsely called sample towards the origin; --grm-project-removed then places the "
                            "samples --grm-mind took out too; at most %d principal components" % GRM_LSQ_MAX_PC)
        p.add_argument("--grm-cutoff", type=float, default=None,
                       help="--grm: X: screen K for related sample pairs before computePca (pcoa_grm_pairs: gcta --grm-cutoff, "
                            "plink --rel-cutoff): a pair is reported when K(i, j) >= X, K as --grm-output-path writes it, after "
                            "--grm-keep-samples / --grm-remove-samples and one --grm-ld-window prune; no N x N matrix leaves the device")
        p.add_argument("--grm-cutoff-divisor", type=str, default=None,
                       help="--grm-cutoff: used (default): num / M', the K that is decomposed; pairwise: num / n(i, j)")
        p.add_argument("--grm-related-output-path", type=str, default=None,
                       help="--grm-cutoff: write the reported pairs to this file, one line per pair in (i, j) order: "
                            "name_i, name_j, K, n")
        p.add_argument("--grm-cutoff-remove", action="store_true",
                       help="--grm-cutoff: drop one sample of every reported pair (the rule of --remove-related) and go on with "
                            "the engine's subset over the rest; --grm-project-removed places the dropped samples too")
        p.add_argument("--grm-king-cutoff", type=float, default=None,
                       help="--grm: X in (0, 0.5]: screen the genotype store for relatives by the KING-robust kinship coefficient "
                            "before computePca (pcoa_grm_king_pairs: plink2 --king-cutoff), where --grm-cutoff runs: a pair is "
                            "reported when (hethet - 2 ibs0) / het_sum over the counted variants is at least X.  It does not depend "
                            "on allele frequencies, so it holds on a cohort with population structure where --grm-cutoff does "
                            "not; no plane engines, no N x N matrix, no second pass over the fileset")
        p.add_argument("--grm-king-rows", type=str, default=None,
                       help="--grm-king-cutoff: used (default): the variants used under the min MAF, --grm-geno, --grm-hwe and the "
                            "--grm-ld-window prune; all: every variant of the fileset")
        p.add_argument("--grm-king-output-path", type=str, default=None,
                       help="--grm-king-cutoff: write the reported pairs to this file in the format of --king-output-path")
        p.add_argument("--grm-king-max-pairs", type=int, default=None,
                       help="--grm-king-cutoff: the most pairs the job takes from the library (default 1048576); if more are "
                            "reported the job stops")
        p.add_argument("--grm-king-remove", action="store_true",
                       help="--grm-king-cutoff: drop one sample of every reported pair (the rule of --remove-related) and go on "
                            "with the engine's subset over the rest; --grm-project-removed places the dropped samples too")
        p.add_argument("--grm-pcrelate-output-path", type=str, default=None,
                       help="--grm: estimate PC-Relate kinship (pcoa_grm_pcrelate_*: kinship adjusted for the ancestry the axes "
                            "found) behind the last computePca and --grm-project-removed, over the final cohort and the placed "
                            "removed samples, and write the pairs at or above --grm-pcrelate-cutoff to this file: name_i, name_j, "
                            "kinship, n")
        p.add_argument("--grm-pcrelate-pcs", type=int, default=None,
                       help="--grm-pcrelate-output-path: the axes beside the intercept, in [1, min(8, --num-pc)] (default min(2, --num-pc))")
        p.add_argument("--grm-pcrelate-cutoff", type=float, default=None,
                       help="--grm-pcrelate-output-path: report the pairs with kinship at or above this (default 2^-4.5)")
        p.add_argument("--grm-pcrelate-maf-threshold", type=float, default=None,
                       help="--grm-pcrelate-output-path: a genotype counts where the individual's own allele frequency lies inside "
                            "(T, 1 - T), T in [0, 0.5) (default 0.01)")
        p.add_argument("--grm-pcrelate-inbreeding-output-path", type=str, default=None,
                       help="--grm-pcrelate-output-path: write name, f = 2 phi(i, i) - 1 and n(i, i) of every sample to this file")
        p.add_argument("--grm-pcrelate-max-pairs", type=int, default=None,
                       help="--grm-pcrelate-output-path: the most pairs the job takes from the library (default 1048576); if more "
                            "are reported the job stops")
        p.add_argument("--grm-output-divisor", type=str, default=None,
                       help="--grm-output-path: used (default): num / M', the mean-imputed K that is decomposed; pairwise: "
                            "num / n(i, j), the pairwise-complete estimator GCTA-style tools store")
        p.add_argument("--dump-similarity", type=str, default=None,
                       help="write S (N x N int64, little-endian, row-major) to this file (parity tests)")
        p.add_argument("--project-input-path", type=str, nargs="+", default=None,
                       help="VCFs whose samples are placed onto the principal coordinates of the --input-path cohort "
                            "(pcoa_project) instead of decomposing the union: their callsets follow the reference's, variants "
                            "are matched by the join / merge of all sets; one GPU, VCF inputs, full layout")
        p.add_argument("--outlier-iterations", type=int, default=0,
                       help="K > 0: up to K rounds of outlier removal around computePca (smartpca's loop): samples further than "
                            "--outlier-sigma standard deviations from the mean of a principal component are removed and "
                            "computePca runs again on S[kept, kept], gathered on the device (pcoa_create_subset) -- no variant "
                            "is read twice.  Rows go out for the kept samples only.  One full engine: stored S, full layout")
        p.add_argument("--outlier-sigma", type=float, default=6.0,
                       help="--outlier-iterations: the threshold, in population standard deviations of an axis")
        p.add_argument("--related-min-jaccard", type=float, default=None,
                       help="X in (0, 1]: screen S for duplicate and related sample pairs before computePca "
                            "(pcoa_similar_pairs): a pair is reported when the Jaccard index of the two carrier sets, "
                            "S(i, j) / (S(i, i) + S(j, j) - S(i, j)), is at least X.  Off by default.  One full engine: stored S, "
                            "full layout")
        p.add_argument("--related-output-path", type=str, default=None,
                       help="--related-min-jaccard: write the reported pairs to this file, one line per pair in (i, j) order: "
                            "name_i, name_j, shared, d_i, d_j, jaccard (tab-separated, one header line)")
        p.add_argument("--related-max-pairs", type=int, default=None,
                       help="--related-min-jaccard: the most pairs the job takes from the library (default 1048576); if more "
                            "are reported the job stops")
        p.add_argument("--remove-related", action="store_true",
                       help="--related-min-jaccard: drop one sample of every reported pair before computePca (the sample with "
                            "the most reported partners first, ties to the highest index) and decompose S[kept, kept], "
                            "gathered on the device (pcoa_create_subset) -- no variant is read twice")
        p.add_argument("--king-cutoff", type=float, default=None,
                       help="X in (0, 0.5]: screen the cohort for relatives by the KING-robust kinship coefficient before "
                            "computePca (pcoa_king_pairs): a pair is reported when (hethet - 2 ibs0) / het_sum over the jointly "
                            "called variants is at least X (0.177: first degree).  It does not depend on allele frequencies, "
                            "so it holds on a cohort with population structure where --related-min-jaccard does not.  Off by "
                            "default.  One PLINK fileset, one device: stored S, full layout, five more N x N int32 matrices")
        p.add_argument("--king-output-path", type=str, default=None,
                       help="--king-cutoff: write the reported pairs to this file, one line per pair in (i, j) order: "
                            "name_i, name_j, hethet, ibs0, het_sum, kinship (tab-separated, one header line)")
        p.add_argument("--king-max-pairs", type=int, default=None,
                       help="--king-cutoff: the most pairs the job takes from the library (default 1048576); if more are "
                            "reported the job stops")
        p.add_argument("--king-remove", action="store_true",
                       help="--king-cutoff: drop one sample of every reported pair before computePca (the rule of "
                            "--remove-related) and decompose S[kept, kept], gathered on the device (pcoa_create_subset)")
        p.add_argument("--similarity-measure", type=str, default="shared",
                       help="shared|jaccard|cosine: what computePca decomposes (pcoa_set_similarity).  shared: the counts S, as "
                            "the reference; jaccard: S(i, j) / (S(i, i) + S(j, j) - S(i, j)); cosine: S(i, j) / sqrt(S(i, i) "
                            "S(j, j)) -- evaluated on the fly from S on the device, which takes out the axis that tracks how "
                            "many variants a sample carries.  One full engine: stored S, full layout, no projection")
        p.add_argument("--missing-calls", type=str, default="ignore",
                       help="ignore|pairwise: what a missing call (PLINK .bed code 01) means.  ignore: a non-carrier, as the "
                            "reference; pairwise: computePca decomposes the pairwise-complete similarity S(i, j) / M(i, j), M the "
                            "number of variants at which both samples were called (pcoa_set_call_companion), which takes out "
                            "the axis that tracks a sample's call rate.  One PLINK fileset, one full engine: stored S, full "
                            "layout, --similarity-measure shared, no projection, loadings or LD pruning")
        p.add_argument("--call-rate-output-path", type=str, default=None,
                       help="--missing-calls pairwise: one line per sample -- name, called variants, variants fed, call rate "
                            "with six decimals, tab-separated")
        p.add_argument("--loadings-output-path", type=str, default=None,
                       help="write the loading of every variant fed to the engine on each of the --num-pc principal "
                            "coordinates, w_c = X (J u_c) / sqrt(lambda_c) (pcoa_loadings_*), to this file: one line per "
                            "variant in feed order -- 0-based index, contig, position, variant id, then the loadings, "
                            "tab-separated.  One engine, --similarity-measure shared, the whole cohort: stored S takes a second "
                            "pass over the variants, --gram implicit reads the resident store")
        p.add_argument("--ld-window", type=int, default=0,
                       help="LD pruning on the device in front of the accumulation (pcoa_ld_*): forward and greedy in feed order, "
                            "a variant is removed when it is monomorphic or when a KEPT variant among the W fed before it, on the "
                            "same contig, has r^2 of the carrier indicators above --ld-r2.  0: off.  One engine, one input set")
        p.add_argument("--ld-r2", type=float, default=None, help="the r^2 threshold of --ld-window, in [0, 1] (default 0.2)")
        p.add_argument("--ld-output-path", type=str, default=None,
                       help="--ld-window: one line per fed variant in feed order -- 0-based index, contig, position, variant id, "
                            "1 (kept) or 0, tab-separated")
        a = p.parse_args(list(arguments))
        self.__dict__.update(vars(a))
        self.numPc = a.num_pc
        self.outputPath = a.output_path
        self.inputPath = a.input_path
        self.minAlleleFrequency = a.min_allele_frequency
        self.related_max_pairs_given = a.related_max_pairs is not None
        if a.related_max_pairs is None:
            self.related_max_pairs = RELATED_MAX_PAIRS
        self.grm_king_max_pairs_given = a.grm_king_max_pairs is not None
        if a.grm_king_max_pairs is None:
            self.grm_king_max_pairs = RELATED_MAX_PAIRS
        self.grm_pcrelate_max_pairs_given = a.grm_pcrelate_max_pairs is not None
        if a.grm_pcrelate_max_pairs is None:
            self.grm_pcrelate_max_pairs = RELATED_MAX_PAIRS
        self.king_max_pairs_given = a.king_max_pairs is not None
        if a.king_max_pairs is None:
            self.king_max_pairs = RELATED_MAX_PAIRS


RELATED_MAX_PAIRS = 1 << 20   # default of --related-max-pairs
GRM_OUTLIER_SIGMA = 6.0       # default of --grm-outlier-sigma
GRM_MIN_COHORT = 32           # a GRM engine's computePca is the Lanczos iteration, which starts at 32 samples


def java_float_to_string(f):
    """Float.toString (the reference prints --min-allele-frequency, a Float, at VariantsPca.scala:99)."""
    f32 = np.float32(f)
    return java_double_to_string(float(f32), shortest=np.format_float_scientific(abs(f32), unique=True, trim="0"))


def java_double_to_string(d, shortest=None):
    """Double.toString, which the reference's string interpolation uses (VariantsPca.scala:239):
    decimal for 1e-3 <= |d| < 1e7, otherwise computerised scientific notation (1.0E-4).
    `shortest`: the shortest round-trip digits of |d| when they are not repr(double)'s (Float.toString)."""
    d = float(d)
    if d != d:
        return "NaN"
    if d in (float("inf"), float("-inf")):
        return "Infinity" if d > 0 else "-Infinity"
    if d == 0.0:
        return "-0.0" if str(d).startswith("-") else "0.0"
    r = shortest if shortest is not None else repr(abs(d))
    mant, _, exp = r.partition("e")
    e10 = int(exp) if exp else 0
    ip, _, fp = mant.partition(".")
    digits = (ip + fp).lstrip("0")
    # decimal exponent of the first significant digit
    if ip.strip("0"):
        e10 += len(ip.lstrip("0")) - 1
    else:
        e10 -= len(fp) - len(fp.lstrip("0")) + 1
    digits = digits.rstrip("0") or "0"
    sign = "-" if d < 0 else ""
    if 1e-3 <= abs(d) < 1e7:
        if e10 >= 0:
            whole = digits[:e10 + 1].ljust(e10 + 1, "0")
            frac = digits[e10 + 1:] or "0"
        else:
            whole = "0"
            frac = "0" * (-e10 - 1) + digits
        return "%s%s.%s" % (sign, whole, frac)
    return "%s%s.%sE%d" % (sign, digits[0], digits[1:] or "0", e10)


# --------------------------------------------------------------------------------------------- driver
def similarity_entries_nonzero(s):
    """RDD[((Int, Int), Int)] of getSimilarityMatrixStream (VariantsPca.scala:262-279) from a dense S: the keys whose
    count is non-zero, both triangles (the reference emits the pairs c1 <= c2 and mirrors the strict upper ones)."""
    s = np.asarray(s)
    rows, cols = np.nonzero(s)
    return [((int(i), int(j)), int(s[i, j])) for i, j in zip(rows, cols)]


class VariantsPcaDriver(object):
    """class VariantsPcaDriver (VariantsPca.scala:81-286) over a local dataset.

    indexes: callset id -> 0..N-1 in callset-list order, names: callset id -> name
    (VariantsCommon.scala:44-47; the ordering rule is preserved)."""

    def __init__(self, conf, indexes, names, data, matrix_size=None):
        self.conf = conf
        self.indexes = dict(indexes)
        self.names = dict(names)
        self.data = data  # list of datasets, each a list of variant dicts (or ('csr', idx, offs))
        print("Matrix size: %d." % (len(self.indexes) if matrix_size is None else matrix_size))  # VariantsCommon.scala:48
        self.engine = None
        self.gram_seconds_before = 0.0   # Gram kernel seconds of engines that --outlier-iterations / --remove-related have replaced
        self.kept = None                 # original indices of the current cohort once --remove-related has dropped samples

    # filterDataset, VariantsPca.scala:96-108
    def filterDataset(self, data):
        maf = self.conf.minAlleleFrequency
        if maf is None:
            return data
        if isinstance(data, tuple):
            # carrier-only inputs (.npz CSR, --synthetic) carry no INFO/AF: the filter cannot be applied, and ignoring
            # it silently would change the result
            raise ValueError("--min-allele-frequency needs variant records with INFO/AF (a VCF input), "
                             "not pre-extracted carriers (.npz / --synthetic)")
        print("Min allele frequency %s." % java_float_to_string(maf))
        out = []
        for variant in data:
            af = (variant.get("info") or {}).get("AF")
            if af is not None and len(af) > 0 and np.float32(af[0]) >= np.float32(maf):
                out.append(variant)
        return out

    # getCallsRdd, VariantsPca.scala:153-168
    def getCallsRdd(self, data, meta=None):
        """meta (--loadings-output-path): a list that receives (contig, position, id) of every row of the result built from
        variant RECORDS; the carrier-only inputs recorded theirs during ingest (load_dataset)."""
        variant_set_count = len(data)
        if variant_set_count == 1:
            d = data[0]
            if isinstance(d, tuple):  # pre-extracted carriers: CSR rows (already filtered) or bitsets
                if d[0] == "bed":
                    return d
                return ("bits", d[1]) if d[0] == "bits" else (d[1], d[2])
            return prepare_call_data(d, self.indexes, meta)
        if any(isinstance(d, tuple) for d in data):
            raise ValueError("joining datasets needs variant records (contig/start/end/ref/alt), not CSR carriers")
        joined_meta = [] if meta is not None else None
        if variant_set_count == 2:
            callsets = join_datasets(data, self.indexes, self.conf.debug_datasets, joined_meta)
        else:
            callsets = merge_datasets(data, variant_set_count, self.indexes, joined_meta)
        out = []
        for k, calls in enumerate(callsets):  # :164-167
            kept = [idx for (has_variation, idx) in calls if has_variation]
            if len(kept) > 0:
                out.append(kept)
                if meta is not None:
                    meta.append(joined_meta[k])
        return out

    # getSimilarityMatrix, VariantsPca.scala:182-191
    def getSimilarityMatrix(self, callsets):
        self.engine = calculate_similarity_matrix(callsets, len(self.indexes), device=self.conf.gpu)
        return self.engine

    # the same with the reference's parallel strategy (:184-190): this rank's partition of the variants on this rank's GPU,
    # then the sum of the partial matrices over the ranks (reduceByKey(_ + _, numReducePartitions)).  Every rank ends up
    # with the whole S.  Returns (engine, telemetry).
    def getSimilarityMatrixSharded(self, callsets, rank, world, device, allreduce="native"):
        import time
        from . import dist
        shard = shard_calls(callsets, rank, world)
        t0 = time.perf_counter()
        self.engine = calculate_similarity_matrix(shard, len(self.indexes), device=device)
        self.engine.sync()
        t_local = time.perf_counter() - t0
        native = None
        if allreduce == "native":
            native = dist.NativeComm(self.engine)
        t1 = time.perf_counter()
        if native is not None:
            native.allreduce()
            self.engine.sync()
        else:
            dist.allreduce_engine(self.engine)
        t_red = time.perf_counter() - t1
        tele = dist.collective_telemetry(t_local, t_red, self.engine.timings(), native.count() if native is not None else None)
        if native is not None:
            native.close()
        return self.engine, tele

    # the strip layout (pcoa_plan_layout): this rank owns S[:, col0:col0+cols] and is fed EVERY variant (no shard_calls);
    # nothing is reduced.  Returns the owner.
    def getSimilarityMatrixStrip(self, callsets, strip, device):
        self.engine = calculate_similarity_matrix(callsets, len(self.indexes), engine=PcoaEngine(len(self.indexes), device=device,
                                                                                                 strip=strip))
        return self.engine

    # computePca over the strips of all ranks (every rank calls it: the exchange is collective).  One process:
    # pcoa_compute_strips; several: strips.compute_pca_over_strips over the process group (host vectors over gloo).
    def computePcaOverStrips(self, owner, world, host_exchange=False):
        from . import engine as E
        from . import strips
        n = len(self.indexes)
        if world == 1:
            comps, _, nonzero = E.compute_strips([owner], self.conf.numPc)
        elif n < 32:   # below the Lanczos path: the strips assembled on every rank, solved by a full engine
            full = PcoaEngine(n, device=owner.device)
            try:
                full.load_gram(gather_strips(owner))
                comps, _, nonzero = full.compute(self.conf.numPc)
            finally:
                full.close()
        else:
            comps, _, nonzero = strips.compute_pca_over_strips([owner], self.conf.numPc, host_exchange=host_exchange)
        print("Non zero rows in matrix: %d / %d." % (nonzero, n))  # :208
        if comps.shape[1] < 2:
            raise IndexError("computePca emits exactly PC1 and PC2 (VariantsPca.scala:229-230); --num-pc must be >= 2")
        reverse = dict((v, k) for (k, v) in self.indexes.items())
        return [(reverse[i], float(comps[i, 0]), float(comps[i, 1])) for i in range(n)]

    # getSimilarityMatrixStream, VariantsPca.scala:262-279 (not called by the reference's main): the same S through
    # upper-triangle pair emission + mirror, i.e. only the keys with a non-zero count exist
    def getSimilarityMatrixStream(self, callsets):
        self.engine = calculate_similarity_matrix(callsets, len(self.indexes), device=self.conf.gpu)
        return similarity_entries_nonzero(self.engine.gram())

    # computePca, VariantsPca.scala:198-231
    def computePca(self, sim_matrix):
        kept = self.kept if self.kept is not None else np.arange(len(self.indexes))   # (--remove-related: the kept samples)
        comps, lam, nonzero = sim_matrix.compute(self.conf.numPc)
        self.last_pca = (comps, lam)   # (--loadings-output-path goes on from them)
        print("Non zero rows in matrix: %d / %d." % (nonzero, kept.size))  # :208
        if comps.shape[1] < 2:
            # the reference indexes array(i + pca.numRows) unconditionally (:230) and fails for --num-pc 1
            raise IndexError("computePca emits exactly PC1 and PC2 (VariantsPca.scala:229-230); --num-pc must be >= 2")
        reverse = dict((v, k) for (k, v) in self.indexes.items())
        return [(reverse[int(i)], float(comps[a, 0]), float(comps[a, 1])) for a, i in enumerate(kept)]

    # --related-min-jaccard X, before the first computePca: the screen of S on the device (pcoa_similar_pairs), the pair file,
    # one stderr line, and with --remove-related the engine replaced by its subset over the kept samples (pcoa_create_subset:
    # one gather of S, no variant fed again); self.kept then names the cohort that computePca and the outlier rounds go on
    # with.  Returns the engine to decompose; sim_matrix is closed when it is replaced (self.engine follows).
    def screenRelated(self, sim_matrix, err=None):
        err = err or sys.stderr
        x, cap = self.conf.related_min_jaccard, self.conf.related_max_pairs
        n = len(self.indexes)
        reverse = dict((v, k) for (k, v) in self.indexes.items())
        name = lambda i: self.names[reverse[int(i)]]
        pairs, n_found, diag = sim_matrix.similar_pairs(x, capacity=cap)
        if n_found > cap:
            raise SystemExit("VariantsPcaDriver: --related-min-jaccard %s reports %d pairs, more than --related-max-pairs %d "
                             "takes; raise --related-max-pairs or the threshold" % (java_double_to_string(x), n_found, cap))
        if self.conf.related_output_path:
            with open(self.conf.related_output_path, "w") as f:
                f.write("name_i\tname_j\tshared\td_i\td_j\tjaccard\n")
                for p in pairs:
                    i, j, shared = int(p["i"]), int(p["j"]), int(p["shared"])
                    union = int(diag[i]) + int(diag[j]) - shared
                    f.write("%s\t%s\t%d\t%d\t%d\t%s\n" % (name(i), name(j), shared, diag[i], diag[j],
                                                          java_double_to_string(float(shared) / float(union))))
        gone = related_removal(pairs, n) if self.conf.remove_related else np.zeros(0, dtype=np.int64)
        err.write("Related pairs: %d at jaccard >= %s; removed %d sample(s)%s\n"
                  % (n_found, java_double_to_string(x), gone.size, (": " + ", ".join(name(i) for i in gone)) if gone.size else ""))
        if gone.size == 0:
            return sim_matrix
        if n - gone.size < min_cohort(self.conf.numPc):
            raise SystemExit("VariantsPcaDriver: --remove-related would leave %d of %d samples, fewer than the %d that %d "
                             "principal components need; raise --related-min-jaccard"
                             % (n - gone.size, n, min_cohort(self.conf.numPc), self.conf.numPc))
        keep = np.setdiff1d(np.arange(n), gone)
        sub = sim_matrix.subset(keep)
        self.gram_seconds_before += sim_matrix.timings()["gram_kernel_seconds"]
        sim_matrix.close()
        self.engine = sub
        self.kept = keep
        return sub

    # --king-cutoff X, before the first computePca: the KING-robust screen over the five planes (pcoa_king_pairs), the pair file,
    # one stderr line, and with --king-remove the rule and the subset of screenRelated.  `king` holds the planes (KingPlanes, or
    # anything with its king_pairs and close); it is closed right after the screen.  Returns the engine to decompose.
    def screenKing(self, sim_matrix, king, err=None):
        err = err or sys.stderr
        x, cap = self.conf.king_cutoff, self.conf.king_max_pairs
        n = len(self.indexes)
        reverse = dict((v, k) for (k, v) in self.indexes.items())
        name = lambda i: self.names[reverse[int(i)]]
        try:
            pairs, n_found, _, _ = king.king_pairs(x, capacity=cap)
        finally:
            king.close()
        if n_found > cap:
            raise SystemExit("VariantsPcaDriver: --king-cutoff %s reports %d pairs, more than --king-max-pairs %d "
                             "takes; raise --king-max-pairs or the cutoff" % (java_double_to_string(x), n_found, cap))
        if self.conf.king_output_path:
            kinship = king_kinship(pairs)
            with open(self.conf.king_output_path, "w") as f:
                f.write("name_i\tname_j\thethet\tibs0\thet_sum\tkinship\n")
                for p, k in zip(pairs, kinship):
                    f.write("%s\t%s\t%d\t%d\t%d\t%s\n" % (name(p["i"]), name(p["j"]), p["hethet"], p["ibs0"], p["het_sum"],
                                                          java_double_to_string(float(k))))
        gone = related_removal(pairs, n) if self.conf.king_remove else np.zeros(0, dtype=np.int64)
        err.write("KING pairs: %d at kinship >= %s; removed %d sample(s)%s\n"
                  % (n_found, java_double_to_string(x), gone.size, (": " + ", ".join(name(i) for i in gone)) if gone.size else ""))
        if gone.size == 0:
            return sim_matrix
        if n - gone.size < min_cohort(self.conf.numPc):
            raise SystemExit("VariantsPcaDriver: --king-remove would leave %d of %d samples, fewer than the %d that %d "
                             "principal components need; raise --king-cutoff"
                             % (n - gone.size, n, min_cohort(self.conf.numPc), self.conf.numPc))
        keep = np.setdiff1d(np.arange(n), gone)
        sub = sim_matrix.subset(keep)
        self.gram_seconds_before += sim_matrix.timings()["gram_kernel_seconds"]
        sim_matrix.close()
        self.engine = sub
        self.kept = keep
        return sub

    # computePca inside --outlier-iterations K: computePca, outlier_rule, and while something is removed and fewer than K
    # rounds have removed something, the engine is replaced by its subset over the kept samples (pcoa_create_subset: one
    # gather of S, no variant fed again) and computePca runs again.  The final cohort always gets a computePca; rows come back
    # for the kept samples only, in the original order.  sim_matrix is closed when it is replaced (self.engine follows).
    def computePcaOutlierRounds(self, sim_matrix, err=None):
        err = err or sys.stderr
        iterations, sigma = self.conf.outlier_iterations, self.conf.outlier_sigma
        if self.conf.numPc < 2:
            raise IndexError("computePca emits exactly PC1 and PC2 (VariantsPca.scala:229-230); --num-pc must be >= 2")
        reverse = dict((v, k) for (k, v) in self.indexes.items())
        kept = self.kept.copy() if self.kept is not None else np.arange(len(self.indexes))   # (--remove-related went first)
        eng, done = sim_matrix, 0
        while True:
            comps, _, nonzero = eng.compute(self.conf.numPc)
            if done == iterations:
                break
            removed = outlier_rule(comps.T, sigma)
            gone = kept[removed]
            err.write("Outlier round %d: removed %d sample(s)%s\n"
                      % (done + 1, gone.size, (": " + ", ".join(self.names[reverse[int(i)]] for i in gone)) if gone.size else ""))
            if gone.size == 0:
                break
            if kept.size - gone.size < min_cohort(self.conf.numPc):
                raise SystemExit("VariantsPcaDriver: --outlier-iterations: round %d would leave %d of %d samples, fewer than the "
                                 "%d that %d principal components need; raise --outlier-sigma"
                                 % (done + 1, kept.size - gone.size, kept.size, min_cohort(self.conf.numPc), self.conf.numPc))
            sub = eng.subset(np.nonzero(~removed)[0])
            self.gram_seconds_before += eng.timings()["gram_kernel_seconds"]
            eng.close()
            eng = self.engine = sub
            kept = kept[~removed]
            done += 1
        print("Non zero rows in matrix: %d / %d." % (nonzero, kept.size))  # :208, once, for the final cohort
        return [(reverse[int(i)], float(comps[a, 0]), float(comps[a, 1])) for a, i in enumerate(kept)]

    # emitResult, VariantsPca.scala:233-246.  stdout: name, dataset, pc1, pc2 sorted by name, as the reference prints.
    # File: the reference hands the rows to Spark's saveAsTextFile, i.e. a DIRECTORY <output-path>-pca.tsv/ of unsorted
    # part-* files (name, pc1, pc2, dataset per line); here the same lines go, sorted by name, into ONE file of that name.
    def emitResult(self, result, out=None, study=None):
        """study (--grm-project-path): (callset id, name, pc1, pc2) of the projected samples: their rows follow the panel's,
        sorted by name among themselves."""
        out = out or sys.stdout
        rows = []
        for (callset_id, pc1, pc2) in result:
            dataset = callset_id.split("-")[0]
            rows.append((self.names[callset_id], pc1, pc2, dataset))
        rows.sort(key=lambda t: t[0])
        if study:
            rows += sorted(((name, pc1, pc2, callset_id.split("-")[0]) for (callset_id, name, pc1, pc2) in study), key=lambda t: t[0])
        for (name, pc1, pc2, dataset) in rows:
            out.write("%s\t%s\t%s\t%s\n" % (name, dataset, java_double_to_string(pc1), java_double_to_string(pc2)))
        if self.conf.outputPath:
            target = self.conf.outputPath + "-pca.tsv"
            if getattr(self.conf, "spark_output_layout", False):   # saveAsTextFile (:241-245): a directory; an existing one is an error
                os.mkdir(target)
                open(os.path.join(target, "_SUCCESS"), "w").close()
                target = os.path.join(target, "part-00000")
            with open(target, "w") as f:
                for (name, pc1, pc2, dataset) in rows:
                    f.write("%s\t%s\t%s\t%s\n" % (name, java_double_to_string(pc1), java_double_to_string(pc2), dataset))

    # --loadings-output-path: w_c = X (J u_c) / sqrt(lambda_c) for every variant the engine was fed, in feed order, from the
    # eigenpairs computePca left.  rows: the variants as calls_as_bits returns them -- streamed past the resident vectors a
    # second time (stored S), or None: the rows are the engine's own store (--gram implicit).
    def emitLoadings(self, rows, meta):
        comps, lam = self.last_pca
        with self.engine.loadings(comps, lam, centre=True, unit=True) as ld:
            if rows is None:
                w = ld.operator()
            elif rows[0] == "bed":
                _, geno, keep, ref_is_a1 = rows
                parts = []
                for v0 in range(0, geno.shape[0], PLINK_BLOCK_ROWS):
                    k = keep[v0:v0 + PLINK_BLOCK_ROWS]
                    if k.any():
                        parts.append(ld.plink_bed(np.ascontiguousarray(geno[v0:v0 + PLINK_BLOCK_ROWS][k]), ref_is_a1=ref_is_a1))
                w = np.concatenate(parts) if parts else np.zeros((0, comps.shape[1]))
            else:
                bits = rows[1]
                parts = [ld.bits(bits[v0:v0 + (1 << 20)]) for v0 in range(0, bits.shape[0], 1 << 20)]
                w = np.concatenate(parts) if parts else np.zeros((0, comps.shape[1]))
        write_loadings(self.conf.loadings_output_path, meta, w)

    def reportIoStats(self, out=None):
        out = out or sys.stdout
        if self.engine is not None:
            t = self.engine.timings()
            out.write("Variants accumulated: %d; Gram kernel %.3f ms; PCoA %.3f ms\n" %
                      (t["gram_variants"], 1e3 * (t["gram_kernel_seconds"] + self.gram_seconds_before),
                       1e3 * t["compute_total_seconds"]))
            info = self.engine.operator_info()
            if info is not None:
                out.write("Implicit similarity operator: %d variants in %.1f MB of carrier bitsets, %d Lanczos steps over "
                          "S v = X^T (X v)\n" % (info[0], info[1] / 1e6, t["lanczos_steps"]))

    def stop(self):
        if self.engine is not None:
            self.engine.close()
            self.engine = None
        if getattr(self, "companion", None) is not None:   # (--missing-calls pairwise: after the engine it was bound to)
            self.companion.close()
            self.companion = None


def write_loadings(path, meta, w):
    """The --loadings-output-path file: one line per variant in feed order -- 0-based index, contig, position, variant id, then
    the loadings as Double.toString prints them, tab-separated.  meta: (contig, position, id) per row; an input that carries
    none (.npz carriers, --synthetic) gets '.' in the three columns."""
    if meta and len(meta) != w.shape[0]:
        raise RuntimeError("--loadings-output-path: %d variant records for %d rows" % (len(meta), w.shape[0]))
    with open(path, "w") as f:
        for v in range(w.shape[0]):
            contig, pos, vid = meta[v] if meta else (".", ".", ".")
            f.write("%d\t%s\t%s\t%s\t%s\n" % (v, contig, pos, vid, "\t".join(java_double_to_string(x) for x in w[v])))


def load_dataset(conf, variant_meta=None):
    """Local stand-in for VariantsCommon (VariantsCommon.scala:33-66): callset index/name maps +
    the variant data.  Returns (indexes, names, [dataset]).  variant_meta: a list that receives (contig, position, id) of
    every row of a carrier-only input (a single VCF or PLINK fileset) as it is read."""
    from . import ingest
    if conf.synthetic:
        return ingest.synthetic_dataset(conf.synthetic)
    if not conf.inputPath:
        raise SystemExit("--input-path (local .vcf[.gz], PLINK .bed/.bim/.fam or .npz) or --synthetic V,N,seed is required: "
                         "the Google Genomics API the reference read from has been shut down")
    paths = conf.inputPath if isinstance(conf.inputPath, (list, tuple)) else [conf.inputPath]
    refs = None if conf.all_references else conf.references
    if len(paths) == 1 and conf.minAlleleFrequency is None:
        if paths[0].endswith(".npz"):
            return ingest.load_npz(paths[0])
        if paths[0][-4:] in (".bed", ".bim", ".fam"):
            return ingest.load_plink(paths[0], refs, ref_allele=conf.plink_ref_allele, as_bed=True, variant_meta=variant_meta)
        return ingest.load_vcf(paths[0], refs, variant_meta=variant_meta)
    # several variant sets (or the AF filter): full variant records are needed for keys and INFO/AF
    if any(p.endswith(".npz") or p[-4:] in (".bed", ".bim", ".fam") for p in paths):
        raise SystemExit("joining variant sets or filtering by allele frequency needs VCF inputs: a .npz dataset or a PLINK "
                         "fileset is read as carriers only (no contig/start/end/ref/alt keys, no INFO/AF)")
    print("Running PCA on %d datasets." % len(paths))  # VariantsCommon.scala:57
    indexes, names, data = {}, {}, []
    used = set()
    for k, path in enumerate(paths):
        set_id = ingest.set_id_of(path, k, used)
        ids, nm, variants = ingest.load_vcf_records(path, parse_refs(refs, k), set_id=set_id)
        # callset index = position in the concatenated callset lists (VariantsCommon.scala:44-45), as the compiled
        # host assigns them; the ids are unique by construction (set_id_of), so nothing is overwritten
        base = len(indexes)
        for i, cid in enumerate(ids):
            if cid in indexes:
                raise ValueError("duplicate callset id %r" % cid)
            indexes[cid] = base + i
        names.update(nm)
        data.append(variants)
    return indexes, names, data


def parse_refs(refs, k):
    """--references holds one list of tuples per variant set, in order (GenomicsConf.scala:47-51)."""
    if not refs:
        return None
    return [refs[k]] if k < len(refs) else [refs[-1]]


def multi_gpu_plan(conf, args, env, device_count, python=None):
    """What `--gpus K` makes of this invocation (dist.launch_plan): ("run", None) = this process is a rank (or K == 1),
    ("spawn", command) = re-execute under torch.distributed.run with K ranks, ("error", message)."""
    from . import dist
    if conf.rank_devices:   # an explicit map: what has to exist is the highest ordinal it names, not K devices
        devs = [int(t) for t in conf.rank_devices.split(",")]
        if len(devs) != conf.gpus:
            return "error", "--rank-devices must name exactly --gpus devices"
        if len(set(devs)) < len(devs) and conf.dist_backend != "gloo":
            return "error", "--rank-devices repeats a device: RCCL needs one GPU per rank (use --dist-backend gloo on a test box)"
        if max(devs) >= device_count or min(devs) < 0:
            return "error", "--rank-devices names GPU %d but only %d GPU(s) are visible" % (max(devs), device_count)
        device_count = max(device_count, conf.gpus)
    return dist.launch_plan(conf.gpus, env, device_count, [os.path.abspath(__file__)] + list(args), python=python or sys.executable)


def gather_strips(owner):
    """The N x N matrix from the [N][cols] strips of every rank, in rank order (all_gather_object: for dumps and tiny N)."""
    import torch.distributed as td
    local = owner.gram()
    if not (td.is_available() and td.is_initialized()) or td.get_world_size() == 1:
        return local
    got = [None] * td.get_world_size()
    td.all_gather_object(got, local)
    return np.concatenate(got, axis=1)


def resolve_layout(conf, n, world, devices):
    """--layout -> None (full) or the column ranges of the strips (pcoa_plan_layout).  auto asks every device for its free
    memory (engines sharing a device split it) and keeps the full layout where it fits, with one rank, or where the devices
    cannot be asked."""
    from . import engine as E
    if conf.layout == "strips" and world > n:
        raise SystemExit("VariantsPcaDriver: --layout strips: %d owners for %d samples; every owner needs a column" % (world, n))
    request = conf.layout
    free = None
    if request == "auto":
        if world == 1 or world > n:
            return None
        try:
            mem = dict((d, E.device_memory(d)[0]) for d in set(devices))
        except E.PcoaError:
            return None
        free = E.engine_free_bytes(devices, lambda d: mem[d])
    layout, ranges = E.plan_layout(n, world, free, request)
    return ranges if layout == "strips" else None


def check_grm_conf(conf):
    """--grm: one GRM engine holds the 2-bit genotypes of one PLINK fileset.  What needs S, carrier bitsets or several engines is
    refused before any file is read or any device is touched, in a message that names --grm and the other flag."""
    if not conf.grm:
        if conf.grm_min_maf is not None:
            raise SystemExit("VariantsPcaDriver: --grm-min-maf needs --grm (the standardised-genotype PCA is off without it)")
        for given, flag in ((conf.grm_geno is not None, "--grm-geno"), (conf.grm_hwe is not None, "--grm-hwe"),
                            (conf.grm_mind is not None, "--grm-mind"),
                            (bool(conf.grm_variant_qc_output_path), "--grm-variant-qc-output-path"),
                            (bool(conf.grm_sample_qc_output_path), "--grm-sample-qc-output-path")):
            if given:
                raise SystemExit("VariantsPcaDriver: %s needs --grm (it is quality control on the genotype store of the "
                                 "standardised-genotype PCA)" % flag)
        if conf.grm_weights_output_path:
            raise SystemExit("VariantsPcaDriver: --grm-weights-output-path needs --grm (the SNP weights are those of the axes of K; "
                             "the loadings of the carrier counts go to --loadings-output-path)")
        if conf.grm_project_path:
            raise SystemExit("VariantsPcaDriver: --grm-project-path needs --grm (it places a second PLINK fileset on the axes of K; "
                             "VCFs are placed on the principal coordinates of S by --project-input-path)")
        if conf.grm_project_lsq:
            raise SystemExit("VariantsPcaDriver: --grm-project-lsq needs --grm (it is the least-squares form of --grm-project-path / "
                             "--grm-project-removed, which place samples on the axes of K)")
        if conf.grm_output_path:
            raise SystemExit("VariantsPcaDriver: --grm-output-path needs --grm (it writes the relationship matrix K of the "
                             "standardised genotypes; the shared counts S go to --dump-similarity)")
        if conf.grm_output_divisor is not None:
            raise SystemExit("VariantsPcaDriver: --grm-output-divisor needs --grm (and --grm-output-path)")
        for given, flag in ((bool(conf.grm_keep_samples), "--grm-keep-samples"), (bool(conf.grm_remove_samples), "--grm-remove-samples"),
                            (conf.grm_outlier_iterations != 0, "--grm-outlier-iterations"),
                            (conf.grm_outlier_sigma is not None, "--grm-outlier-sigma"),
                            (conf.grm_project_removed, "--grm-project-removed")):
            if given:
                raise SystemExit("VariantsPcaDriver: %s needs --grm (it subsets the genotype store of the standardised-genotype PCA; "
                                 "a stored similarity matrix is subset by --outlier-iterations / --remove-related)" % flag)
        for given, flag in ((conf.grm_cutoff is not None, "--grm-cutoff"), (conf.grm_cutoff_divisor is not None, "--grm-cutoff-divisor"),
                            (conf.grm_related_output_path is not None, "--grm-related-output-path"),
                            (conf.grm_cutoff_remove, "--grm-cutoff-remove")):
            if given:
                raise SystemExit("VariantsPcaDriver: %s needs --grm (it screens the relationship matrix K of the standardised "
                                 "genotypes; a stored similarity matrix is screened by --related-min-jaccard / --king-cutoff)" % flag)
        for given, flag in GRM_KING_FLAGS(conf):
            if given:
                raise SystemExit("VariantsPcaDriver: %s needs --grm (it screens the genotype store of the standardised-genotype "
                                 "PCA by KING-robust kinship; a stored similarity matrix is screened by --king-cutoff)" % flag)
        for given, flag in GRM_PCRELATE_FLAGS(conf):
            if given:
                raise SystemExit("VariantsPcaDriver: %s needs --grm (it estimates PC-Relate kinship on the genotype store and the "
                                 "axes of the standardised-genotype PCA)" % flag)
        for given, flag in ((conf.grm_ld_window != 0, "--grm-ld-window"), (conf.grm_ld_r2 is not None, "--grm-ld-r2"),
                            (bool(conf.grm_ld_output_path), "--grm-ld-output-path")):
            if given:
                raise SystemExit("VariantsPcaDriver: %s needs --grm (it prunes the genotype store of the standardised-genotype "
                                 "PCA; the carrier counts S are pruned by --ld-window)" % flag)
        return
    if conf.grm_keep_samples and conf.grm_remove_samples:
        raise SystemExit("VariantsPcaDriver: --grm-keep-samples and --grm-remove-samples exclude each other (one list names the cohort)")
    if conf.grm_outlier_iterations < 0:
        raise SystemExit("VariantsPcaDriver: --grm-outlier-iterations must be >= 0 (0 = off)")
    if conf.grm_outlier_sigma is None:
        conf.grm_outlier_sigma = GRM_OUTLIER_SIGMA
    if not (conf.grm_outlier_sigma > 0 and np.isfinite(conf.grm_outlier_sigma)):
        raise SystemExit("VariantsPcaDriver: --grm-outlier-sigma must be a finite number > 0 (the threshold of --grm-outlier-iterations)")
    if conf.grm_ld_window == 0:
        if conf.grm_ld_r2 is not None:
            raise SystemExit("VariantsPcaDriver: --grm-ld-r2 needs --grm-ld-window W (the pruning is off without it)")
        if conf.grm_ld_output_path:
            raise SystemExit("VariantsPcaDriver: --grm-ld-output-path needs --grm-ld-window W (the pruning is off without it)")
    else:
        if not 1 <= conf.grm_ld_window <= LD_MAX_WINDOW:
            raise SystemExit("VariantsPcaDriver: --grm-ld-window (the LD pruning of --grm) takes a number of variants in [1, %d] (0: off), not '%d'"
                             % (LD_MAX_WINDOW, conf.grm_ld_window))
        if conf.grm_ld_r2 is None:
            conf.grm_ld_r2 = LD_DEFAULT_R2
        if not 0.0 <= conf.grm_ld_r2 <= 1.0:      # (NaN fails both comparisons)
            raise SystemExit("VariantsPcaDriver: --grm-ld-r2 (the threshold of --grm-ld-window) takes a value in [0, 1], not '%s'"
                             % conf.grm_ld_r2)
    if conf.grm_cutoff is None:
        for given, flag in ((conf.grm_cutoff_divisor is not None, "--grm-cutoff-divisor"),
                            (conf.grm_related_output_path is not None, "--grm-related-output-path"),
                            (conf.grm_cutoff_remove, "--grm-cutoff-remove")):
            if given:
                raise SystemExit("VariantsPcaDriver: %s needs --grm-cutoff X (the screen is off without it)" % flag)
    else:
        if not np.isfinite(conf.grm_cutoff):
            raise SystemExit("VariantsPcaDriver: --grm-cutoff must be a finite number (the K at or above which a pair is reported)")
        if conf.grm_cutoff_divisor is not None and conf.grm_cutoff_divisor not in GRM_OUTPUT_DIVISORS:
            raise SystemExit("VariantsPcaDriver: --grm-cutoff-divisor takes used or pairwise, not '%s'" % conf.grm_cutoff_divisor)
    if conf.grm_king_cutoff is None:
        for given, flag in GRM_KING_FLAGS(conf)[1:]:
            if given:
                raise SystemExit("VariantsPcaDriver: %s needs --grm-king-cutoff X (the screen is off without it)" % flag)
    else:
        if not (conf.grm_king_cutoff > 0 and conf.grm_king_cutoff <= 0.5):   # (NaN fails both comparisons)
            raise SystemExit("VariantsPcaDriver: --grm-king-cutoff must be a finite number in (0, 0.5]")
        if conf.grm_king_rows is not None and conf.grm_king_rows not in GRM_KING_ROWS:
            raise SystemExit("VariantsPcaDriver: --grm-king-rows takes all or used, not '%s'" % conf.grm_king_rows)
        if conf.grm_king_max_pairs < 0:
            raise SystemExit("VariantsPcaDriver: --grm-king-max-pairs must be >= 0 (the pairs --grm-king-cutoff may report)")
        if conf.grm_king_remove and conf.grm_cutoff_remove:
            raise SystemExit("VariantsPcaDriver: --grm-king-remove and --grm-cutoff-remove exclude each other (one relatedness "
                             "screen removes samples per run)")
    if conf.grm_pcrelate_output_path is None:
        for given, flag in GRM_PCRELATE_FLAGS(conf)[1:]:
            if given:
                raise SystemExit("VariantsPcaDriver: %s needs --grm-pcrelate-output-path FILE (PC-Relate is off without it)" % flag)
    else:
        most = min(GRM_PCRELATE_MAX_PCS, conf.numPc)
        if conf.grm_pcrelate_pcs is not None and not 1 <= conf.grm_pcrelate_pcs <= most:
            raise SystemExit("VariantsPcaDriver: --grm-pcrelate-pcs must be an integer in [1, %d] (min(8, --num-pc)), not %d"
                             % (most, conf.grm_pcrelate_pcs))
        if conf.grm_pcrelate_cutoff is not None and not np.isfinite(conf.grm_pcrelate_cutoff):
            raise SystemExit("VariantsPcaDriver: --grm-pcrelate-cutoff must be a finite number (the kinship at or above which a pair "
                             "is reported)")
        if conf.grm_pcrelate_maf_threshold is not None and not (0.0 <= conf.grm_pcrelate_maf_threshold < 0.5):   # (NaN fails)
            raise SystemExit("VariantsPcaDriver: --grm-pcrelate-maf-threshold must be a number in [0, 0.5)")
        if conf.grm_pcrelate_max_pairs < 0:
            raise SystemExit("VariantsPcaDriver: --grm-pcrelate-max-pairs must be >= 0 (the pairs --grm-pcrelate-output-path may "
                             "report)")
    if conf.grm_project_lsq:
        if not conf.grm_project_path and not conf.grm_project_removed:
            raise SystemExit("VariantsPcaDriver: --grm-project-lsq needs --grm-project-path or --grm-project-removed (it chooses how "
                             "their samples are placed)")
        if conf.numPc > GRM_LSQ_MAX_PC:
            raise SystemExit("VariantsPcaDriver: --grm-project-lsq takes at most %d principal components, not %d (pcoa_grm_project_lsq "
                             "solves a system of that order per sample)" % (GRM_LSQ_MAX_PC, conf.numPc))
    if conf.grm_output_divisor is not None and conf.grm_output_divisor not in GRM_OUTPUT_DIVISORS:
        raise SystemExit("VariantsPcaDriver: --grm-output-divisor takes used or pairwise, not '%s'" % conf.grm_output_divisor)
    if conf.grm_output_divisor is not None and not conf.grm_output_path:
        raise SystemExit("VariantsPcaDriver: --grm-output-divisor needs --grm-output-path (it chooses the divisor of the matrix "
                         "written there)")
    world = max(conf.gpus, int(os.environ.get("WORLD_SIZE", "1")))
    refused = [
        (world > 1, "runs on one GRM engine: it cannot take --gpus %d" % world),
        (conf.layout == "strips", "holds no similarity matrix to tile: it cannot take --layout strips"),
        (conf.gram == "implicit", "is an operator of its own over 2-bit genotypes: it cannot take --gram implicit"),
        (bool(conf.project_input_path), "places a second PLINK fileset on the axes of K with --grm-project-path: it cannot take "
                                        "--project-input-path"),
        (bool(conf.dump_similarity), "never forms a matrix: it cannot take --dump-similarity"),
        (conf.similarity_measure != "shared", "decomposes K, not a measure over the shared counts: it cannot take "
                                              "--similarity-measure %s" % conf.similarity_measure),
        (conf.missing_calls != "ignore", "mean-imputes missing calls itself: it cannot take --missing-calls %s" % conf.missing_calls),
        (conf.outlier_iterations != 0, "holds no matrix to subset: it cannot take --outlier-iterations"),
        (conf.related_min_jaccard is not None, "holds no shared counts to screen: it cannot take --related-min-jaccard"),
        (conf.king_cutoff is not None, "holds no genotype-class matrices to screen: it cannot take --king-cutoff"),
        (bool(conf.ld_window), "prunes its genotype store by dosage r^2 with --grm-ld-window: it cannot take --ld-window (the "
                               "carrier-indicator pruner in front of an accumulation)"),
        (bool(conf.loadings_output_path), "writes the SNP weights of K with --grm-weights-output-path: it cannot take "
                                          "--loadings-output-path"),
    ]
    for hit, why in refused:
        if hit:
            raise SystemExit("VariantsPcaDriver: --grm " + why)
    if conf.grm_min_maf is not None and not (0.0 <= conf.grm_min_maf < 0.5):
        raise SystemExit("VariantsPcaDriver: --grm-min-maf takes a frequency in [0, 0.5), not '%s'" % conf.grm_min_maf)
    if conf.grm_geno is not None and not (0.0 <= conf.grm_geno <= 1.0):      # (NaN fails both comparisons)
        raise SystemExit("VariantsPcaDriver: --grm-geno takes a share of missing calls in [0, 1], not '%s'" % conf.grm_geno)
    if conf.grm_hwe is not None and not (0.0 <= conf.grm_hwe < 1.0):
        raise SystemExit("VariantsPcaDriver: --grm-hwe takes a p-value in [0, 1), not '%s'" % conf.grm_hwe)
    if conf.grm_mind is not None and not (0.0 <= conf.grm_mind <= 1.0):
        raise SystemExit("VariantsPcaDriver: --grm-mind takes a share of missing calls in [0, 1], not '%s'" % conf.grm_mind)
    paths = conf.inputPath or []
    if conf.synthetic or conf.minAlleleFrequency is not None or len(paths) != 1 or not is_plink_path(paths[0]):
        raise SystemExit("VariantsPcaDriver: --grm reads the genotypes of one PLINK fileset: --input-path must name a single "
                         ".bed / .bim / .fam (dosages from VCF ingest are not built)")
    if conf.grm_project_path:
        check_grm_study(paths[0], conf.grm_project_path)


GRM_OUTPUT_DIVISORS = ("used", "pairwise")
GRM_LSQ_MAX_PC = 16
GRM_OUTPUT_BAND_ROWS = 1024


def grm_dense_rule(codes, ref_is_a1, min_maf=0.0, divisor="used"):
    """The numpy statement of pcoa_grm_block (include/pcoa.h): (K, n) of a cohort given as [V][N] PLINK codes (0 = 00
    homozygous A1, 1 = 01 missing, 2 = 10 heterozygous, 3 = 11 homozygous A2).  With a_vi = c_iv ? g_iv - mu_v : 0.0:
    num(i, j) = sum_v (d_v a_v,lo) a_v,hi (d on the operand of the smaller sample index), n(i, j) = sum_v used_v c_iv c_jv;
    divisor "used": K = num / M', "pairwise": K = n > 0 ? num / n : 0.0.  M' = 0: K is undefined (ValueError)."""
    if divisor not in GRM_OUTPUT_DIVISORS:
        raise ValueError("divisor must be one of used, pairwise, not %r" % (divisor,))
    codes = np.asarray(codes)
    hom = 3 if ref_is_a1 else 0
    c = codes != 1
    g = (codes == 2).astype(np.float64) + 2.0 * (codes == hom).astype(np.float64)
    nv = c.sum(axis=1).astype(np.int64)
    av = (codes == 2).sum(axis=1).astype(np.int64) + 2 * (codes == hom).sum(axis=1).astype(np.int64)
    nf, af = nv.astype(np.float64), av.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = np.where(nv > 0, af / nf, 0.0)
        used = (nv > 0) & (av > 0) & (av < 2 * nv) & (np.minimum(av, 2 * nv - av).astype(np.float64) >= min_maf * (2.0 * nf))
        d = np.where(used, 1.0 / (mu * (1.0 - 0.5 * mu)), 0.0)
    m = int(used.sum())
    if m == 0:
        raise ValueError("none of the %d variants is used: K is undefined" % codes.shape[0])
    a = np.where(c, g - mu[:, None], 0.0)
    upper = (d[:, None] * a).T @ a                 # [i][j] = sum_v (d a_i) a_j: the rule where i <= j
    num = np.triu(upper) + np.triu(upper, 1).T
    cu = (c & used[:, None]).astype(np.int64)
    n = cu.T @ c.astype(np.int64)
    if divisor == "used":
        k = num / float(m)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            k = np.where(n > 0, num / n.astype(np.float64), 0.0)
    return k, n


GRM_PAIR_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("k", np.float64), ("n", np.int64)])   # pcoa_grm_pair (include/pcoa.h)


def grm_pairs_rule(k, cutoff, n=0):
    """The rule of --grm-cutoff and of pcoa_grm_pairs (include/pcoa.h): `k` is the N x N matrix K as grm_dense_rule or
    pcoa_grm_block return it; the pair (i, j), i < j, is reported iff k[i, j] >= cutoff -- one comparison in double on the value
    already divided.  `n`: the N x N pair counts (the PAIRWISE divisor) or one integer (M', the USED divisor) for the records'
    last field.  Returns the reported pairs in increasing (i, j) order as a structured array GRM_PAIR_DTYPE."""
    k = np.asarray(k, dtype=np.float64)
    if k.ndim != 2 or k.shape[0] != k.shape[1]:
        raise ValueError("k must be N x N")
    hit = (k >= np.float64(cutoff)) & np.triu(np.ones(k.shape, dtype=bool), 1)
    i, j = np.nonzero(hit)                      # row-major: increasing (i, j)
    out = np.zeros(i.size, dtype=GRM_PAIR_DTYPE)
    out["i"], out["j"], out["k"] = i, j, k[i, j]
    out["n"] = np.asarray(n)[i, j] if np.ndim(n) == 2 else int(n)
    return out


PCRELATE_MAX_COV = 9


def pcrelate_hat_rule(basis):
    """The numpy statement of pcoa_pcrelate_hat (include/pcoa.h), bit for bit: hat = (basis basis^T)^-1 basis for `basis`
    [n_cov][N], 1 <= n_cov <= 9.  G[c][c'] = sum_i basis[c][i] * basis[c'][i] with i ascending (np.cumsum adds in sequence), the
    square-root-free L D L^T of pcoa_grm_project_lsq in its sequence, then the forward / diagonal / backward solve of every sample
    column (vectorised over the samples: every product and difference is one rounded ufunc).  ValueError where the library
    answers PCOA_ERR_INVALID_ARG."""
    b = np.ascontiguousarray(basis, dtype=np.float64)
    if b.ndim != 2:
        raise ValueError("basis must be [n_cov][N]")
    k, n = b.shape
    if not 1 <= k <= PCRELATE_MAX_COV:
        raise ValueError("n_cov = %d is outside [1, %d]" % (k, PCRELATE_MAX_COV))
    if n < k:
        raise ValueError("n = %d samples cannot determine n_cov = %d covariates" % (n, k))
    if not np.isfinite(b).all():
        raise ValueError("basis holds a value that is not a finite number")
    h = [[0.0] * (c + 1) for c in range(k)]
    for c in range(k):
        for j in range(c + 1):
            h[c][j] = float(np.cumsum(b[c] * b[j])[-1])
    for c in range(k):
        hcc = h[c][c]
        for j in range(c):
            s = h[c][j]
            for q in range(j):
                s = s - h[c][q] * h[j][q]
            h[c][j] = s
        s = hcc
        for q in range(c):
            w = h[c][q]
            l = w / h[q][q]
            s = s - w * l
            h[c][q] = l
        if not hcc > 0.0 or not np.isfinite(s) or s <= 2.0 ** -40 * hcc:
            raise ValueError("covariate %d is collinear with the covariates before it" % c)
        h[c][c] = s
    y = np.zeros_like(b)
    for c in range(k):
        s = b[c].copy()
        for q in range(c):
            s = s - h[c][q] * y[q]
        y[c] = s
    for c in range(k):
        y[c] = y[c] / h[c][c]
    x = np.zeros_like(b)
    for c in range(k - 1, -1, -1):
        s = y[c].copy()
        for q in range(c + 1, k):
            s = s - h[q][c] * x[q]
        x[c] = s
    return x


def grm_pcrelate_isaf_rule(beta, basis):
    """mu_iv [V][N] of pcoa_grm_pcrelate_isaf from beta [V][n_cov] and basis [n_cov][N]: e = beta_v0 * basis[0][i], then
    e = e + beta_vc * basis[c][i] for c = 1 .. n_cov - 1, every product and sum rounded on its own; mu = 0.5 * e."""
    beta = np.asarray(beta, dtype=np.float64)
    basis = np.asarray(basis, dtype=np.float64)
    if beta.ndim != 2 or basis.ndim != 2 or beta.shape[1] != basis.shape[0]:
        raise ValueError("beta must be [V][n_cov] and basis [n_cov][N]")
    e = beta[:, 0:1] * basis[0][None, :]
    for c in range(1, basis.shape[0]):
        e = e + beta[:, c:c + 1] * basis[c][None, :]
    return 0.5 * e


def grm_pcrelate_beta_rule(codes, ref_is_a1, hat):
    """beta [V][n_cov] of pcoa_grm_pcrelate_fit up to the order of its additions: sum_i hat[c][i] * (c_iv ? g_iv : mu_v), for
    every row of the store."""
    codes = np.asarray(codes)
    hom = 3 if ref_is_a1 else 0
    c = codes != 1
    g = (codes == 2).astype(np.float64) + 2.0 * (codes == hom).astype(np.float64)
    nv = c.sum(axis=1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = np.where(nv > 0, g.sum(axis=1) / nv, 0.0)
    return np.where(c, g, mu[:, None]) @ np.asarray(hat, dtype=np.float64).T


def grm_pcrelate_rule(codes, ref_is_a1, beta, basis, t, min_maf=0.0, keep=None):
    """The numpy statement of pcoa_grm_pcrelate_block (include/pcoa.h): (phi, n, num, den) of a cohort given as [V][N] PLINK
    codes, the fit beta [V][n_cov], the covariates basis [n_cov][N] and the threshold t in [0, 0.5).  used_v is
    grm_dense_rule's under min_maf, and `keep` ([V] bool, an LD mask) where given.  m = used and called and t < mu < 1 - t;
    a = m ? g - e : 0; b = m ? sqrt(mu (1 - mu)) : 0; num = a^T a, den = b^T b, n = m^T m; phi = den > 0 ? num / (4 den) : 0."""
    if not (np.isfinite(t) and 0.0 <= t < 0.5):
        raise ValueError("t = %r is outside [0, 0.5)" % (t,))
    codes = np.asarray(codes)
    hom = 3 if ref_is_a1 else 0
    c = codes != 1
    g = (codes == 2).astype(np.float64) + 2.0 * (codes == hom).astype(np.float64)
    nv = c.sum(axis=1).astype(np.int64)
    av = (codes == 2).sum(axis=1).astype(np.int64) + 2 * (codes == hom).sum(axis=1).astype(np.int64)
    used = (nv > 0) & (av > 0) & (av < 2 * nv) & (np.minimum(av, 2 * nv - av).astype(np.float64) >= min_maf * (2.0 * nv.astype(np.float64)))
    if keep is not None:
        used = used & np.asarray(keep, dtype=bool)
    if not used.any():
        raise ValueError("none of the %d variants is used: phi is undefined" % codes.shape[0])
    beta, basis = np.asarray(beta, dtype=np.float64), np.asarray(basis, dtype=np.float64)
    if beta.ndim != 2 or basis.ndim != 2 or beta.shape[1] != basis.shape[0]:
        raise ValueError("beta must be [V][n_cov] and basis [n_cov][N]")
    e = beta[:, 0:1] * basis[0][None, :]           # the contract's sequence, as grm_pcrelate_isaf_rule forms it
    for q in range(1, basis.shape[0]):
        e = e + beta[:, q:q + 1] * basis[q][None, :]
    mu = 0.5 * e
    m = used[:, None] & c & (mu > t) & (mu < 1.0 - t)
    a = np.where(m, g - e, 0.0)
    with np.errstate(invalid="ignore"):
        b = np.where(m, np.sqrt(np.where(m, mu * (1.0 - mu), 0.0)), 0.0)
    num, den = a.T @ a, b.T @ b
    mi = m.astype(np.int64)
    n = mi.T @ mi
    with np.errstate(divide="ignore", invalid="ignore"):
        phi = np.where(den > 0, num / (4.0 * den), 0.0)
    return phi, n, num, den


def write_grm_files(prefix, ids, bands):
    """PREFIX.grm.bin / PREFIX.grm.N.bin / PREFIX.grm.id, the layout GCTA and PLINK read.  ids: (set id, sample name) per row;
    bands: an iterable of (row0, K rows [r][>= row0 + r] float64, n rows of the same shape), consecutive from row 0: of row i
    the entries (i, 0) .. (i, i) are written, as float32.  Returns the bytes written to the two .bin files."""
    total = 0
    with open(prefix + ".grm.bin", "wb") as fk, open(prefix + ".grm.N.bin", "wb") as fn:
        for row0, kb, nb in bands:
            for r in range(kb.shape[0]):
                i = row0 + r
                fk.write(np.asarray(kb[r, :i + 1], dtype=np.float64).astype("<f4").tobytes())
                fn.write(np.asarray(nb[r, :i + 1]).astype("<f4").tobytes())
                total += 8 * (i + 1)
    with open(prefix + ".grm.id", "w") as f:
        for set_id, name in ids:
            f.write("%s\t%s\n" % (set_id, name))
    return total


def grm_write_output(conf, eng, ids, err=None):
    """--grm-output-path: K band by band (GRM_OUTPUT_BAND_ROWS rows, columns 0 .. band end) out of the engine through
    pcoa_grm_block with host pointers -- no N x N array exists on either side -- and the stderr line."""
    divisor = conf.grm_output_divisor or "used"
    n = eng.n

    def bands():
        for r0 in range(0, n, GRM_OUTPUT_BAND_ROWS):
            r = min(GRM_OUTPUT_BAND_ROWS, n - r0)
            kb, nb = eng.grm_block(r0, r, 0, r0 + r, divisor, pairs=True)
            yield r0, kb, nb

    nbytes = write_grm_files(conf.grm_output_path, ids, bands())
    (err or sys.stderr).write("GRM written: %d samples, %d used variants, divisor %s, %d bytes\n"
                              % (n, eng.grm_info()[1], divisor, nbytes))


def plink_prefix(path):
    return path[:-4] if path[-4:] in (".bed", ".bim", ".fam") else path


def check_grm_study(panel_path, study_path):
    """--grm-project-path, before any engine exists: the study is a PLINK fileset whose .bim equals the panel's line by line in
    contig, id, position and both alleles (a fileset with the alleles exchanged is refused, not flipped), and none of its sample
    names repeats a panel name."""
    if not is_plink_path(study_path):
        raise SystemExit("VariantsPcaDriver: --grm --grm-project-path must name a PLINK .bed / .bim / .fam, not %s" % study_path)
    panel, study = plink_prefix(panel_path), plink_prefix(study_path)

    def bim_lines(prefix):
        with open(prefix + ".bim") as f:
            return [ln.split() for ln in f if ln.strip()]

    a, b = bim_lines(panel), bim_lines(study)
    for k in range(max(len(a), len(b))):
        if k >= len(a) or k >= len(b):
            raise SystemExit("VariantsPcaDriver: --grm --grm-project-path: %s.bim and %s.bim differ at line %d: %s.bim ends after "
                             "%d lines (both filesets must hold the same variants in the same order)"
                             % (study, panel, k + 1, study if k >= len(b) else panel, min(len(a), len(b))))
        x, y = a[k], b[k]
        key_x, key_y = (x[0], x[1], x[3], x[4], x[5]), (y[0], y[1], y[3], y[4], y[5])
        if key_x != key_y:
            swapped = key_x[:3] == key_y[:3] and (x[4], x[5]) == (y[5], y[4])
            raise SystemExit("VariantsPcaDriver: --grm --grm-project-path: %s.bim and %s.bim differ at line %d: study '%s', panel "
                             "'%s'%s (contig, id, position and both alleles must agree)"
                             % (study, panel, k + 1, " ".join(key_y), " ".join(key_x),
                                ": the alleles are exchanged, and genotypes are not flipped" if swapped else ""))

    def fam_names(prefix):
        with open(prefix + ".fam") as f:
            return [ln.split()[1] for ln in f if ln.strip()]

    seen = set(fam_names(panel))
    for name in fam_names(study):
        if name in seen:
            raise SystemExit("VariantsPcaDriver: --grm --grm-project-path: the study sample '%s' of %s.fam repeats a sample name of "
                             "the panel" % (name, study))


def grm_place(conf, panel_eng, study, comps, lam, what, labels, err=None):
    """The samples of `study` on the panel's axes -- mean-imputed (pcoa_grm_project), or with --grm-project-lsq by least squares
    (pcoa_grm_project_lsq) -- and the stderr line(s).  labels[q]: the name a message gives sample q.  Returns (coords [Nq][k],
    placed [Nq] bool): an undetermined sample of the least-squares form is named on stderr and not placed."""
    err = err or sys.stderr
    used = panel_eng.grm_info()[1]
    if not conf.grm_project_lsq:
        coords, called = panel_eng.grm_project(study, comps, lam)
        err.write("Projected %d %ssamples over %d used variants (mean call share %.4f)\n"
                  % (study.n, what, used, float(called.mean()) / used))
        return coords, np.ones(study.n, dtype=bool)
    coords, called, determined = panel_eng.grm_project_lsq(study, comps)
    err.write("Projected %d %ssamples over %d used variants (mean call share %.4f, least squares, %d undetermined)\n"
              % (study.n, what, used, float(called.mean()) / used, int((~determined).sum())))
    for q in np.nonzero(~determined)[0]:
        err.write("Not placed: %s is called at %d of %d used variants, which do not determine %d coordinates\n"
                  % (labels[int(q)], int(called[q]), used, comps.shape[1]))
    return coords, determined


def grm_project_study(conf, panel_eng, comps, lam, err=None):
    """--grm-project-path: the study's .bed rows into a GRM study store (the panel's keep mask applies: the .bim files are
    equal), its samples placed on the panel's axes, and the stderr line.  Returns ([(callset id, name, pc1, pc2)], in the
    study's .fam order)."""
    from . import ingest
    refs = None if conf.all_references else conf.references
    indexes, names, data = ingest.load_plink(conf.grm_project_path, refs, ref_allele=conf.plink_ref_allele, as_bed=True)
    _, geno, keep, ref_is_a1 = data[0]
    nq = len(indexes)
    with PcoaEngine(nq, device=conf.gpu, grm_study=True) as study:
        for v0 in range(0, geno.shape[0], PLINK_BLOCK_ROWS):
            k = keep[v0:v0 + PLINK_BLOCK_ROWS]
            if k.any():
                study.accumulate_plink_bed(np.ascontiguousarray(geno[v0:v0 + PLINK_BLOCK_ROWS][k]), ref_is_a1=ref_is_a1)
        study.finalize()
        reverse = dict((v, k) for (k, v) in indexes.items())
        coords, placed = grm_place(conf, panel_eng, study, comps, lam, "", [names[reverse[q]] for q in range(nq)], err)
    # the set id as the compiled host assigns it: the second set of the run ('_1' behind a stem the panel has taken)
    set_id = ingest.set_id_of(conf.grm_project_path, 1, set([ingest.set_id_of(conf.inputPath[0])]))
    return [("%s-%d" % (set_id, q), names[reverse[q]], float(coords[q, 0]), float(coords[q, 1])) for q in range(nq) if placed[q]]


def grm_accumulate(call_rdd, matrix_size, min_maf, device=0, err=None, max_missing=1.0, hwe_min_p=0.0):
    """--grm: the raw .bed rows of a PLINK fileset into one GRM engine, block by block (pcoa_accumulate_plink_bed), and the
    stderr line that says what the engine will decompose.  --grm-geno / --grm-hwe are set straight after the create, so that
    every later step -- and every subset, which inherits them -- honours them."""
    _, geno, keep, ref_is_a1 = call_rdd
    eng = PcoaEngine(matrix_size, device=device, grm=True)
    eng.grm_set_min_maf(min_maf)
    eng.grm_set_variant_filters(max_missing, hwe_min_p)
    all_kept = bool(keep.all())
    for v0 in range(0, geno.shape[0], PLINK_BLOCK_ROWS):
        rows = geno[v0:v0 + PLINK_BLOCK_ROWS]
        if not all_kept:
            k = keep[v0:v0 + PLINK_BLOCK_ROWS]
            if not k.any():
                continue
            rows = rows[k]
        eng.accumulate_plink_bed(np.ascontiguousarray(rows), ref_is_a1=ref_is_a1)
    eng.finalize()
    variants, used, store = eng.grm_info()
    (err or sys.stderr).write("Standardised genotypes: %d of %d variants used (min MAF %g), store %d bytes\n"
                              % (used, variants, min_maf, store))
    return eng


def grm_qc_used_rule(counts, p, n_samples, min_maf, max_missing, hwe_min_p):
    """used_v of include/pcoa.h from the counts and p-values an engine returned, without an LD mask: the column of
    --grm-variant-qc-output-path (both hosts evaluate the same fp64 expressions)."""
    n = counts[:, 0].astype(np.int64)
    a = counts[:, 1].astype(np.int64) + 2 * counts[:, 2].astype(np.int64)
    used = (n > 0) & (a > 0) & (a < 2 * n) & (np.minimum(a, 2 * n - a).astype(np.float64) >= min_maf * (2.0 * n.astype(np.float64)))
    used &= (n_samples - n).astype(np.float64) <= max_missing * float(n_samples)
    if hwe_min_p != 0.0:
        used &= p >= hwe_min_p
    return used


def grm_qc(conf, eng, names, meta, err=None):
    """--grm-mind and the two QC files, on the engine of the whole fileset straight after the feed: the variant file (counts,
    missing share, HWE p and used_v of the fed cohort), the sample file (before anyone is removed), the stderr line.  Returns
    the indices of the samples --grm-mind keeps (increasing), or None without it."""
    n, (total, _, _) = eng.n, eng.grm_info()
    min_maf = conf.grm_min_maf or 0.0
    geno = 1.0 if conf.grm_geno is None else conf.grm_geno
    hwe = 0.0 if conf.grm_hwe is None else conf.grm_hwe
    if conf.grm_variant_qc_output_path:
        counts, p = eng.grm_counts(), eng.grm_hwe()
        used = grm_qc_used_rule(counts, p, n, min_maf, geno, hwe)
        labelled = bool(meta) and len(meta) == total
        with open(conf.grm_variant_qc_output_path, "w") as f:
            for v in range(total):
                contig, pos, vid = meta[v] if labelled else (".", ".", ".")
                f.write("%d\t%s\t%s\t%s\t%d\t%d\t%d\t%.6f\t%.17g\t%d\n"
                        % (v, contig, pos, vid, counts[v, 0], counts[v, 1], counts[v, 2], float(n - counts[v, 0]) / float(n), p[v],
                           1 if used[v] else 0))
    kept, gone = None, 0
    if conf.grm_mind is not None or conf.grm_sample_qc_output_path:
        sc = eng.grm_sample_counts()
        stay = np.ones(n, dtype=bool)
        if conf.grm_mind is not None and total > 0:
            stay = ~((total - sc[:, 0]).astype(np.float64) / float(total) > conf.grm_mind)
        if conf.grm_sample_qc_output_path:
            with open(conf.grm_sample_qc_output_path, "w") as f:
                for i in range(n):
                    called = int(sc[i, 0])
                    f.write("%s\t%d\t%d\t%d\t%.6f\t%.6f\t%d\n"
                            % (names[i], called, sc[i, 1], sc[i, 2], float(called) / float(total) if total else 0.0,
                               float(sc[i, 1]) / float(called) if called else 0.0, 1 if stay[i] else 0))
        if conf.grm_mind is not None:
            kept, gone = np.nonzero(stay)[0], int((~stay).sum())
    st = eng.grm_qc_stats()
    (err or sys.stderr).write("GRM QC: removed %d variant(s) by MAF, %d by missing rate, %d by HWE; %d sample(s) by call rate\n"
                              % (st["grm_qc_fail_maf"], st["grm_qc_fail_missing"], st["grm_qc_fail_hwe"], gone))
    return kept


def grm_sample_list(conf, names):
    """--grm-keep-samples / --grm-remove-samples, before any engine exists: `names` are the fileset's sample names in index
    order.  Returns the kept indices (increasing), or None without a list.  An unknown or repeated name is refused."""
    flag, path = ("--grm-keep-samples", conf.grm_keep_samples) if conf.grm_keep_samples else ("--grm-remove-samples", conf.grm_remove_samples)
    if not path:
        return None
    index = dict((name, i) for i, name in enumerate(names))
    try:
        with open(path) as f:
            listed = [ln.strip() for ln in f if ln.strip()]
    except IOError as e:
        raise SystemExit("VariantsPcaDriver: %s: cannot read %s (%s)" % (flag, path, e.strerror))
    seen = set()
    for name in listed:
        if name not in index:
            raise SystemExit("VariantsPcaDriver: --grm %s: '%s' of %s is not a sample of the fileset" % (flag, name, path))
        if name in seen:
            raise SystemExit("VariantsPcaDriver: --grm %s: '%s' is listed twice in %s" % (flag, name, path))
        seen.add(name)
    picked = np.array(sorted(index[name] for name in listed), dtype=np.int64)
    kept = picked if conf.grm_keep_samples else np.setdiff1d(np.arange(len(names)), picked)
    least = max(GRM_MIN_COHORT, conf.numPc + 1)
    if kept.size < least:
        raise SystemExit("VariantsPcaDriver: --grm %s leaves %d of %d samples, fewer than the %d a GRM engine with %d principal "
                         "components needs" % (flag, kept.size, len(names), least, conf.numPc))
    return kept


def grm_subset_engine(src, keep, min_maf, study=False, err=None):
    """pcoa_create_grm_subset of `src` over its samples `keep`, and the stderr lines: what was gathered, and (a panel) what the
    reduced cohort's engine will decompose."""
    err = err or sys.stderr
    before = src.grm_subset_stats()["grm_subset_bytes"]
    sub = src.grm_subset(keep, study=study)
    err.write("GRM subset: kept %d of %d samples, %d bytes gathered\n"
              % (len(keep), src.n, src.grm_subset_stats()["grm_subset_bytes"] - before))
    if not study:
        variants, used, store = sub.grm_info()
        err.write("Standardised genotypes: %d of %d variants used (min MAF %g), store %d bytes\n" % (used, variants, min_maf, store))
    return sub


GRM_CUTOFF_CAPACITY = 1 << 20


def write_grm_related(path, pairs, names):
    """--grm-related-output-path: one line per reported pair, in the order given: name_i, name_j, K, n (`names`: the names of
    the screened engine's samples in index order).  K is written as Java's Double.toString does, like the kinship of
    --king-output-path."""
    with open(path, "w") as f:
        f.write("name_i\tname_j\tk\tn\n")
        for p in pairs:
            f.write("%s\t%s\t%s\t%d\n" % (names[int(p["i"])], names[int(p["j"])], java_double_to_string(float(p["k"])), int(p["n"])))


def grm_screen_related(conf, eng, names, err=None):
    """--grm-cutoff X on the engine that is about to be decomposed (pcoa_grm_pairs): the pair file, the stderr line and, with
    --grm-cutoff-remove, the samples related_removal takes out (indices of `eng`, sorted; empty otherwise)."""
    divisor = conf.grm_cutoff_divisor or "used"
    pairs, n_found = eng.grm_pairs(conf.grm_cutoff, divisor, capacity=GRM_CUTOFF_CAPACITY)
    if n_found > pairs.size:   # more than the first call's room: the count is known now
        pairs, n_found = eng.grm_pairs(conf.grm_cutoff, divisor, capacity=n_found)
    if conf.grm_related_output_path:
        write_grm_related(conf.grm_related_output_path, pairs, names)
    gone = related_removal(pairs, eng.n) if conf.grm_cutoff_remove else np.zeros(0, dtype=np.int64)
    (err or sys.stderr).write("GRM relatedness: %d pair(s) with K >= %s (divisor %s), removed %d sample(s)\n"
                              % (n_found, java_double_to_string(conf.grm_cutoff), divisor, gone.size))
    return gone


GRM_KING_ROWS = ("all", "used")   # --grm-king-rows: PCOA_GRM_ROWS_ALL / PCOA_GRM_ROWS_USED


def GRM_KING_FLAGS(conf):
    """(given, flag) of --grm-king-cutoff and its dependants, the cutoff first."""
    return [(conf.grm_king_cutoff is not None, "--grm-king-cutoff"), (conf.grm_king_rows is not None, "--grm-king-rows"),
            (conf.grm_king_output_path is not None, "--grm-king-output-path"),
            (conf.grm_king_max_pairs_given, "--grm-king-max-pairs"), (conf.grm_king_remove, "--grm-king-remove")]


def write_king_pairs(path, pairs, names):
    """The pair file of --king-output-path and --grm-king-output-path: one header line, then name_i, name_j, hethet, ibs0,
    het_sum, kinship per pair, tab-separated, the kinship as Java's Double.toString writes it."""
    kinship = king_kinship(pairs)
    with open(path, "w") as f:
        f.write("name_i\tname_j\thethet\tibs0\thet_sum\tkinship\n")
        for p, k in zip(pairs, kinship):
            f.write("%s\t%s\t%d\t%d\t%d\t%s\n" % (names[int(p["i"])], names[int(p["j"])], p["hethet"], p["ibs0"], p["het_sum"],
                                                  java_double_to_string(float(k))))


def grm_screen_king(conf, eng, names, err=None):
    """--grm-king-cutoff X on the engine that is about to be decomposed (pcoa_grm_king_pairs): the pair file, the stderr line
    and, with --grm-king-remove, the samples related_removal takes out (indices of `eng`, sorted; empty otherwise)."""
    x, cap, rows = conf.grm_king_cutoff, conf.grm_king_max_pairs, conf.grm_king_rows or "used"
    pairs, n_found, n_rows = eng.grm_king_pairs(x, rows=rows, capacity=cap)
    if n_found > cap:
        raise SystemExit("VariantsPcaDriver: --grm-king-cutoff %s reports %d pairs, more than --grm-king-max-pairs %d "
                         "takes; raise --grm-king-max-pairs or the cutoff" % (java_double_to_string(x), n_found, cap))
    if conf.grm_king_output_path:
        write_king_pairs(conf.grm_king_output_path, pairs, names)
    gone = related_removal(pairs, eng.n) if conf.grm_king_remove else np.zeros(0, dtype=np.int64)
    (err or sys.stderr).write("GRM KING: %d pair(s) with kinship >= %s over %d row(s) (rows %s), removed %d sample(s)\n"
                              % (n_found, java_double_to_string(x), n_rows, rows, gone.size))
    return gone


GRM_PCRELATE_MAX_PCS = 8
GRM_PCRELATE_CUTOFF = 0.044194173824159216   # 2^-4.5, between third and fourth degree (the literal both hosts share)
GRM_PCRELATE_MAF_THRESHOLD = 0.01
GRM_PCRELATE_BLOCK = 1024                  # the diagonal blocks n(i, i) is read in


def GRM_PCRELATE_FLAGS(conf):
    """(given, flag) of --grm-pcrelate-output-path and its dependants, the output path first."""
    return [(conf.grm_pcrelate_output_path is not None, "--grm-pcrelate-output-path"),
            (conf.grm_pcrelate_pcs is not None, "--grm-pcrelate-pcs"), (conf.grm_pcrelate_cutoff is not None, "--grm-pcrelate-cutoff"),
            (conf.grm_pcrelate_maf_threshold is not None, "--grm-pcrelate-maf-threshold"),
            (conf.grm_pcrelate_inbreeding_output_path is not None, "--grm-pcrelate-inbreeding-output-path"),
            (conf.grm_pcrelate_max_pairs_given, "--grm-pcrelate-max-pairs")]


def write_pcrelate_pairs(path, pairs, names):
    """--grm-pcrelate-output-path: one header line, then name_i, name_j, kinship, n per reported pair in (i, j) order,
    tab-separated, the kinship as Java's Double.toString writes it."""
    with open(path, "w") as f:
        f.write("name_i\tname_j\tkinship\tn\n")
        for p in pairs:
            f.write("%s\t%s\t%s\t%d\n" % (names[int(p["i"])], names[int(p["j"])], java_double_to_string(float(p["k"])), int(p["n"])))


def write_pcrelate_inbreeding(path, names, phi_diag, n_diag):
    """--grm-pcrelate-inbreeding-output-path: one header line, then name, f = 2 phi(i, i) - 1 (one product, one difference, as
    Java's Double.toString writes it) and n(i, i) per sample in cohort order."""
    with open(path, "w") as f:
        f.write("name\tf\tn\n")
        for name, phi, n in zip(names, phi_diag, n_diag):
            f.write("%s\t%s\t%d\n" % (name, java_double_to_string(2.0 * float(phi) - 1.0), int(n)))


def grm_pcrelate(driver, full, eng, kept, meta, err=None):
    """--grm-pcrelate-output-path, behind the last computePca and --grm-project-removed.  The cohort is the final cohort (`kept`,
    engine `eng`) plus the removed samples --grm-project-removed placed (driver.last_placed), in fileset index order; its engine
    is `eng` itself, or a panel subset of the whole-fileset engine `full` over the cohort, pruned under --grm-ld-window like every
    round's engine.  The covariates are a row of ones and the first K coordinates of every cohort sample -- u_c for the final
    cohort, the projected coordinate for a placed one -- and the hat matrix is pcoa_pcrelate_hat's.  n(i, i) of the inbreeding
    file is read with pcoa_grm_pcrelate_block's pair counts over diagonal blocks."""
    from .engine import pcrelate_hat
    conf, err = driver.conf, err or sys.stderr
    k = conf.grm_pcrelate_pcs if conf.grm_pcrelate_pcs is not None else min(2, conf.numPc)
    x = GRM_PCRELATE_CUTOFF if conf.grm_pcrelate_cutoff is None else conf.grm_pcrelate_cutoff
    t = GRM_PCRELATE_MAF_THRESHOLD if conf.grm_pcrelate_maf_threshold is None else conf.grm_pcrelate_maf_threshold
    cap = conf.grm_pcrelate_max_pairs
    comps, _ = driver.last_pca
    reverse = dict((v, c) for (c, v) in driver.indexes.items())
    placed_idx, placed_coords = getattr(driver, "last_placed", None) or (np.zeros(0, dtype=np.int64), np.zeros((0, comps.shape[1])))
    kept = np.asarray(kept, dtype=np.int64)
    cohort = np.concatenate([kept, np.asarray(placed_idx, dtype=np.int64)])
    coords = np.concatenate([np.asarray(comps)[:, :k], np.asarray(placed_coords)[:, :k]], axis=0)
    order = np.argsort(cohort, kind="stable")
    cohort, coords = cohort[order], coords[order]
    sub = None
    if len(placed_idx):
        least = max(GRM_MIN_COHORT, conf.numPc + 1)
        if cohort.size < least:
            raise SystemExit("VariantsPcaDriver: --grm-pcrelate-output-path: the cohort holds %d samples, fewer than the %d a GRM "
                             "engine with %d principal components needs" % (cohort.size, least, conf.numPc))
        sub = grm_subset_engine(full, cohort, conf.grm_min_maf or 0.0, err=err)
        if conf.grm_ld_window:
            grm_ld_prune(conf, sub, meta)
        eng = sub
    try:
        names = [driver.names[reverse[int(i)]] for i in cohort]
        basis = np.ascontiguousarray(np.vstack([np.ones((1, cohort.size)), coords.T]))
        eng.grm_pcrelate_fit(basis, pcrelate_hat(basis))
        pairs, n_found, diag = eng.grm_pcrelate_pairs(x, t, capacity=cap, diag=True)
        if n_found > cap:
            raise SystemExit("VariantsPcaDriver: --grm-pcrelate-cutoff %s reports %d pairs, more than --grm-pcrelate-max-pairs %d "
                             "takes; raise --grm-pcrelate-max-pairs or the cutoff" % (java_double_to_string(x), n_found, cap))
        write_pcrelate_pairs(conf.grm_pcrelate_output_path, pairs, names)
        if conf.grm_pcrelate_inbreeding_output_path:
            n_diag = np.zeros(cohort.size, dtype=np.int64)
            for r0 in range(0, cohort.size, GRM_PCRELATE_BLOCK):
                r = min(GRM_PCRELATE_BLOCK, cohort.size - r0)
                n_diag[r0:r0 + r] = np.diagonal(eng.grm_pcrelate_block(r0, r, r0, r, t, pairs=True)[1])
            write_pcrelate_inbreeding(conf.grm_pcrelate_inbreeding_output_path, names, diag, n_diag)
        err.write("GRM PC-Relate: %d pair(s) with kinship >= %s among %d sample(s), %d %s, %d used variant(s), threshold %s\n"
                  % (n_found, java_double_to_string(x), cohort.size, k, "axis" if k == 1 else "axes", eng.grm_info()[1],
                     java_double_to_string(t)))
    finally:
        if sub is not None:
            sub.close()


def grm_compute_rounds(driver, full, kept, meta, err=None):
    """computePca of --grm around --grm-keep-samples / --grm-remove-samples (`kept`: the list's indices, or None) and
    --grm-outlier-iterations K: the loop of computePcaOutlierRounds with the engine replaced by its grm_subset over the kept
    samples; --grm-ld-window prunes every round's engine, because the candidates follow the cohort's frequencies.  `full`, the
    engine of the whole fileset, is closed as soon as it is replaced unless --grm-project-removed needs it.  Returns (rows of
    the kept samples, the final engine, their original indices); driver.engine and driver.last_pca follow."""
    conf, err = driver.conf, err or sys.stderr
    if conf.numPc < 2:
        raise IndexError("computePca emits exactly PC1 and PC2 (VariantsPca.scala:229-230); --num-pc must be >= 2")
    min_maf = conf.grm_min_maf or 0.0
    reverse = dict((v, k) for (k, v) in driver.indexes.items())
    eng = full

    def replace(sub):
        if eng is not full or not conf.grm_project_removed:
            eng.close()
        driver.engine = sub
        return sub

    if kept is None:
        kept = np.arange(len(driver.indexes))
    else:
        eng = replace(grm_subset_engine(eng, kept, min_maf, err=err))
    pruned = False   # eng carries the prune of --grm-ld-window already
    if conf.grm_cutoff is not None:
        # --grm-cutoff: the screen sees the K that would be decomposed: behind the list's subset and one prune of that engine
        if conf.grm_ld_window:
            grm_ld_prune(conf, eng, meta)
            pruned = True
        gone = grm_screen_related(conf, eng, [driver.names[reverse[int(i)]] for i in kept], err=err)
        if gone.size:
            least = max(GRM_MIN_COHORT, conf.numPc + 1)
            if kept.size - gone.size < least:
                raise SystemExit("VariantsPcaDriver: --grm --grm-cutoff-remove leaves %d of %d samples, fewer than the %d a GRM "
                                 "engine with %d principal components needs" % (kept.size - gone.size, kept.size, least, conf.numPc))
            stay = np.setdiff1d(np.arange(kept.size), gone)
            eng = replace(grm_subset_engine(eng, stay, min_maf, err=err))
            kept = kept[stay]
            pruned = False
    if conf.grm_king_cutoff is not None:
        # --grm-king-cutoff: where --grm-cutoff runs, on the variants that would be decomposed (rows used) or on all of them
        if conf.grm_ld_window and not pruned:
            grm_ld_prune(conf, eng, meta)
            pruned = True
        gone = grm_screen_king(conf, eng, [driver.names[reverse[int(i)]] for i in kept], err=err)
        if gone.size:
            least = max(GRM_MIN_COHORT, conf.numPc + 1)
            if kept.size - gone.size < least:
                raise SystemExit("VariantsPcaDriver: --grm --grm-king-remove leaves %d of %d samples, fewer than the %d a GRM "
                                 "engine with %d principal components needs" % (kept.size - gone.size, kept.size, least, conf.numPc))
            stay = np.setdiff1d(np.arange(kept.size), gone)
            eng = replace(grm_subset_engine(eng, stay, min_maf, err=err))
            kept = kept[stay]
            pruned = False
    done, iterations, sigma = 0, conf.grm_outlier_iterations, conf.grm_outlier_sigma
    while True:
        if conf.grm_ld_window and not pruned:
            grm_ld_prune(conf, eng, meta)
        pruned = False
        comps, lam, nonzero = eng.compute(conf.numPc)
        if done == iterations:
            break
        removed = outlier_rule(comps.T, sigma)
        gone = kept[removed]
        err.write("Outlier round %d: removed %d sample(s)%s\n"
                  % (done + 1, gone.size, (": " + ", ".join(driver.names[reverse[int(i)]] for i in gone)) if gone.size else ""))
        if gone.size == 0:
            break
        least = max(GRM_MIN_COHORT, conf.numPc + 1)
        if kept.size - gone.size < least:
            raise SystemExit("VariantsPcaDriver: --grm-outlier-iterations: round %d would leave %d of %d samples, fewer than the "
                             "%d a GRM engine with %d principal components needs; raise --grm-outlier-sigma"
                             % (done + 1, kept.size - gone.size, kept.size, least, conf.numPc))
        eng = replace(grm_subset_engine(eng, np.nonzero(~removed)[0], min_maf, err=err))
        kept = kept[~removed]
        done += 1
    driver.last_pca = (comps, lam)
    print("Non zero rows in matrix: %d / %d." % (nonzero, kept.size))  # :208, once, for the final cohort
    return [(reverse[int(i)], float(comps[a, 0]), float(comps[a, 1])) for a, i in enumerate(kept)], eng, kept


def grm_project_removed(driver, full, eng, kept, err=None, never=None):
    """--grm-project-removed: the samples of the whole fileset that are not in the final cohort, as one study subset of the
    ORIGINAL engine, on the final panel's axes.  never: the samples --grm-mind took out, which are not placed (a sparsely called
    sample is what a mean-imputed projection misplaces) unless --grm-project-lsq places by least squares.  Returns [(callset id,
    name, pc1, pc2)] in index order."""
    removed = np.setdiff1d(np.arange(len(driver.indexes)), kept)
    if never is not None and not driver.conf.grm_project_lsq:
        removed = np.setdiff1d(removed, never)
    driver.last_placed = None
    if removed.size == 0:
        return []
    comps, lam = driver.last_pca
    reverse = dict((v, k) for (k, v) in driver.indexes.items())
    with grm_subset_engine(full, removed, 0.0, study=True, err=err) as study:
        coords, placed = grm_place(driver.conf, eng, study, comps, lam, "removed ", [driver.names[reverse[int(i)]] for i in removed], err)
    driver.last_placed = (removed[np.asarray(placed, dtype=bool)], np.asarray(coords)[np.asarray(placed, dtype=bool)])
    return [(reverse[int(i)], driver.names[reverse[int(i)]], float(coords[q, 0]), float(coords[q, 1])) for q, i in enumerate(removed)
            if placed[q]]


def grm_ld_prune(conf, eng, meta, out=None):
    """--grm-ld-window: pcoa_grm_ld_prune over the fed store with a break in front of the first variant of every new contig
    (meta: (contig, position, id) per row), the stdout line, and the --grm-ld-output-path file."""
    total = eng.grm_info()[0]
    contigs = [m[0] for m in meta] if meta and len(meta) == total else None
    breaks = [v for v in range(1, total) if contigs[v] != contigs[v - 1]] if contigs else []
    cand, kept = eng.grm_ld_prune(conf.grm_ld_window, conf.grm_ld_r2, breaks)
    (out or sys.stdout).write("GRM LD pruning: kept %d of %d candidate variants (%d in the store), window %d, r2 %g\n"
                              % (kept, cand, total, conf.grm_ld_window, conf.grm_ld_r2))
    if conf.grm_ld_output_path:
        write_ld_mask(conf.grm_ld_output_path, meta if contigs else None, eng.grm_ld_mask())


def check_gram_conf(conf):
    """--gram implicit: one operator engine holds the carrier bitsets of every variant.  What needs S, or several engines, is
    refused before any file is read or any device is touched."""
    if conf.gram != "implicit":
        return
    if conf.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("VariantsPcaDriver: --gram implicit runs on one operator engine: it cannot take --gpus %d"
                         % max(conf.gpus, int(os.environ.get("WORLD_SIZE", "1"))))
    if conf.layout == "strips":
        raise SystemExit("VariantsPcaDriver: --gram implicit holds no similarity matrix to tile: it cannot take --layout strips")
    if conf.project_input_path:
        raise SystemExit("VariantsPcaDriver: --gram implicit holds no similarity matrix to project against: it cannot take "
                         "--project-input-path")
    if conf.dump_similarity:
        raise SystemExit("VariantsPcaDriver: --gram implicit never forms the similarity matrix: it cannot take --dump-similarity")


STRIPS_REFUSE_OUTLIERS = ("--outlier-iterations subsets one whole similarity matrix on one engine: it cannot take --layout "
                          "strips")


def check_outlier_conf(conf):
    """--outlier-iterations / --outlier-sigma: what cannot be served is refused before any file is read or any engine exists."""
    k, x = conf.outlier_iterations, conf.outlier_sigma
    if k < 0:
        raise SystemExit("VariantsPcaDriver: --outlier-iterations must be >= 0 (0 = off)")
    if not (x > 0 and x != float("inf")):
        raise SystemExit("VariantsPcaDriver: --outlier-sigma must be a finite number > 0 (the threshold of --outlier-iterations)")
    if k == 0:
        return
    if conf.gram == "implicit":
        raise SystemExit("VariantsPcaDriver: --outlier-iterations subsets a stored similarity matrix: it cannot take --gram implicit")
    if conf.layout == "strips":
        raise SystemExit("VariantsPcaDriver: " + STRIPS_REFUSE_OUTLIERS)
    if conf.project_input_path:
        raise SystemExit("VariantsPcaDriver: --outlier-iterations decomposes the cohort it is given: it cannot take "
                         "--project-input-path")


STRIPS_REFUSE_RELATED = ("--related-min-jaccard screens one whole similarity matrix on one engine: it cannot take --layout "
                         "strips")


def check_related_conf(conf):
    """--related-min-jaccard and its companions: what cannot be served is refused before any file is read or any engine
    exists."""
    x = conf.related_min_jaccard
    if x is None:
        for flag, given in (("--related-output-path", conf.related_output_path is not None),
                            ("--related-max-pairs", conf.related_max_pairs_given), ("--remove-related", conf.remove_related)):
            if given:
                raise SystemExit("VariantsPcaDriver: %s needs --related-min-jaccard X (the screen is off without it)" % flag)
        return
    if not (x > 0 and x <= 1):   # (NaN fails both comparisons)
        raise SystemExit("VariantsPcaDriver: --related-min-jaccard must be a finite number in (0, 1]")
    if conf.related_max_pairs < 0:
        raise SystemExit("VariantsPcaDriver: --related-max-pairs must be >= 0 (the pairs --related-min-jaccard may report)")
    if conf.gram == "implicit":
        raise SystemExit("VariantsPcaDriver: --related-min-jaccard screens a stored similarity matrix: it cannot take --gram implicit")
    if conf.layout == "strips":
        raise SystemExit("VariantsPcaDriver: " + STRIPS_REFUSE_RELATED)
    if conf.project_input_path:
        raise SystemExit("VariantsPcaDriver: --related-min-jaccard screens the cohort it decomposes: it cannot take "
                         "--project-input-path")


STRIPS_REFUSE_KING = "--king-cutoff screens five whole Gram matrices on one device: it cannot take --layout strips"


def check_king_conf(conf):
    """--king-cutoff and its companions: what cannot be served is refused before any file is read or any engine exists."""
    x = conf.king_cutoff
    if x is None:
        for flag, given in (("--king-output-path", conf.king_output_path is not None),
                            ("--king-max-pairs", conf.king_max_pairs_given), ("--king-remove", conf.king_remove)):
            if given:
                raise SystemExit("VariantsPcaDriver: %s needs --king-cutoff X (the screen is off without it)" % flag)
        return
    if not (x > 0 and x <= 0.5):   # (NaN fails both comparisons)
        raise SystemExit("VariantsPcaDriver: --king-cutoff must be a finite number in (0, 0.5]")
    if conf.king_max_pairs < 0:
        raise SystemExit("VariantsPcaDriver: --king-max-pairs must be >= 0 (the pairs --king-cutoff may report)")
    if conf.gram == "implicit":
        raise SystemExit("VariantsPcaDriver: --king-cutoff screens stored Gram matrices: it cannot take --gram implicit")
    if conf.layout == "strips":
        raise SystemExit("VariantsPcaDriver: " + STRIPS_REFUSE_KING)
    world = max(conf.gpus, int(os.environ.get("WORLD_SIZE", "1")))
    if world > 1:
        raise SystemExit("VariantsPcaDriver: --king-cutoff runs on one engine and its five planes: it cannot take --gpus %d" % world)
    if conf.ld_window:
        raise SystemExit("VariantsPcaDriver: --king-cutoff: the planes would need the pruned rows: it cannot take --ld-window")
    if conf.related_min_jaccard is not None:
        raise SystemExit("VariantsPcaDriver: --king-cutoff: one relatedness screen per run: it cannot take --related-min-jaccard")
    if conf.project_input_path:
        raise SystemExit("VariantsPcaDriver: --king-cutoff screens the cohort it decomposes: it cannot take --project-input-path")
    paths = conf.inputPath or []
    if conf.synthetic or conf.minAlleleFrequency is not None or len(paths) != 1 or not is_plink_path(paths[0]):
        raise SystemExit("VariantsPcaDriver: --king-cutoff reads the genotype classes of one PLINK fileset: --input-path must name a "
                         "single .bed / .bim / .fam (VCF ingest yields carriers only)")


class KingPlanes(object):
    """The five plane engines of --king-cutoff (PCOA_KING_*): created together, fed together, closed together."""

    def __init__(self, n, device=0):
        self.engines = []
        try:
            for _ in KING_PLANES:
                self.engines.append(PcoaEngine(n, device=device))
        except Exception:
            self.close()
            raise

    def accumulate(self, rows):
        PcoaEngine.accumulate_plink_bed_king(self.engines, rows)

    def king_pairs(self, x, capacity):
        return PcoaEngine.king_pairs(self.engines, x, capacity=capacity)

    def close(self):
        for e in self.engines:
            e.close()
        self.engines = []


def king_accumulate(call_rdd, matrix_size, device=0):
    """--king-cutoff: the blocks of raw .bed rows the main engine was fed, fed to the five planes
    (pcoa_accumulate_plink_bed_king).  Returns the KingPlanes."""
    _, geno, keep, _ = call_rdd
    king = KingPlanes(matrix_size, device=device)
    all_kept = bool(keep.all())
    for v0 in range(0, geno.shape[0], PLINK_BLOCK_ROWS):
        rows = geno[v0:v0 + PLINK_BLOCK_ROWS]
        if not all_kept:
            k = keep[v0:v0 + PLINK_BLOCK_ROWS]
            if not k.any():
                continue
            rows = rows[k]
        king.accumulate(np.ascontiguousarray(rows))
    return king


STRIPS_REFUSE_MEASURE = ("--similarity-measure %s needs the diagonal of one whole similarity matrix on one engine: it cannot "
                         "take --layout strips")


def check_measure_conf(conf):
    """--similarity-measure: an unknown name, and what a measure cannot serve, is refused before any file is read or any
    engine exists."""
    m = conf.similarity_measure
    if m not in SIMILARITY_MEASURES:
        raise SystemExit("VariantsPcaDriver: --similarity-measure takes shared, jaccard or cosine, not '%s'" % m)
    if m == "shared":
        return
    if conf.gram == "implicit":
        raise SystemExit("VariantsPcaDriver: --similarity-measure %s is evaluated from a stored similarity matrix: it cannot take "
                         "--gram implicit" % m)
    if conf.layout == "strips":
        raise SystemExit("VariantsPcaDriver: " + STRIPS_REFUSE_MEASURE % m)
    if conf.project_input_path:
        raise SystemExit("VariantsPcaDriver: --similarity-measure %s: projection under a measure is not built: it cannot take "
                         "--project-input-path" % m)


STRIPS_REFUSE_MISSING = ("--missing-calls pairwise needs two whole similarity matrices on one device: it cannot take --layout "
                         "strips")


def is_plink_path(path):
    return path[-4:] in (".bed", ".bim", ".fam")


def check_missing_conf(conf):
    """--missing-calls: an unknown value, and what the pairwise-complete similarity cannot serve, is refused before any file
    is read or any engine exists."""
    m = conf.missing_calls
    if m not in MISSING_CALLS:
        raise SystemExit("VariantsPcaDriver: --missing-calls takes ignore or pairwise, not '%s'" % m)
    if m == "ignore":
        if conf.call_rate_output_path:
            raise SystemExit("VariantsPcaDriver: --call-rate-output-path needs --missing-calls pairwise")
        return
    if conf.gram == "implicit":
        raise SystemExit("VariantsPcaDriver: --missing-calls pairwise is evaluated from two stored similarity matrices: it cannot "
                         "take --gram implicit")
    if conf.layout == "strips":
        raise SystemExit("VariantsPcaDriver: " + STRIPS_REFUSE_MISSING)
    if conf.gpus > 1:
        raise SystemExit("VariantsPcaDriver: --missing-calls pairwise runs on one engine and its companion: it cannot take --gpus %d"
                         % conf.gpus)
    if conf.project_input_path:
        raise SystemExit("VariantsPcaDriver: --missing-calls pairwise: projection under the pairwise-complete similarity is not "
                         "built: it cannot take --project-input-path")
    if conf.similarity_measure != "shared":
        raise SystemExit("VariantsPcaDriver: --missing-calls pairwise: its combination with a measure is not built: it cannot take "
                         "--similarity-measure %s" % conf.similarity_measure)
    if conf.ld_window:
        raise SystemExit("VariantsPcaDriver: --missing-calls pairwise: LD pruning in front of a paired accumulation is not built: it "
                         "cannot take --ld-window")
    if conf.loadings_output_path:
        raise SystemExit("VariantsPcaDriver: --missing-calls pairwise: the decomposed matrix is no longer (X J)^T (X J): it cannot "
                         "take --loadings-output-path")
    paths = conf.inputPath or []
    if conf.synthetic or conf.minAlleleFrequency is not None or len(paths) != 1 or not is_plink_path(paths[0]):
        raise SystemExit("VariantsPcaDriver: --missing-calls pairwise reads the missing calls of one PLINK fileset: --input-path must "
                         "name a single .bed / .bim / .fam (missing calls from VCF ingest are not built)")


def write_call_rates(path, names, called, n_variants):
    """The --call-rate-output-path file: one line per sample in callset order -- name, called variants c_i, variants fed V,
    c_i / V with six decimals (0.000000 where V = 0), tab-separated."""
    with open(path, "w") as f:
        for name, c in zip(names, called):
            f.write("%s\t%d\t%d\t%.6f\n" % (name, int(c), int(n_variants), (float(c) / float(n_variants)) if n_variants else 0.0))


LD_MAX_WINDOW = 1024   # PCOA_LD_MAX_WINDOW
LD_DEFAULT_R2 = 0.2


def check_ld_conf(conf):
    """--ld-window: the windows run over the variants in feed order in front of one engine; everything else is refused before
    any file is read or any device is touched."""
    if conf.ld_window == 0:
        if conf.ld_output_path:
            raise SystemExit("VariantsPcaDriver: --ld-output-path needs --ld-window W (the pruning is off without it)")
        if conf.ld_r2 is not None:
            raise SystemExit("VariantsPcaDriver: --ld-r2 needs --ld-window W (the pruning is off without it)")
        return
    if not 1 <= conf.ld_window <= LD_MAX_WINDOW:
        raise SystemExit("VariantsPcaDriver: --ld-window takes a number of variants in [1, %d] (0: off), not '%d'"
                         % (LD_MAX_WINDOW, conf.ld_window))
    if conf.ld_r2 is None:
        conf.ld_r2 = LD_DEFAULT_R2
    if not 0.0 <= conf.ld_r2 <= 1.0:      # (NaN fails both comparisons)
        raise SystemExit("VariantsPcaDriver: --ld-r2 takes a threshold in [0, 1], not '%s'" % conf.ld_r2)
    world = max(conf.gpus, int(os.environ.get("WORLD_SIZE", "1")))
    if world > 1:
        raise SystemExit("VariantsPcaDriver: --ld-window: variant shards would cut the windows: it cannot take --gpus %d" % world)
    if conf.layout == "strips":
        raise SystemExit("VariantsPcaDriver: --ld-window runs in front of one engine's accumulation: it cannot take --layout strips")
    paths = conf.inputPath if isinstance(conf.inputPath, (list, tuple)) else [conf.inputPath]
    if len(paths) > 1:
        raise SystemExit("VariantsPcaDriver: --ld-window takes one input set: joined and merged sets reach the engine in "
                         "hash-partition order, not in feed order")
    if conf.project_input_path:
        raise SystemExit("VariantsPcaDriver: --ld-window prunes the cohort it decomposes: it cannot take --project-input-path")


def ld_accumulate(engine, rows, meta, window, r2_max):
    """--ld-window: the rows of calls_as_bits through the pruner with PCOA_LD_ACCUMULATE, a break wherever the contig of the next
    variant differs from the last one's (meta: (contig, position, id) per row, or none).  Returns (keep mask, pruner stats)."""
    if rows[0] == "bed":
        _, geno, ref_keep, ref_is_a1 = rows
        at = np.flatnonzero(ref_keep)
        total = int(at.size)
        block = lambda a, b: np.ascontiguousarray(geno[at[a:b]])
    else:
        bits = rows[1]
        total = int(bits.shape[0])
        block = lambda a, b: bits[a:b]
    contigs = [m[0] for m in meta] if meta and len(meta) == total else None
    edges = [0] + ([v for v in range(1, total) if contigs[v] != contigs[v - 1]] if contigs else []) + [total]
    parts = []
    with engine.ld_pruner(window, r2_max, accumulate=True) as pr:
        for k, (s, e) in enumerate(zip(edges[:-1], edges[1:])):
            if k > 0:
                pr.break_contig()
            for a in range(s, e, PLINK_BLOCK_ROWS):
                b = min(e, a + PLINK_BLOCK_ROWS)
                parts.append(pr.plink_bed(block(a, b), ref_is_a1=ref_is_a1) if rows[0] == "bed" else pr.bits(block(a, b)))
        stats = pr.stats()
    engine.finalize()
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=bool)), stats


def write_ld_mask(path, meta, keep):
    """The --ld-output-path file: one line per fed variant in feed order -- 0-based index, contig, position, variant id (as
    --loadings-output-path records them; '.' where the input carries none), 1 (kept) or 0, tab-separated."""
    if meta and len(meta) != len(keep):
        raise RuntimeError("--ld-output-path: %d variant records for %d rows" % (len(meta), len(keep)))
    with open(path, "w") as f:
        for v in range(len(keep)):
            contig, pos, vid = meta[v] if meta else (".", ".", ".")
            f.write("%d\t%s\t%s\t%s\t%d\n" % (v, contig, pos, vid, 1 if keep[v] else 0))


def check_loadings_conf(conf):
    """--loadings-output-path: the identity B = (X J)^T (X J) behind the loadings holds for the shared counts of the whole
    cohort on one engine; everything else is refused before any file is read or any device is touched."""
    if not conf.loadings_output_path:
        return
    world = max(conf.gpus, int(os.environ.get("WORLD_SIZE", "1")))
    if world > 1:
        raise SystemExit("VariantsPcaDriver: --loadings-output-path streams the variants past one engine: it cannot take --gpus %d"
                         % world)
    if conf.layout == "strips":
        raise SystemExit("VariantsPcaDriver: --loadings-output-path runs on one whole engine: it cannot take --layout strips")
    if conf.project_input_path:
        raise SystemExit("VariantsPcaDriver: --loadings-output-path writes the loadings of the cohort it decomposes: it cannot "
                         "take --project-input-path")
    if conf.outlier_iterations > 0:
        raise SystemExit("VariantsPcaDriver: --loadings-output-path needs the eigenpairs of the cohort the variants were counted "
                         "over: it cannot take --outlier-iterations %d" % conf.outlier_iterations)
    if conf.remove_related:
        raise SystemExit("VariantsPcaDriver: --loadings-output-path needs the eigenpairs of the cohort the variants were counted "
                         "over: it cannot take --remove-related")
    if conf.similarity_measure != "shared":
        raise SystemExit("VariantsPcaDriver: --loadings-output-path: under --similarity-measure %s the decomposed matrix is no "
                         "longer (X J)^T (X J); it takes --similarity-measure shared only" % conf.similarity_measure)


def calls_as_bits(call_rdd, n, flag="--gram implicit", instead="--gram stored"):
    """--gram implicit: an RDD[Seq[Int]] in any of the forms getCallsRdd returns, as what an operator engine stores -- raw
    PLINK rows and bitsets as they are, carrier lists packed into bitsets.  A list that names a callset twice (a merge of sets
    with a repeated key; the reference counts it with multiplicity, VariantsPca.scala:187) cannot be a bitset: refused."""
    if isinstance(call_rdd, tuple) and isinstance(call_rdd[0], str):
        return call_rdd
    if isinstance(call_rdd, tuple):
        idx, offs = np.asarray(call_rdd[0], dtype=np.int64), np.asarray(call_rdd[1], dtype=np.int64)
        idx = idx[offs[0]:offs[-1]]
        rows = np.repeat(np.arange(offs.size - 1, dtype=np.int64), np.diff(offs))
    else:
        rows = np.repeat(np.arange(len(call_rdd), dtype=np.int64), [len(c) for c in call_rdd])
        idx = np.fromiter((i for c in call_rdd for i in c), dtype=np.int64, count=int(rows.size))
    n_rows = (len(call_rdd[1]) - 1) if isinstance(call_rdd, tuple) else len(call_rdd)
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise IndexError("callset index outside [0, %d) in a carrier list" % n)   # mapping(call.callsetId) throws (:59)
    key = rows * n + idx
    if np.unique(key).size != key.size:
        raise SystemExit("VariantsPcaDriver: %s: a carrier list names a callset twice; a carrier bitset cannot carry "
                         "that multiplicity -- use %s" % (flag, instead))
    bits = np.zeros((n_rows, (n + 31) // 32), dtype=np.uint32)
    np.bitwise_or.at(bits, (rows, idx >> 5), (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return ("bits", bits)


def check_projection_conf(conf):
    """--project-input-path: what cannot be served is refused before any file is read or any device is touched."""
    from . import ingest
    if conf.gpus > 1:
        raise SystemExit("VariantsPcaDriver: --project-input-path runs on one GPU: it cannot take --gpus %d" % conf.gpus)
    if conf.layout == "strips":
        raise SystemExit("VariantsPcaDriver: --project-input-path needs the reference's S whole on one engine: it cannot take "
                         "--layout strips")
    if conf.synthetic or not conf.inputPath:
        raise SystemExit("VariantsPcaDriver: --project-input-path needs VCF inputs on both sides (--input-path)")
    stems = set()
    for k, path in enumerate(list(conf.inputPath) + list(conf.project_input_path)):
        if path.endswith(".npz") or path[-4:] in (".bed", ".bim", ".fam"):
            raise SystemExit("VariantsPcaDriver: --project-input-path needs VCF inputs on both sides: %s is not a VCF" % path)
        stem = ingest.set_id_of(path)
        if k >= len(conf.inputPath) and stem in stems:
            raise SystemExit("VariantsPcaDriver: --project-input-path: callset-id collision: %s has the set id '%s' of an earlier "
                             "input (callset ids are <set id>-<column>); rename the file" % (path, stem))
        stems.add(stem)


def main_projection(conf):
    """--project-input-path: the PCA of the --input-path cohort on a full engine over N_ref, the other samples placed onto it
    (pcoa_project) from a strip owner over columns [N_ref, N).  Lists go to the strip whole and, filtered to indexes < N_ref,
    to the reference engine."""
    from . import ingest
    ref_paths, proj_paths = list(conf.inputPath), list(conf.project_input_path)
    refs = None if conf.all_references else conf.references
    if len(ref_paths) > 1:
        print("Running PCA on %d datasets." % len(ref_paths))  # VariantsCommon.scala:57
    indexes, names, data, used = {}, {}, [], set()
    n_ref = 0
    for k, path in enumerate(ref_paths + proj_paths):
        set_id = ingest.set_id_of(path, k, used)
        ids, nm, variants = ingest.load_vcf_records(path, parse_refs(refs, k), set_id=set_id)
        base = len(indexes)
        for i, cid in enumerate(ids):
            indexes[cid] = base + i
        names.update(nm)
        data.append(variants)
        if k + 1 == len(ref_paths):
            n_ref = len(indexes)
    n = len(indexes)
    driver = VariantsPcaDriver(conf, indexes, names, data, matrix_size=n_ref)
    if n_ref == 0 or n == n_ref:
        raise SystemExit("VariantsPcaDriver: --project-input-path: both the reference and the projected inputs need samples")
    if conf.numPc < 2:
        raise IndexError("computePca emits exactly PC1 and PC2 (VariantsPca.scala:229-230); --num-pc must be >= 2")
    filtered = [driver.filterDataset(d) for d in driver.data]
    rows = driver.getCallsRdd(filtered)
    for r in rows:
        if len(set(r)) != len(r):
            raise SystemExit("VariantsPcaDriver: --project-input-path: a joined variant names a callset twice; a carrier bitset "
                             "cannot carry that multiplicity")
    ref = PcoaEngine(n_ref, device=conf.gpu)
    cross = PcoaEngine(n, device=conf.gpu, strip=(n_ref, n - n_ref))
    driver.engine = ref
    try:
        calculate_similarity_matrix([[i for i in r if i < n_ref] for r in rows], n_ref, engine=ref)
        calculate_similarity_matrix(rows, n, engine=cross)
        if conf.dump_similarity:
            ref.gram().astype("<i8").tofile(conf.dump_similarity)
        comps, lam, nonzero = ref.compute(conf.numPc)
        print("Non zero rows in matrix: %d / %d." % (nonzero, n_ref))  # :208
        coords = ref.project(cross, comps, lam)
        print("Projected %d samples onto %d principal components of %d reference samples." % (n - n_ref, conf.numPc, n_ref))
        reverse = dict((v, k) for (k, v) in indexes.items())
        result = [(reverse[i], float(comps[i, 0]), float(comps[i, 1])) for i in range(n_ref)]
        result += [(reverse[n_ref + q], float(coords[q, 0]), float(coords[q, 1])) for q in range(n - n_ref)]
        driver.emitResult(result)
        driver.reportIoStats(sys.stderr)
    finally:
        cross.close()
        driver.stop()
    return 0


def main(args):
    """VariantsPcaDriver.main (VariantsPca.scala:38-50)."""
    conf = PcaConf(args)
    check_grm_conf(conf)
    check_outlier_conf(conf)
    check_related_conf(conf)
    check_king_conf(conf)
    check_measure_conf(conf)
    check_missing_conf(conf)
    check_gram_conf(conf)
    check_loadings_conf(conf)
    check_ld_conf(conf)
    if conf.project_input_path:
        check_projection_conf(conf)
        return main_projection(conf)
    rank, world = 0, 1
    if conf.gpus > 1 or "WORLD_SIZE" in os.environ:
        import torch  # plumbing: rendezvous and the device count
        what, detail = multi_gpu_plan(conf, args, os.environ, torch.cuda.device_count())
        if what == "error":
            raise SystemExit("VariantsPcaDriver: " + detail)
        if what == "spawn":
            import subprocess
            env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
            return subprocess.call(detail, env=env)
        world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import torch
        import torch.distributed as td
        rank = int(os.environ.get("RANK", "0"))
        local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
        if conf.rank_devices:
            local_rank = [int(t) for t in conf.rank_devices.split(",")][rank]
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local_rank)
        if conf.dist_backend == "gloo":
            conf.allreduce = "torch"   # the library's communicator is RCCL
            td.init_process_group("gloo", rank=rank, world_size=world)
        else:
            td.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        quiet = open(os.devnull, "w") if rank != 0 else None   # the reference's driver prints once
        if quiet is not None:
            sys.stdout = quiet
    # (contig, position, id) per row, recorded only with a flag that needs them (--ld-window: the contigs place the breaks)
    variant_meta = [] if (conf.loadings_output_path or conf.ld_window or conf.grm_weights_output_path or conf.grm_ld_window
                          or conf.grm_variant_qc_output_path) else None
    indexes, names, data = load_dataset(conf, variant_meta)
    grm_order, grm_listed = None, None
    if conf.grm:   # --grm-keep-samples / --grm-remove-samples: a wrong list is refused before anything is printed or any engine exists
        grm_order = sorted(indexes.items(), key=lambda kv: kv[1])   # the engine's index order: the .fam's
        grm_listed = grm_sample_list(conf, [names[cid] for cid, _ in grm_order])
    driver = VariantsPcaDriver(conf, indexes, names, data)
    filtered = [driver.filterDataset(d) for d in driver.data]
    calls_rdd = driver.getCallsRdd(filtered, variant_meta)
    n = len(driver.indexes)
    ld_rows = None
    if conf.ld_window:   # the pruner's rows, and the refusal of a repeated callset, before any device work
        ld_rows = calls_as_bits(calls_rdd, n, flag="--ld-window", instead="carrier lists that are sets")

    def ld_ingest(engine):
        keep, st = ld_accumulate(engine, ld_rows, variant_meta, conf.ld_window, conf.ld_r2)
        print("LD pruning: kept %d of %d variants (%d monomorphic)" % (st["ld_kept"], st["ld_variants"], st["ld_monomorphic"]))
        if conf.ld_output_path:
            write_ld_mask(conf.ld_output_path, variant_meta, keep)
        return engine

    if conf.grm:
        order, listed = grm_order, grm_listed
        full = driver.engine = grm_accumulate(calls_rdd, n, conf.grm_min_maf or 0.0, device=conf.gpu,
                                              max_missing=1.0 if conf.grm_geno is None else conf.grm_geno,
                                              hwe_min_p=0.0 if conf.grm_hwe is None else conf.grm_hwe)
        mind_gone = None
        if (conf.grm_geno is not None or conf.grm_hwe is not None or conf.grm_mind is not None or conf.grm_variant_qc_output_path
                or conf.grm_sample_qc_output_path):
            mind_kept = grm_qc(conf, full, [names[cid] for cid, _ in order], variant_meta)
            if mind_kept is not None and mind_kept.size < n:
                mind_gone = np.setdiff1d(np.arange(n), mind_kept)
                listed = mind_kept if listed is None else np.intersect1d(listed, mind_kept)
                least = max(GRM_MIN_COHORT, conf.numPc + 1)
                if listed.size < least:
                    raise SystemExit("VariantsPcaDriver: --grm --grm-mind leaves %d of %d samples, fewer than the %d a GRM engine "
                                     "with %d principal components needs" % (listed.size, n, least, conf.numPc))
        if listed is None and conf.grm_outlier_iterations == 0 and conf.grm_cutoff is None and conf.grm_king_cutoff is None:
            if conf.grm_ld_window:
                grm_ld_prune(conf, driver.engine, variant_meta)
            result, kept = driver.computePca(driver.engine), np.arange(n)
        else:
            result, _, kept = grm_compute_rounds(driver, full, listed, variant_meta)
        comps, lam = driver.last_pca
        study = grm_project_study(conf, driver.engine, comps, lam) if conf.grm_project_path else []
        if conf.grm_project_removed:
            study = study + grm_project_removed(driver, full, driver.engine, kept, never=mind_gone)
        if conf.grm_pcrelate_output_path is not None:
            grm_pcrelate(driver, full, driver.engine, kept, variant_meta)
        if conf.grm_project_removed and full is not driver.engine:
            full.close()
        driver.emitResult(result, study=study or None)
        if conf.grm_weights_output_path:
            write_loadings(conf.grm_weights_output_path, variant_meta, driver.engine.grm_weights(comps, lam, scaled=True))
        if conf.grm_output_path:
            grm_write_output(conf, driver.engine, [(order[int(i)][0].split("-")[0], driver.names[order[int(i)][0]]) for i in kept])
        driver.reportIoStats(sys.stderr)
        driver.stop()
        return 0
    if conf.gram == "implicit":
        if conf.ld_window:
            driver.engine = ld_ingest(PcoaEngine(n, device=conf.gpu, operator=True))
        else:
            driver.engine = calculate_similarity_matrix(calls_as_bits(calls_rdd, n), n,
                                                        engine=PcoaEngine(n, device=conf.gpu, operator=True))
        result = driver.computePca(driver.engine)
        driver.emitResult(result)
        if conf.loadings_output_path:   # (--ld-window: every variant read gets its line, so the rows are streamed again)
            driver.emitLoadings(ld_rows, variant_meta)
        driver.reportIoStats(sys.stderr)
        driver.stop()
        return 0
    loadings_rows = None
    if conf.loadings_output_path:   # the second pass's rows, and the refusal of a repeated callset, before any device work
        loadings_rows = calls_as_bits(calls_rdd, n, flag="--loadings-output-path", instead="carrier lists that are sets")
    if world > 1:
        import torch.distributed as td
        devices = [int(t) for t in conf.rank_devices.split(",")] if conf.rank_devices else list(range(world))
        decided = [resolve_layout(conf, n, world, devices) if rank == 0 else None]
        td.broadcast_object_list(decided, src=0)      # every rank takes rank 0's decision (free memory differs by the moment)
        ranges = decided[0]
    else:
        ranges = resolve_layout(conf, n, 1, [conf.gpu])
    if ranges is not None and conf.outlier_iterations > 0:   # --layout auto resolved to strips
        raise SystemExit("VariantsPcaDriver: " + STRIPS_REFUSE_OUTLIERS)
    if ranges is not None and conf.related_min_jaccard is not None:
        raise SystemExit("VariantsPcaDriver: " + STRIPS_REFUSE_RELATED)
    if ranges is not None and conf.king_cutoff is not None:     # --layout auto resolved to strips
        raise SystemExit("VariantsPcaDriver: " + STRIPS_REFUSE_KING)
    if ranges is not None and conf.similarity_measure != "shared":
        raise SystemExit("VariantsPcaDriver: " + STRIPS_REFUSE_MEASURE % conf.similarity_measure)
    if ranges is not None and conf.missing_calls == "pairwise":   # --layout auto resolved to strips
        raise SystemExit("VariantsPcaDriver: " + STRIPS_REFUSE_MISSING)
    if ranges is not None and conf.ld_window:
        raise SystemExit("VariantsPcaDriver: --ld-window runs in front of one engine's accumulation: it cannot take --layout strips")
    if ranges is not None and conf.loadings_output_path:     # --layout auto resolved to strips
        raise SystemExit("VariantsPcaDriver: --loadings-output-path runs on one whole engine: it cannot take --layout strips")
    if ranges is not None:
        owner = driver.getSimilarityMatrixStrip(calls_rdd, ranges[rank], local_rank if world > 1 else conf.gpu)
        if rank == 0:
            sys.stderr.write("strip layout: %d owner(s), each fed every variant, no reduction; columns %s\n"
                             % (world, ", ".join("[%d, %d) on device %d" % (c0, c0 + w, d) for (c0, w), d in
                                                 zip(ranges, devices if world > 1 else [conf.gpu]))))
        if conf.dump_similarity:
            s = gather_strips(owner)
            if rank == 0:
                s.astype("<i8").tofile(conf.dump_similarity)
        result = driver.computePcaOverStrips(owner, world, host_exchange=world > 1 and conf.dist_backend == "gloo")
        if rank == 0:
            driver.emitResult(result)
            driver.reportIoStats(sys.stderr)
        if world > 1:
            td.barrier()
            td.destroy_process_group()
        driver.stop()
        return 0
    if world > 1:
        sim_matrix, tele = driver.getSimilarityMatrixSharded(calls_rdd, rank, world, local_rank, conf.allreduce)
        if rank == 0:
            sys.stderr.write("Reduced over %d ranks (RCCL communicator: %s ranks): all-reduce %.3f ms; per-rank accumulate "
                             "%.3f .. %.3f s\n" % (world, tele["rccl_ranks"], tele["allreduce_ms"], tele["rank_elapsed_min_s"],
                                                   tele["rank_elapsed_max_s"]))
    elif conf.ld_window:
        sim_matrix = driver.engine = ld_ingest(PcoaEngine(n, device=conf.gpu))
    elif conf.missing_calls == "pairwise":
        sim_matrix, driver.companion, fed = calculate_similarity_matrix_calls(calls_rdd, n, device=conf.gpu)
        driver.engine = sim_matrix
    else:
        sim_matrix = driver.getSimilarityMatrix(calls_rdd)
    if rank == 0:
        if conf.dump_similarity:
            sim_matrix.gram().astype("<i8").tofile(conf.dump_similarity)
        if conf.similarity_measure != "shared":    # on the engine that runs computePca; its subsets inherit it
            sim_matrix.set_similarity(conf.similarity_measure)
        if conf.missing_calls == "pairwise":       # bound just before the screen and the rounds; the subsets get their own
            missing = driver.companion.similar_pairs(1.0, capacity=0)[2]      # diag(Q): the missing calls of every sample
            sim_matrix.set_call_companion(driver.companion, fed)
            print("Missing calls: %d of %d genotypes (pairwise-complete similarity)" % (int(missing.sum()), fed * n))
            if conf.call_rate_output_path:
                reverse = dict((v, k) for (k, v) in driver.indexes.items())
                write_call_rates(conf.call_rate_output_path, [driver.names[reverse[i]] for i in range(n)], fed - missing, fed)
        if conf.related_min_jaccard is not None:   # the screen first, then the rounds on the reduced cohort
            sim_matrix = driver.screenRelated(sim_matrix)
        if conf.king_cutoff is not None:           # likewise; the planes live from here to the end of the screen
            sim_matrix = driver.screenKing(sim_matrix, king_accumulate(calls_rdd, n, device=conf.gpu))
        result = driver.computePcaOutlierRounds(sim_matrix) if conf.outlier_iterations > 0 else driver.computePca(sim_matrix)
        driver.emitResult(result)
        if conf.loadings_output_path:
            driver.emitLoadings(loadings_rows, variant_meta)
        driver.reportIoStats(sys.stderr)
    if world > 1:
        import torch.distributed as td
        td.barrier()
        td.destroy_process_group()
    driver.stop()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

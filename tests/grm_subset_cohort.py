"""The numpy statement of pcoa_create_grm_subset / pcoa_grm_rows (include/pcoa.h), shared by
tests/test_grm_subset_cpu.py and tests/test_gpu_grm_subset.py: the store's rows as .bed rows, the rows of a sample subset on the
packed bytes, the keep-list patterns the gather is held to, and the planted cohort of the outlier rounds."""
import numpy as np

SWAP = np.array([3, 1, 2, 0], dtype=np.uint8)          # 00 <-> 11: a row fed with ref_is_a1 = 0 as the store codes it


def unpack_rows(packed_rows, n):
    """[V][>= ceil(n / 4)] uint8 .bed rows -> [V][n] uint8 codes (sample s in bits 2 (s % 4) of byte s / 4)."""
    rows = np.asarray(packed_rows, dtype=np.uint8)
    nb = (n + 3) // 4
    q = rows[:, :nb]
    codes = np.stack([(q >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(rows.shape[0], nb * 4)
    return np.ascontiguousarray(codes[:, :n])


def pack_rows(codes):
    """[V][n] codes -> [V][ceil(n / 4)] uint8 .bed rows, the unused slots of the last byte 00 (PLINK's convention)."""
    codes = np.asarray(codes, dtype=np.uint8)
    v, n = codes.shape
    nb = (n + 3) // 4
    full = np.zeros((v, nb * 4), dtype=np.uint8)
    full[:, :n] = codes
    q = full.reshape(v, nb, 4)
    return np.ascontiguousarray(q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6), dtype=np.uint8)


def store_rows(packed_rows, n, ref_is_a1):
    """What pcoa_grm_rows returns for an engine of n samples fed `packed_rows` with ref_is_a1: the store's one coding (a .bed row
    with ref_is_a1 = 1), whatever the padding slots and extra bytes of the input held."""
    codes = unpack_rows(packed_rows, n)
    return pack_rows(codes if ref_is_a1 else SWAP[codes])


def spec_grm_subset_rows(packed_rows, n_src, keep):
    """.bed rows of n_src samples -> .bed rows of the len(keep) samples `keep`, tail slots 00: slot a of a row is slot keep[a] of
    the source row.  Works on the packed bytes, bit by bit, without unpacking a whole row."""
    rows = np.asarray(packed_rows, dtype=np.uint8)
    keep = np.asarray(keep, dtype=np.int64)
    assert keep.ndim == 1 and (keep.size == 0 or (keep.min() >= 0 and keep.max() < n_src)) and np.all(np.diff(keep) > 0)
    m = keep.size
    out = np.zeros((rows.shape[0], (m + 3) // 4), dtype=np.uint8)
    for a in range(m):
        k = int(keep[a])
        out[:, a >> 2] |= ((rows[:, k >> 2] >> (2 * (k & 3))) & 3) << (2 * (a & 3))
    return out


def keep_patterns(n_src, seed=0):
    """name -> strictly increasing int32 index list: the issue's patterns at n_src samples."""
    rng = np.random.default_rng(1000 * seed + n_src)
    idx = np.arange(n_src, dtype=np.int32)
    mid = min(n_src - 1, 16 * ((n_src // 2) // 16) + 5)            # slot 5 of a word in the middle
    b0, b1 = n_src // 3, n_src // 3 + max(1, n_src // 4)
    pats = {
        "identity": idx,
        "first_dropped": idx[1:],
        "last_dropped": idx[:-1],
        "one_mid_word": np.delete(idx, mid),
        "every_second": idx[::2],
        "one_per_16": idx[7::16] if n_src > 7 else idx[:1],     # every output word reads 16 source words
        "block": np.delete(idx, np.arange(b0, min(b1, n_src))),
        "random_3pct": idx[rng.random(n_src) >= 0.03],
        "random_50pct": idx[rng.random(n_src) >= 0.5],
    }
    return dict((k, np.ascontiguousarray(v, dtype=np.int32)) for k, v in pats.items())


def planted_outlier_cohort(n=240, v=3000, seed=7):
    """(codes [V][n + 3], planted): a Balding-Nichols cohort of n samples in two populations plus three samples of all-het
    genotypes, placed among them.  PC1 is the population axis; the planted samples, alike among themselves and unlike everybody
    else, own PC2 (eigenvalue 3.9 against a bulk that ends at 1.5) and sit 8.8 standard deviations out on it; without them
    no sample is further out than 3.5 on either axis (tests/test_grm_subset_cpu.py holds both with numpy's eigh)."""
    from test_grm_cpu import balding_nichols
    rng = np.random.default_rng(seed)
    base = balding_nichols(rng, n, v, missing=0.0, proportions=(1, 1))
    planted = np.array([5, n // 2, n - 2], dtype=np.int64)
    total = n + 3
    codes = np.empty((v, total), dtype=np.uint8)
    rest = np.setdiff1d(np.arange(total), planted)
    codes[:, rest] = base
    codes[:, planted] = 2
    return codes, planted

"""GPU tests of the relatedness cut-off on K (pcoa_grm_pairs, --grm-cutoff): the pair list of csrc/grm_pairs.hip equals the numpy
statement variants_pca.grm_pairs_rule bit for bit on cohorts where every partial sum is an integer, equals thresholding the K
that pcoa_grm_block returns on rounded cohorts whatever the band, the accumulate calls or the segments, equals the pure-numpy
list at cutoffs that no entry comes near, keeps the capacity contract of pcoa_similar_pairs, follows the state of the ctx,
refuses what it must and leaves the ctx as it was, and both hosts write the same pair file and the same coordinates."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, load_pkg, write_golden_plink
from test_grm_cpu import balding_nichols, dosage, edge_rows, exact_cohort, pack_bed, random_codes, spec_grm_counts, spec_grm_weights

pytestmark = pytest.mark.gpu

DIVISORS = ("used", "pairwise")
BANDS = (0, 64, 128)


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def vp():
    return load_pkg("variants_pca")


def fill(eng, codes, ref_is_a1=False, cuts=None):
    rows = pack_bed(codes)
    edges = [0] + sorted(cuts or []) + [rows.shape[0]]
    for a, b in zip(edges[:-1], edges[1:]):
        eng.accumulate_plink_bed(np.ascontiguousarray(rows[a:b]), ref_is_a1=ref_is_a1)
    eng.sync()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def want_pairs(vp, k, cutoff, cnt, m, divisor):
    return vp.grm_pairs_rule(k, cutoff, cnt if divisor == "pairwise" else m)


def upper(k):
    return k[np.triu_indices(k.shape[0], 1)]


# ---- 1. exact cohorts -------------------------------------------------------------------------------------------------------
EXACT_V = [(4, 1), (64, 2), (512, 3)]


def tied_cutoffs(k):
    """cutoffs that several entries above the diagonal hit exactly: the most frequent value, the most frequent positive one and
    the largest one that occurs twice or more; and one that nothing hits (everything above it, nothing at it)"""
    vals, counts = np.unique(upper(k), return_counts=True)
    out = [vals[np.argmax(counts)]]
    pos = vals > 0
    if pos.any():
        out.append(vals[pos][np.argmax(counts[pos])])
    if (counts >= 2).any():
        out.append(vals[counts >= 2][-1])
    for c in out:
        assert (upper(k) == c).sum() >= 2
    return sorted(set(float(c) for c in out)) + [float(vals[0]) - 1.0]


@pytest.mark.parametrize("n", [32, 33, 63, 64, 65, 130, 1025])
def test_pairs_equal_the_rule_bit_for_bit_on_exact_cohorts(P, vp, n):
    """mu_v = 1 and d_v = 2: every partial sum an integer, M' a power of two: K is numpy's K bit for bit, so the list, its k and
    n and the diagonal must be numpy's whatever the band; many entries are equal, so >= against > shows at once."""
    rng = np.random.default_rng(7000 + n)
    with P.PcoaEngine(n, grm=True) as eng:
        for q, (vu, vx) in enumerate(EXACT_V):
            ref_is_a1 = bool((q + n) & 1)
            codes = exact_cohort(rng, n, vu, vx, ref_is_a1)
            eng.reset()
            fill(eng, codes, ref_is_a1)
            for divisor in DIVISORS:
                k, cnt = vp.grm_dense_rule(codes, ref_is_a1, 0.0, divisor)
                for cutoff in tied_cutoffs(k):
                    want = want_pairs(vp, k, cutoff, cnt, vu, divisor)
                    for band in BANDS:
                        got, found, diag = eng.grm_pairs(cutoff, divisor, band_rows=band, capacity=n * n, diag=True)
                        where = (n, vu, vx, divisor, cutoff, band)
                        assert found == want.size, where
                        assert same_bits(got, want), where
                        assert same_bits(diag, np.ascontiguousarray(np.diagonal(k))), where
                # the list of everything: n (n - 1) / 2 pairs in order
                assert eng.grm_pairs(-1e300, divisor, capacity=0)[1] == n * (n - 1) // 2
                assert eng.grm_pairs(1e300, divisor)[1] == 0


# ---- 2. rounded cohorts -----------------------------------------------------------------------------------------------------
def planted(rng):
    """balding_nichols 260 x 1,000 with relatives: samples 7 and 201 become copies of 3 and 100, samples 50 and 259 the
    allele-wise children of (10, 20) and (130, 140): one allele drawn from each parent's genotype"""
    codes = balding_nichols(rng, 260, 1000)
    g, c = dosage(codes, False)
    g = g.astype(np.int64)
    for dup, src in ((7, 3), (201, 100)):
        codes[:, dup] = codes[:, src]
    for child, (pa, pb) in ((50, (10, 20)), (259, (130, 140))):
        a = (rng.random(codes.shape[0]) * 2 < g[:, pa]).astype(np.int64)     # an allele of a parent with g copies: p = g / 2
        b = (rng.random(codes.shape[0]) * 2 < g[:, pb]).astype(np.int64)
        dose = a + b                                                          # copies of the non-reference allele (A1)
        kid = np.array([3, 2, 0], dtype=np.uint8)[dose]                       # A2 is the reference: 11 = 0 copies, 00 = 2
        kid[(c[:, pa] == 0) | (c[:, pb] == 0)] = 1
        codes[:, child] = kid
    return codes


PLANTED_PAIRS = [(3, 7), (100, 201), (10, 50), (20, 50), (130, 259), (140, 259)]


@pytest.fixture(scope="module")
def rounded():
    rng = np.random.default_rng(2600)
    return {"bn": planted(rng), "edge": edge_rows(random_codes(rng, 300, 130))}


def gap_cutoff(values, near):
    """the midpoint of the widest gap between consecutive sorted values among the gaps that reach into [0.8 near, 1.2 near];
    `near` itself where every value lies on one side of that window"""
    s = np.unique(values)
    touches = (s[1:] > 0.8 * near) & (s[:-1] < 1.2 * near)
    if not touches.any():
        return float(near)
    gaps = np.where(touches, s[1:] - s[:-1], -1.0)
    g = int(np.argmax(gaps))
    return float(0.5 * (s[g] + s[g + 1]))


def entry_bound(codes, n_pairs, divisor):
    """DESIGN 4.18's bound (V + 16) 2^-52 (|A|^T diag(d) |A|)_ij / divisor_ij"""
    g, c = dosage(codes, False)
    mu, d, used, m = spec_grm_weights(spec_grm_counts(codes, False), 0.0)
    a = np.abs(np.where(c == 1, g.astype(np.float64) - mu[:, None], 0.0))
    w = (a.T * d) @ a
    with np.errstate(divide="ignore", invalid="ignore"):
        w = w / float(m) if divisor == "used" else np.where(n_pairs > 0, w / n_pairs.astype(np.float64), 0.0)
    return (codes.shape[0] + 16) * 2.0 ** -52 * w


@pytest.mark.parametrize("name", ["bn", "edge"])
def test_pairs_equal_thresholding_the_block_reader_and_numpy_on_rounded_cohorts(P, vp, rounded, name):
    codes = rounded[name]
    v, n = codes.shape
    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(n, grm=True) as other:
        fill(eng, codes)
        fill(other, codes, cuts=[1, 7, 130, 131])
        m = eng.grm_info()[1]
        for divisor in DIVISORS:
            k_dev = eng.grm_dense(divisor)
            k_np, cnt = vp.grm_dense_rule(codes, False, 0.0, divisor)
            bound = entry_bound(codes, cnt, divisor)
            iu = np.triu_indices(n, 1)
            for near in (0.05, 0.35, 0.9):
                cutoff = gap_cutoff(k_np[iu], near)
                # against pcoa_grm_block of the same ctx: exact, whatever the band and the feeding
                want = want_pairs(vp, k_dev, cutoff, cnt, m, divisor)
                for band in BANDS:
                    got, found = eng.grm_pairs(cutoff, divisor, band_rows=band)
                    assert found == want.size and same_bits(got, want), (name, divisor, near, band)
                got2, found2 = other.grm_pairs(cutoff, divisor)
                assert found2 == want.size and same_bits(got2, want), (name, divisor, near)
                # against pure numpy: no entry of numpy's K lies within the bound of the cutoff, so no pair may be left out
                assert np.all(np.abs(k_np[iu] - cutoff) > bound[iu]), (name, divisor, near, cutoff)
                pure = want_pairs(vp, k_np, cutoff, cnt, m, divisor)
                assert found == pure.size, (name, divisor, near)
                assert np.array_equal(got["i"], pure["i"]) and np.array_equal(got["j"], pure["j"]) and np.array_equal(got["n"], pure["n"])
                assert np.all(np.abs(got["k"] - pure["k"]) <= bound[pure["i"], pure["j"]])
                print("%s %s near %g: cutoff %.6g, %d pair(s)" % (name, divisor, near, cutoff, found))
                if name == "bn" and near == 0.35:
                    listed = set(zip(got["i"].tolist(), got["j"].tolist()))
                    assert all(p in listed for p in PLANTED_PAIRS), (divisor, sorted(listed))


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(tests)r)
from conftest import load_pkg
from test_grm_cpu import edge_rows, pack_bed, random_codes
P = load_pkg()
vp = load_pkg("variants_pca")
rng = np.random.default_rng(96)
n, v = 130, 300
codes = edge_rows(random_codes(rng, v, n))
rows = pack_bed(codes)
with P.PcoaEngine(n, grm=True) as eng:
    for a, b in ((0, 50), (50, 97), (97, 300)):
        eng.accumulate_plink_bed(np.ascontiguousarray(rows[a:b]))
    info = eng.grm_info()
    assert info[2] == -(-v // 96) * 96 * grm_row_bytes, info   # segments of 96 rows
    for divisor in ("used", "pairwise"):
        k = eng.grm_dense(divisor)
        cnt = eng.grm_pairs_block(0, n, 0, n)
        for cutoff in (-0.02, 0.0, 0.05):
            want = vp.grm_pairs_rule(k, cutoff, cnt if divisor == "pairwise" else info[1])
            assert want.size > 0
            for band in (0, 64, 128):
                got, found = eng.grm_pairs(cutoff, divisor, band_rows=band)
                assert found == want.size and got.tobytes() == want.tobytes(), (divisor, cutoff, band)
print("SEGMENTS-OK")
"""


def test_pairs_across_segment_boundaries():
    """V = 300 at N = 130 in four segments of 96 rows, fed in ragged calls (the knob is read once per process)."""
    env = dict(os.environ)
    env["PCOA_GRM_SEGMENT_ROWS"] = "96"
    code = (CHILD % {"tests": os.path.join(ROOT, "tests")}).replace("grm_row_bytes", "48")   # 130 samples: 3 x 64 slots, 16 a word
    res = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, timeout=300)
    assert res.returncode == 0 and "SEGMENTS-OK" in res.stdout, res.stdout[-3000:]


# ---- 3. capacity and state --------------------------------------------------------------------------------------------------
def test_capacity_returns_a_prefix_and_the_full_count(P, vp, rounded):
    codes = rounded["edge"]
    v, n = codes.shape
    lib = P._lib.load()
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, codes)
        full, found = eng.grm_pairs(0.0, "pairwise", band_rows=64)
        assert found == full.size and found > 100
        for cap in (0, 1, found - 1):
            buf = np.zeros(found + 3, dtype=P.PcoaEngine.GRM_PAIR_DTYPE)
            buf["i"], buf["j"], buf["k"], buf["n"] = -7, -8, -9.5, -10
            got = ctypes.c_int64(-1)
            rc = lib.pcoa_grm_pairs(eng._ctx, 0.0, 1, 64, ctypes.c_void_p(buf.ctypes.data) if cap else None, cap, ctypes.byref(got), None)
            assert rc == 0 and got.value == found, cap
            assert same_bits(buf[:cap], full[:cap]), cap
            tail = buf[cap:]
            assert np.all(tail["i"] == -7) and np.all(tail["j"] == -8) and np.all(tail["k"] == -9.5) and np.all(tail["n"] == -10), cap
        pairs, nf = eng.grm_pairs(0.0, "pairwise", capacity=0)
        assert pairs.size == 0 and nf == found


def test_the_screen_follows_the_state_of_the_ctx_and_leaves_it_alone(P, vp, rounded):
    codes = rounded["bn"]
    v, n = codes.shape

    def check(e, what):
        info = e.grm_info()
        for divisor in DIVISORS:
            k = e.grm_dense(divisor)
            cnt = e.grm_pairs_block(0, e.n, 0, e.n)
            cutoff = gap_cutoff(upper(k), 0.05)
            want = want_pairs(vp, k, cutoff, cnt, info[1], divisor)
            got, found, diag = e.grm_pairs(cutoff, divisor, band_rows=128, diag=True)
            assert want.size > 0 and found == want.size and same_bits(got, want), (what, divisor)
            assert same_bits(diag, np.ascontiguousarray(np.diagonal(k))), (what, divisor)

    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, codes)
        c0 = eng.compute(2)
        check(eng, "plain")
        c1 = eng.compute(2)
        assert same_bits(c1[0], c0[0]) and same_bits(c1[1], c0[1]) and c1[2] == c0[2]
        keep = np.setdiff1d(np.arange(n), [7, 50, 201, 259, 64])
        with eng.grm_subset(keep) as sub:
            check(sub, "subset")
        eng.grm_set_min_maf(0.2)
        assert 0 < eng.grm_info()[1] < v
        check(eng, "min_maf")
        eng.grm_set_min_maf(0.0)
        cand, kept = eng.grm_ld_prune(20, 0.1)
        assert 0 < kept < cand
        check(eng, "ld")
        eng.grm_ld_clear()
        c2 = eng.compute(2)
        assert same_bits(c2[0], c0[0]) and same_bits(c2[1], c0[1])


# ---- 4. refusals and statistics ---------------------------------------------------------------------------------------------
def test_refusals_and_statistics(P, rounded):
    L = P._lib
    lib = L.load()
    codes = rounded["edge"]
    v, n = codes.shape
    vpt = ctypes.c_void_p
    buf = np.zeros(16, dtype=P.PcoaEngine.GRM_PAIR_DTYPE)

    def raw(ctx, cutoff=0.05, div=0, band=0, out=True, cap=16, found=True):
        got = ctypes.c_int64(0)
        return lib.pcoa_grm_pairs(ctx, cutoff, div, band, vpt(buf.ctypes.data) if out else None, cap,
                                  ctypes.byref(got) if found else None, None)

    assert raw(None) == L.PCOA_ERR_INVALID_ARG and b"pcoa_grm_pairs" in lib.pcoa_last_error(None)
    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(n) as full, P.PcoaEngine(n, operator=True) as op, \
            P.PcoaEngine(n, grm_study=True) as study:
        fill(eng, codes)
        fill(study, codes)
        c0 = eng.compute(2)
        eng.reset_timings()
        for kw in (dict(found=False), dict(cutoff=float("nan")), dict(cutoff=float("inf")), dict(cutoff=-float("inf")), dict(div=2),
                   dict(div=-1), dict(band=-64), dict(band=32), dict(band=100), dict(cap=-1), dict(out=False)):
            assert raw(eng._ctx, **kw) == L.PCOA_ERR_INVALID_ARG, kw
            assert b"pcoa_grm_pairs" in lib.pcoa_last_error(eng._ctx) and len(lib.pcoa_last_error(eng._ctx)) > 30
        for other, word in ((full, "full engine"), (op, "operator")):
            with pytest.raises(P.PcoaError) as ei:
                other.grm_pairs(0.05)
            assert ei.value.code == L.PCOA_ERR_STATE and word in str(ei.value)
        with pytest.raises(P.PcoaError) as ei:
            study.grm_pairs(0.05)
        assert ei.value.code == L.PCOA_ERR_STATE and "no weights of its own" in str(ei.value)
        with pytest.raises(ValueError):
            eng.grm_pairs(0.05, "mean")
        st = eng.grm_pairs_stats()
        assert st["grm_pairs_calls"] == 0 and st["grm_pairs_bands"] == 0 and st["grm_pairs_bytes"] == 0
        # the ctx is usable after every refusal; the statistics advance: 130 rows in bands of 64 are 3 bands of 192, 128 and 64 columns
        _, found = eng.grm_pairs(0.0, "used", band_rows=64)
        st = eng.grm_pairs_stats()
        assert found > 0 and st["grm_pairs_calls"] == 1 and st["grm_pairs_bands"] == 3
        assert st["grm_pairs_flops"] == 2.0 * v * (64 * 192 + 64 * 128 + 2 * 64)
        assert st["grm_pairs_bytes"] >= 8 * (64 * 130 + 64 * 66 + 2 * 2) and st["grm_pairs_seconds"] >= st["grm_pairs_screen_seconds"] > 0
        eng.grm_pairs(0.0, "pairwise")
        st2 = eng.grm_pairs_stats()
        assert st2["grm_pairs_calls"] == 2 and st2["grm_pairs_bands"] == 4 and st2["grm_pairs_flops"] == st["grm_pairs_flops"] + 4.0 * v * 130 * 192
        c1 = eng.compute(2)
        assert same_bits(c1[0], c0[0]) and same_bits(c1[1], c0[1]) and c1[2] == c0[2]
        # M' = 0, as pcoa_grm_block reports it
        eng.reset()
        eng.accumulate_plink_bed(pack_bed(np.full((5, n), 3, np.uint8)))
        with pytest.raises(P.PcoaError) as ei:
            eng.grm_pairs(0.05)
        assert ei.value.code == L.PCOA_ERR_STATE and "none of the 5 variants" in str(ei.value)
        eng.reset()
        fill(eng, codes)
        assert eng.grm_pairs(0.0, "used", band_rows=64)[1] == found


# ---- 5. hosts ---------------------------------------------------------------------------------------------------------------
def test_both_hosts_screen_remove_and_project_alike(tmp_path, vp):
    from test_grm_cpu import _run_driver, _run_python
    g = load_golden("tile260")
    n = write_golden_plink(g, str(tmp_path / "tile260"))
    path = str(tmp_path / "tile260") + ".bed"
    raw = np.fromfile(path, dtype=np.uint8)[3:].reshape(-1, (n + 3) // 4)
    codes = ((raw[:, :, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(raw.shape[0], -1)[:, :n]
    m = spec_grm_weights(spec_grm_counts(codes, False))[3]
    names = ["S%04d" % i for i in range(n)]
    iu = np.triu_indices(n, 1)
    for divisor in ("pairwise",):      # (the divisor whose n column differs from pair to pair; a host run takes over a second)
        k_np, cnt = vp.grm_dense_rule(codes, False, 0.0, divisor)
        cutoff = gap_cutoff(k_np[iu], float(np.quantile(k_np[iu], 0.999)))        # some thirty pairs of 33,670
        assert np.all(np.abs(k_np[iu] - cutoff) > entry_bound(codes, cnt, divisor)[iu])
        want = want_pairs(vp, k_np, cutoff, cnt, m, divisor)
        gone = vp.related_removal(want, n)
        assert 0 < want.size < 200 and 0 < gone.size < n - 32
        outs = {}
        for tag, run in (("cpp", _run_driver), ("py", _run_python)):
            rel = str(tmp_path / ("%s_%s.tsv" % (tag, divisor)))
            res = run(["--input-path", path, "--grm", "--grm-cutoff", repr(cutoff), "--grm-related-output-path", rel, "--grm-cutoff-remove",
                       "--grm-project-removed", "--grm-cutoff-divisor", divisor])
            assert res.returncode == 0, res.stderr[-2000:]
            line = [ln for ln in res.stderr.splitlines() if ln.startswith("GRM relatedness:")]
            outs[tag] = (open(rel, "rb").read(), line, res.stdout)
        assert outs["cpp"][0] == outs["py"][0]                                    # the pair files, byte for byte
        assert outs["cpp"][1] == outs["py"][1] == ["GRM relatedness: %d pair(s) with K >= %s (divisor %s), removed %d sample(s)"
                                                   % (want.size, vp.java_double_to_string(cutoff), divisor, gone.size)]
        assert outs["cpp"][2] == outs["py"][2]                                    # the coordinates
        lines = outs["cpp"][0].decode().splitlines()
        assert lines[0] == "name_i\tname_j\tk\tn"
        assert [tuple(ln.split("\t")[:2]) for ln in lines[1:]] == [(names[p["i"]], names[p["j"]]) for p in want]
        assert [int(ln.split("\t")[3]) for ln in lines[1:]] == want["n"].tolist()
        got_k = np.array([float(ln.split("\t")[2]) for ln in lines[1:]])
        assert np.all(np.abs(got_k - want["k"]) <= entry_bound(codes, cnt, divisor)[want["i"], want["j"]])
        # every sample gets a row: the kept ones, then the removed ones placed on their axes
        rows = [ln.split("\t")[0] for ln in outs["cpp"][2].splitlines() if ln.startswith("S")]
        stay = np.setdiff1d(np.arange(n), gone)
        assert rows == [names[i] for i in stay] + [names[i] for i in gone]

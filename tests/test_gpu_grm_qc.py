"""GPU tests of the variant and sample QC of a GRM engine (pcoa_grm_set_variant_filters, pcoa_grm_hwe, pcoa_grm_sample_counts,
--grm-geno / --grm-hwe / --grm-mind).  The sample counts are compared EXACTLY with tests/grm_qc_cohort.py; the
Hardy-Weinberg p-values are held to the exact rational value within relative (4 N + 32) 2^-53 (the roundings of the recurrence,
the two sums and the quotient); used_v, M' and everything behind them are compared exactly, on cohorts where no exact p-value
lies within that bound of the threshold.  tests/test_grm_qc_cpu.py shows that the cohorts tell the right rule from two wrong ones."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import grm_qc_cohort as Q
from conftest import ROOT, align_sign, load_pkg
from test_grm_cpu import balding_nichols, edge_rows, exact_cohort, pack_bed, random_codes, spec_grm_counts

pytestmark = pytest.mark.gpu

RANGE_ROWS = 512   # kGrmRangeRows: rows whose partial counts one lane accumulates before it writes
SAMPLE_AXIS = [32, 33, 47, 48, 49, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097]
ROW_COUNTS = [1, 2, 3, 4, 7, 8, 15, 16, 17, 255, 256, 257, RANGE_ROWS - 1, RANGE_ROWS, RANGE_ROWS + 1]


@pytest.fixture(scope="module")
def P():
    return load_pkg()


def test_the_range_constant_is_the_kernels():
    import re
    src = open(os.path.join(ROOT, "spark-examples_amd", "csrc", "pcoa_internal.h")).read()
    assert int(re.search(r"constexpr int32_t kGrmRangeRows = (\d+);", src).group(1)) == RANGE_ROWS


def fill(eng, codes, ref_is_a1=False, cuts=None):
    """rows with garbage in the padding slots and three extra row bytes"""
    rows = pack_bed(codes, 3, np.random.default_rng(9))
    edges = [0] + sorted(cuts or []) + [rows.shape[0]]
    for a, b in zip(edges[:-1], edges[1:]):
        eng.accumulate_plink_bed(np.ascontiguousarray(rows[a:b]), ref_is_a1=ref_is_a1)
    eng.sync()


def cohort(n, v, seed=None):
    return edge_rows(random_codes(np.random.default_rng(1000 + n + v if seed is None else seed), v, n))


def check_hwe(eng, codes, ref_is_a1):
    """every row's p-value against the exact one; the cohort must have no near tie (a condition on the input)"""
    n = codes.shape[1]
    counts = spec_grm_counts(codes, ref_is_a1)
    for c in counts:
        assert Q.near_ties(int(c[0]), int(c[1]), int(c[2])) == [], c
    want = Q.hwe_of_counts(counts)
    got = eng.grm_hwe()
    assert got.shape == (codes.shape[0],)
    for r, (g, w) in enumerate(zip(got, want)):
        assert Q.hwe_within(g, w, n), (r, counts[r].tolist(), float(g), float(w))
    return got


# ---- sample counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SAMPLE_AXIS)
def test_sample_counts_at_the_sample_axis_edges(P, n):
    """ALL and USED under a min MAF, both reference alleles, garbage in the padding slots; at N <= 257 the p-values too"""
    codes = cohort(n, 70)
    for ref_is_a1 in (False, True):
        with P.PcoaEngine(n, grm=True) as eng:
            fill(eng, codes, ref_is_a1)
            assert np.array_equal(eng.grm_sample_counts(), Q.spec_sample_counts(codes, ref_is_a1))
            eng.grm_set_min_maf(0.1)
            used = Q.spec_used(spec_grm_counts(codes, ref_is_a1), n, 0.1)
            assert 0 < used.sum() < codes.shape[0] and eng.grm_info()[1] == used.sum()
            assert np.array_equal(eng.grm_sample_counts(used=True), Q.spec_sample_counts(codes, ref_is_a1, used))
            if n <= 257:
                check_hwe(eng, codes, ref_is_a1)


@pytest.mark.parametrize("v", ROW_COUNTS)
def test_sample_counts_where_a_counter_widens_and_at_one_range(P, v):
    n = 65
    codes = cohort(n, v)
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, codes)
        assert np.array_equal(eng.grm_sample_counts(), Q.spec_sample_counts(codes, False))
        used = Q.spec_used(spec_grm_counts(codes, False), n)
        assert np.array_equal(eng.grm_sample_counts(used=True), Q.spec_sample_counts(codes, False, used))
        check_hwe(eng, codes, False)
        st = eng.grm_qc_stats()
        assert st["grm_qc_sample_counts_calls"] == 2 and st["grm_qc_hwe_calls"] == 1 and st["grm_qc_sample_counts_seconds"] > 0


@pytest.mark.parametrize("ref_is_a1", [False, True])
def test_sample_counts_with_every_slice_saturated(P, ref_is_a1):
    """two whole ranges and six rows: the last 300 rows are all 11 (words of all ones in the .bed rows) but for the first three
    samples: sample 0 is missing at every row, sample 1 het at every row, sample 2 homozygous A2 at every row"""
    n, v = 70, 2 * RANGE_ROWS + 6
    codes = random_codes(np.random.default_rng(3), v, n)
    codes[-300:] = 3
    codes[:, 0] = 1
    codes[:, 1] = 2
    codes[:, 2] = 3
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, codes, ref_is_a1)
        got = eng.grm_sample_counts()
        assert np.array_equal(got, Q.spec_sample_counts(codes, ref_is_a1))
        assert got[0].tolist() == [0, 0, 0] and got[1].tolist() == [v, v, 0]
        assert got[3].tolist()[2] >= (300 if ref_is_a1 else 0)
        assert got[2].tolist() == [v, 0, v if ref_is_a1 else 0]
        check_hwe(eng, codes, ref_is_a1)


def test_an_empty_store_gives_zeros(P):
    with P.PcoaEngine(40, grm=True) as eng:
        assert not eng.grm_sample_counts().any() and not eng.grm_sample_counts(used=True).any()
        assert eng.grm_hwe().shape == (0,)
        fill(eng, cohort(40, 20))
        eng.reset()
        assert not eng.grm_sample_counts().any()


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(tests)r)
import grm_qc_cohort as Q
from conftest import load_pkg
from test_grm_cpu import edge_rows, pack_bed, random_codes, spec_grm_counts
P = load_pkg()
n, v = 130, 1500
codes = edge_rows(random_codes(np.random.default_rng(11), v, n))
rows = pack_bed(codes)
with P.PcoaEngine(n, grm=True) as eng:
    for a, b in ((0, 50), (50, 699), (699, 1401), (1401, v)):
        eng.accumulate_plink_bed(np.ascontiguousarray(rows[a:b]))
    assert eng.grm_info()[0] == v
    eng.grm_set_min_maf(0.05)
    eng.grm_set_variant_filters(0.08, 0.01)
    counts = spec_grm_counts(codes, False)
    used = Q.spec_used(counts, n, 0.05, 0.08, 0.01)
    assert eng.grm_info()[1] == used.sum() and 0 < used.sum() < v
    assert np.array_equal(eng.grm_sample_counts(), Q.spec_sample_counts(codes, False))
    assert np.array_equal(eng.grm_sample_counts(used=True), Q.spec_sample_counts(codes, False, used))
    got = eng.grm_hwe()
    for r, (g, w) in enumerate(zip(got, Q.hwe_of_counts(counts))):
        assert Q.near_ties(*[int(x) for x in counts[r]]) == [] and Q.hwe_within(g, w, n), (r, counts[r].tolist(), float(g), float(w))
print("SEGMENTS-OK")
"""


def test_sample_counts_across_a_segment_cut_inside_a_range():
    """segments of 700 rows: the first range of a segment is whole, the second ends at the cut (the knob is read once per process)"""
    env = dict(os.environ)
    env["PCOA_GRM_SEGMENT_ROWS"] = "700"
    res = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests")}], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0 and "SEGMENTS-OK" in res.stdout, res.stdout[-3000:]


def test_a_study_ctx_counts_all_rows_and_has_no_used_rows(P):
    L = load_pkg("_lib")
    n = 7
    codes = cohort(n, 40)
    with P.PcoaEngine(n, grm_study=True) as eng:
        fill(eng, codes)
        assert np.array_equal(eng.grm_sample_counts(), Q.spec_sample_counts(codes, False))
        with pytest.raises(P.PcoaError) as ei:
            eng.grm_sample_counts(used=True)
        assert ei.value.code == L.PCOA_ERR_STATE and "study" in str(ei.value)
        check_hwe(eng, codes, False)
        assert np.array_equal(eng.grm_sample_counts(), Q.spec_sample_counts(codes, False))


# ---- the exact test -------------------------------------------------------------------------------------------------------------
def test_hwe_of_planted_rows_at_4096_samples(P):
    n = 4096
    codes = np.concatenate([Q.planted_hwe_rows(n, 5), random_codes(np.random.default_rng(6), 12, n, missing=0.02)])
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, codes)
        got = check_hwe(eng, codes, False)
    want = Q.hwe_of_counts(spec_grm_counts(codes, False))
    assert want[1] < Fraction(1, 2 ** 900) and got[1] <= 2.0 ** -800       # no het at frequency 1 / 2
    assert want[0] < Fraction(1, 2 ** 900)                                 # all het
    assert min(want[2], want[3]) > Fraction(1, 1000) and got[4] == 1.0     # in equilibrium; a singleton has one term


@pytest.mark.parametrize("n", [33, 257])
def test_hwe_of_planted_rows_at_small_n(P, n):
    codes = Q.planted_hwe_rows(n, n)
    with P.PcoaEngine(n, grm_study=True) as eng:
        fill(eng, codes)
        check_hwe(eng, codes, False)


# ---- the filters ----------------------------------------------------------------------------------------------------------------
N_F, V_F, MAF_F, GENO_F, HWE_F = 96, 120, 0.05, 0.125, 1e-3


@pytest.fixture(scope="module")
def filtered():
    codes = Q.filter_cohort(N_F, V_F, 21)
    codes.setflags(write=False)
    counts = spec_grm_counts(codes, False)
    ps = Q.hwe_of_counts(counts)
    thr = Fraction(HWE_F)
    for p in ps:   # no exact p within the kernel's bound of the threshold
        assert abs(p - thr) > 2 * Q.hwe_bound(N_F) * max(p, thr)
    return codes, counts, ps, Q.spec_used(counts, N_F, MAF_F, GENO_F, HWE_F)


def test_used_counts_weights_and_stats_equal_the_spec(P, filtered):
    codes, counts, ps, used = filtered
    exactly = [r for r in range(V_F) if N_F - counts[r, 0] == N_F // 8]
    assert len(exactly) >= 3 and all(used[r] for r in exactly)             # a missing share equal to max_missing is kept
    assert (~Q.spec_used(counts, N_F, 0.0, GENO_F, 0.0)).sum() > (~Q.spec_used(counts, N_F)).sum()
    with P.PcoaEngine(N_F, grm=True) as eng:
        fill(eng, codes)
        assert eng.grm_variant_filters() == (1.0, 0.0)
        eng.grm_set_min_maf(MAF_F)
        eng.grm_set_variant_filters(GENO_F, HWE_F)
        assert eng.grm_variant_filters() == (GENO_F, HWE_F)
        assert eng.grm_info()[:2] == (V_F, int(used.sum()))
        assert np.array_equal(eng.grm_counts(), counts)
        comps, lam, nz = eng.compute(2)
        w = eng.grm_weights(comps, lam, scaled=True)
        assert np.all(w[~used] == 0.0) and np.all(np.any(w[used] != 0.0, axis=1))
        assert nz == int(((codes[used] != 1).sum(axis=0) > 0).sum())
        st = eng.grm_qc_stats()
        assert (st["grm_qc_fail_maf"], st["grm_qc_fail_missing"], st["grm_qc_fail_hwe"]) == Q.spec_fails(counts, N_F, MAF_F, GENO_F, HWE_F)
        assert st["grm_qc_fail_missing"] > 0 and st["grm_qc_fail_hwe"] >= 6
        # one filter at a time
        eng.grm_set_variant_filters(GENO_F, 0.0)
        assert eng.grm_info()[1] == Q.spec_used(counts, N_F, MAF_F, GENO_F, 0.0).sum()
        eng.grm_set_variant_filters(1.0, HWE_F)
        assert eng.grm_info()[1] == Q.spec_used(counts, N_F, MAF_F, 1.0, HWE_F).sum()
        eng.grm_set_variant_filters(0.0, 0.0)
        assert eng.grm_info()[1] == Q.spec_used(counts, N_F, MAF_F, 0.0, 0.0).sum()


def products(eng, x):
    import torch
    y = eng.grm_matvec_device(torch.from_numpy(x).cuda()).cpu().numpy()
    return y, eng.grm_block(0, eng.n, 0, eng.n)


def test_the_defaults_leave_every_result_bit_identical(P, filtered):
    codes = filtered[0]
    x = np.random.default_rng(1).standard_normal(N_F)
    with P.PcoaEngine(N_F, grm=True) as a, P.PcoaEngine(N_F, grm=True) as b:
        fill(a, codes)
        fill(b, codes)
        b.grm_set_variant_filters(GENO_F, HWE_F)
        assert b.grm_info()[1] < a.grm_info()[1]
        b.grm_set_variant_filters(1.0, 0.0)
        ya, ka = products(a, x)
        yb, kb = products(b, x)
        assert np.array_equal(ya, yb) and np.array_equal(ka, kb)
        ca, cb = a.compute(2), b.compute(2)
        assert np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1]) and ca[2] == cb[2]


def test_filters_equal_an_engine_fed_only_the_passing_rows(P, filtered):
    """K x on the planted cohort: an unused row adds 0.0 to every accumulator and the rows fit one range either way, so the order
    of the non-zero additions is the same.  grm_block adds four rows per step, so its comparison runs on a cohort where every
    partial sum is an integer (mu = 1, d = 2) and any order gives the same bits; the filters remove rows of it too."""
    codes, counts, ps, used = filtered
    x = np.random.default_rng(2).standard_normal(N_F)
    with P.PcoaEngine(N_F, grm=True) as a, P.PcoaEngine(N_F, grm=True) as b:
        fill(a, codes)
        a.grm_set_min_maf(MAF_F)
        a.grm_set_variant_filters(GENO_F, HWE_F)
        fill(b, codes[used])
        b.grm_set_min_maf(MAF_F)
        assert a.grm_info()[1] == b.grm_info()[1] == used.sum()
        assert np.array_equal(products(a, x)[0], products(b, x)[0])
    ex = exact_cohort(np.random.default_rng(4), N_F, 200, 9)
    cx = spec_grm_counts(ex, False)
    thr = Fraction(1, 100)
    for p in Q.hwe_of_counts(cx):
        assert abs(p - thr) > 2 * Q.hwe_bound(N_F) * max(p, thr)
    ux = Q.spec_used(cx, N_F, 0.0, 0.06, 0.01)
    assert 20 < ux.sum() < Q.spec_used(cx, N_F).sum() - 20
    xi = np.random.default_rng(5).integers(-8, 9, size=N_F).astype(np.float64)
    with P.PcoaEngine(N_F, grm=True) as a, P.PcoaEngine(N_F, grm=True) as b:
        fill(a, ex)
        a.grm_set_variant_filters(0.06, 0.01)
        fill(b, ex[ux])
        assert a.grm_info()[1] == b.grm_info()[1] == ux.sum()
        ya, ka = products(a, xi)
        yb, kb = products(b, xi)
        assert np.array_equal(ya, yb) and np.array_equal(ka, kb) and np.abs(ka).max() > 0


def test_other_values_drop_an_ld_mask_the_same_keep_it_and_reset_keeps_the_filters(P, filtered):
    L = load_pkg("_lib")
    codes, counts, ps, used = filtered
    with P.PcoaEngine(N_F, grm=True) as eng:
        fill(eng, codes)
        eng.grm_set_min_maf(MAF_F)
        eng.grm_set_variant_filters(GENO_F, HWE_F)
        cand, kept = eng.grm_ld_prune(20, 0.2)
        assert cand == used.sum() and 0 < kept <= cand                   # the prune judges its candidates under the filters
        mask = eng.grm_ld_mask()
        assert not np.any(mask & ~used)
        # USED counts the rows under min MAF, the filters and the mask
        assert np.array_equal(eng.grm_sample_counts(used=True), Q.spec_sample_counts(codes, False, Q.spec_used(counts, N_F, MAF_F, GENO_F, HWE_F, mask)))
        assert eng.grm_info()[1] == kept
        eng.grm_set_variant_filters(GENO_F, HWE_F)                        # the same values
        assert np.array_equal(eng.grm_ld_mask(), mask) and eng.grm_info()[1] == kept
        eng.grm_set_variant_filters(GENO_F, 0.0)                          # another value
        with pytest.raises(P.PcoaError) as ei:
            eng.grm_ld_mask()
        assert ei.value.code == L.PCOA_ERR_STATE
        assert eng.grm_info()[1] == Q.spec_used(counts, N_F, MAF_F, GENO_F, 0.0).sum()
        eng.grm_set_variant_filters(GENO_F, HWE_F)
        eng.reset()
        assert eng.grm_variant_filters() == (GENO_F, HWE_F) and eng.grm_info()[:2] == (0, 0)
        fill(eng, codes)
        assert eng.grm_info()[1] == used.sum()


def test_a_subset_inherits_the_filters_and_derives_from_its_own_columns(P, filtered):
    codes, counts, ps, used = filtered
    keep = np.sort(np.random.default_rng(8).choice(N_F, size=64, replace=False)).astype(np.int32)
    sub_codes = np.ascontiguousarray(codes[:, keep])
    sub_counts = spec_grm_counts(sub_codes, False)
    thr = Fraction(HWE_F)
    for p in Q.hwe_of_counts(sub_counts):
        assert abs(p - thr) > 2 * Q.hwe_bound(64) * max(p, thr)
    want = Q.spec_used(sub_counts, 64, MAF_F, GENO_F, HWE_F)
    x = np.random.default_rng(3).standard_normal(64)
    with P.PcoaEngine(N_F, grm=True) as eng, P.PcoaEngine(64, grm=True) as fresh:
        fill(eng, codes)
        eng.grm_set_min_maf(MAF_F)
        eng.grm_set_variant_filters(GENO_F, HWE_F)
        with eng.grm_subset(keep) as sub:
            assert sub.grm_variant_filters() == (GENO_F, HWE_F)
            fresh.accumulate_plink_bed(pack_bed(np.array([3, 1, 2, 0], dtype=np.uint8)[sub_codes]), ref_is_a1=True)
            fresh.grm_set_min_maf(MAF_F)
            fresh.grm_set_variant_filters(GENO_F, HWE_F)
            assert sub.grm_info()[1] == fresh.grm_info()[1] == want.sum()
            assert np.array_equal(sub.grm_counts(), sub_counts)
            assert np.array_equal(sub.grm_hwe(), fresh.grm_hwe())
            assert np.array_equal(sub.grm_sample_counts(used=True), Q.spec_sample_counts(sub_codes, False, want))
            ys, ks = products(sub, x)
            yf, kf = products(fresh, x)
            assert np.array_equal(ys, yf) and np.array_equal(ks, kf)


def test_every_error_leaves_the_ctx_usable(P, filtered):
    L = load_pkg("_lib")
    codes, counts, ps, used = filtered
    with P.PcoaEngine(N_F, grm=True) as eng:
        fill(eng, codes)
        eng.grm_set_min_maf(MAF_F)
        eng.grm_set_variant_filters(GENO_F, HWE_F)
        for bad in ((float("nan"), 0.0), (0.5, float("nan")), (-0.01, 0.0), (1.01, 0.0), (0.5, -1e-9), (0.5, 1.0)):
            with pytest.raises(P.PcoaError) as ei:
                eng.grm_set_variant_filters(*bad)
            assert ei.value.code == L.PCOA_ERR_INVALID_ARG, bad
        for args in ((-1, 2), (0, V_F + 1), (V_F, 1)):
            with pytest.raises(P.PcoaError) as ei:
                eng.grm_hwe(*args)
            assert ei.value.code == L.PCOA_ERR_INVALID_ARG
        assert eng._lib.pcoa_grm_sample_counts(eng._ctx, 2, None) == L.PCOA_ERR_INVALID_ARG
        assert eng._lib.pcoa_grm_sample_counts(eng._ctx, 0, None) == L.PCOA_ERR_INVALID_ARG
        assert eng.grm_variant_filters() == (GENO_F, HWE_F) and eng.grm_info()[1] == used.sum()
    with P.PcoaEngine(40, grm_study=True) as study, P.PcoaEngine(40) as full, P.PcoaEngine(40, operator=True) as op:
        for other, word in ((study, "study"), (full, "full engine"), (op, "operator")):
            with pytest.raises(P.PcoaError) as ei:
                other.grm_set_variant_filters(0.5, 0.0)
            assert ei.value.code == L.PCOA_ERR_STATE and word in str(ei.value)
            with pytest.raises(P.PcoaError) as ei:
                other.grm_variant_filters()
            assert ei.value.code == L.PCOA_ERR_STATE and word in str(ei.value)
        for other, word in ((full, "full engine"), (op, "operator")):
            for call in (other.grm_hwe, other.grm_sample_counts):
                with pytest.raises(P.PcoaError) as ei:
                    call()
                assert ei.value.code == L.PCOA_ERR_STATE and word in str(ei.value)
        fill(study, cohort(40, 30))
        assert study.grm_info()[0] == 30


# ---- the hosts ------------------------------------------------------------------------------------------------------------------
def write_plink(prefix, codes):
    v, n = codes.shape
    with open(prefix + ".fam", "w") as f:
        for i in range(n):
            f.write("FAM%d S%04d 0 0 0 -9\n" % (i, i))
    with open(prefix + ".bim", "w") as f:
        for k in range(v):
            f.write("17\trs%d\t0\t%d\tC\tA\n" % (k, 41196312 + 7 * k))
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6c, 0x1b, 0x01]))
        f.write(pack_bed(codes).tobytes())


def coords_of(stdout):
    rows = [line.split("\t") for line in stdout.splitlines() if line.count("\t") == 3]
    return np.array([[float(r[-2]), float(r[-1])] for r in rows])


def planted_fileset():
    """N = 96, V = 400 with population structure: 8 variants with 29 of 96 calls missing, 6 without a heterozygote at a third of
    the alleles, 5 samples with 160 of 400 calls missing"""
    n, v = 96, 400
    rng = np.random.default_rng(96)
    codes = balding_nichols(rng, n, v, missing=0.01)
    low_geno = list(range(20, 20 + 8 * 9, 9))
    off_hwe = list(range(200, 200 + 6 * 11, 11))
    low_mind = [3, 17, 40, 66, 90]
    for r in off_hwe:
        row = np.full(n, 3, np.uint8)
        row[: n // 3] = 0
        codes[r] = rng.permutation(row)
    for r in low_geno:
        row = codes[r]
        row[row == 1] = 3
        row[rng.choice(n, size=29, replace=False)] = 1
    for s in low_mind:
        col = codes[:, s]
        col[col == 1] = 3
        col[rng.choice(v, size=160, replace=False)] = 1
    return codes, low_geno, off_hwe, low_mind


def test_both_hosts_filter_write_the_qc_files_and_decompose_the_passing_cohort(tmp_path):
    from test_grm_cpu import _run_driver, _run_python
    geno, hwe, mind = 0.2, 1e-6, 0.3
    codes, low_geno, off_hwe, low_mind = planted_fileset()
    v, n = codes.shape
    counts = spec_grm_counts(codes, False)
    sc = Q.spec_sample_counts(codes, False)
    stay = ~((v - sc[:, 0]).astype(np.float64) / float(v) > mind)
    assert np.flatnonzero(~stay).tolist() == low_mind
    sub = np.ascontiguousarray(codes[:, stay])
    sub_counts = spec_grm_counts(sub, False)
    thr = Fraction(hwe)
    for c, m in ((counts, n), (sub_counts, int(stay.sum()))):
        for p in Q.hwe_of_counts(c):
            assert abs(p - thr) > 2 * Q.hwe_bound(m) * max(p, thr)
    fails = Q.spec_fails(counts, n, 0.0, geno, hwe)
    assert fails[1:] == (len(low_geno), len(off_hwe))
    used_full = Q.spec_used(counts, n, 0.0, geno, hwe)
    used_sub = Q.spec_used(sub_counts, int(stay.sum()), 0.0, geno, hwe)
    assert np.flatnonzero(~used_sub).tolist() == sorted(low_geno + off_hwe)      # the reduced cohort loses the same variants
    write_plink(str(tmp_path / "all"), codes)
    write_plink(str(tmp_path / "passing"), sub[used_sub])
    line = "GRM QC: removed %d variant(s) by MAF, %d by missing rate, %d by HWE; %d sample(s) by call rate" % (fails + (len(low_mind),))
    files = {}
    for tag, run in (("cpp", _run_driver), ("py", _run_python)):
        vq, sq = str(tmp_path / ("variants_%s.tsv" % tag)), str(tmp_path / ("samples_%s.tsv" % tag))
        res = run(["--input-path", str(tmp_path / "all.bed"), "--all-references", "--grm", "--grm-geno", str(geno), "--grm-hwe", str(hwe),
                   "--grm-mind", str(mind), "--grm-variant-qc-output-path", vq, "--grm-sample-qc-output-path", sq, "--grm-project-removed"])
        assert res.returncode == 0, res.stderr[-2000:]
        assert line in res.stderr, res.stderr[-2000:]
        files[tag] = (open(vq, "rb").read(), open(sq, "rb").read())
        plain = run(["--input-path", str(tmp_path / "passing.bed"), "--all-references", "--grm"])
        assert plain.returncode == 0, plain.stderr[-2000:]
        a, b = coords_of(res.stdout), coords_of(plain.stdout)
        assert a.shape == (int(stay.sum()), 2) and b.shape == a.shape      # the samples --grm-mind removed are not placed
        assert np.abs(align_sign(a, b) - b).max() < 1e-6
    assert files["cpp"] == files["py"]
    vrows = [ln.split("\t") for ln in files["py"][0].decode().splitlines()]
    assert len(vrows) == v and [int(r[0]) for r in vrows] == list(range(v)) and vrows[7][1:4] == ["17", str(41196312 + 49), "rs7"]
    assert np.array_equal(np.array([[int(x) for x in r[4:7]] for r in vrows]), counts)
    assert [int(r[9]) for r in vrows] == used_full.astype(int).tolist()
    assert all(r[7] == "%.6f" % (float(n - c[0]) / float(n)) for r, c in zip(vrows, counts))
    for r, want in zip(vrows, Q.hwe_of_counts(counts)):
        assert Q.hwe_within(float(r[8]), want, n) and r[8] == "%.17g" % float(r[8])
    srows = [ln.split("\t") for ln in files["py"][1].decode().splitlines()]
    assert len(srows) == n and np.array_equal(np.array([[int(x) for x in r[1:4]] for r in srows]), sc)
    assert [int(r[6]) for r in srows] == stay.astype(int).tolist()
    assert all(r[4] == "%.6f" % (float(c[0]) / float(v)) and r[5] == "%.6f" % (float(c[1]) / float(c[0])) for r, c in zip(srows, sc))

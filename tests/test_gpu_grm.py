"""GPU tests of the standardised-genotype operator (pcoa_create_grm): the per-variant counts are the spec's integers in every
input form, the product K x equals the spec bit for bit on cohorts where the spec is order-free and stays inside its summation
bound elsewhere, results are bit-identical run to run and across call sizes, computePca over the operator gives numpy's
eigenpairs of the dense K, and what a GRM ctx cannot serve says so and leaves it usable.  The spec is the numpy statement in
test_grm_cpu.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, align_sign, load_golden, load_pkg, write_golden_plink
from test_grm_cpu import balding_nichols, dense_k, edge_rows, exact_cohort, pack_bed, random_codes, spec_grm_bound, \
    spec_grm_called_samples, spec_grm_counts, spec_grm_matvec, spec_grm_weights

pytestmark = pytest.mark.gpu

SEGMENT_KNOB = "PCOA_GRM_SEGMENT_ROWS"


@pytest.fixture(scope="module")
def P():
    return load_pkg()


def store_bytes(n, variants, segment_rows=None):
    """What pcoa_grm_info reports (include/pcoa.h): whole segments of ~256 MiB -- whole multiples of 2,048 rows where a segment
    holds that many -- of rows at a pitch of ceil(N / 4) bytes rounded up to 16."""
    pitch = ((n + 3) // 4 + 15) // 16 * 16
    rows = max(1, (256 << 20) // pitch)
    if rows >= 2048:
        rows -= rows % 2048
    if segment_rows:
        rows = segment_rows
    return -(-variants // rows) * rows * pitch


def feed(eng, codes, ref_is_a1, form, rng):
    """The input forms: 0 host rows in one call, 1 host rows with garbage in the padding slots and in extra row bytes, handed over
    in ragged calls with an empty call in between, 2 device rows with garbage in one call, 3 page-locked host rows queued
    (PCOA_BED_HOST_ASYNC) in ragged calls."""
    import torch
    v = codes.shape[0]
    rows = pack_bed(codes, 3 if form == 1 else 1 if form == 2 else 0, rng if form in (1, 2) else None)
    cuts = [0, v]
    if form in (1, 3) and v > 1:
        cuts = sorted(set([0, v] + [int(c) for c in rng.integers(1, v, size=min(3, v - 1))]))
    keep = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        part = np.ascontiguousarray(rows[a:b])
        if form == 2:
            eng.accumulate_plink_bed(torch.from_numpy(part).cuda(), ref_is_a1=ref_is_a1)
        elif form == 3:
            keep.append(torch.from_numpy(part).pin_memory())
            eng.accumulate_plink_bed(keep[-1], ref_is_a1=ref_is_a1, asynchronous=True)
        else:
            eng.accumulate_plink_bed(part, ref_is_a1=ref_is_a1)
            eng.accumulate_plink_bed(part[:0], ref_is_a1=ref_is_a1)     # an empty call adds nothing
    eng.sync()


def product(eng, x):
    import torch
    return eng.grm_matvec_device(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()).cpu().numpy()


# ---- counts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,v", [(33, 70), (260, 1000), (1025, 300)])
@pytest.mark.parametrize("ref_is_a1", [False, True])
def test_counts_are_the_specs_integers_in_every_input_form(P, n, v, ref_is_a1):
    rng = np.random.default_rng(10 * n + ref_is_a1)
    codes = edge_rows(random_codes(rng, v, n))
    want = spec_grm_counts(codes, ref_is_a1)
    with P.PcoaEngine(n, grm=True) as eng:
        assert eng.grm_info() == (0, 0, 0) and eng.operator_info() is None
        for form in range(4):
            eng.reset()
            feed(eng, codes, ref_is_a1, form, rng)
            assert np.array_equal(eng.grm_counts(), want), form
            assert eng.grm_info() == (v, spec_grm_weights(want)[3], store_bytes(n, v)), form
            assert np.array_equal(eng.grm_counts(5, 7), want[5:12])


# ---- exact products ---------------------------------------------------------------------------------------------------------
# N: the issue's list, then the sample-direction constants of grm_bits.hip minus one, exact, plus one: a lane's 16 samples (at
# three lanes: a ctx needs N >= 32), a wave's chunk of 64 word columns (1,024 samples, in the list already) and a pass-1
# workgroup's group of 256 (4,096 samples); N = 70,000 once, beyond any 16-bit index.
# V = (used, unused): the used rows a power of two, the unused ones filling up to a butterfly block of 32 rows, the 512 rows of a
# pass-1 workgroup and of a pass-2 range, and the 2,048 rows segments are whole multiples of, each minus one, exact, plus one.
SHAPES_N = [32, 33, 47, 48, 49, 63, 64, 65, 1023, 1024, 1025, 2504, 4095, 4096, 4097, 4100, 70000]
SHAPES_V = [(1, 2), (64, 1)]
EXTRA_V = [(1, 0), (1, 30), (32, 0), (32, 1), (64, 447), (512, 0), (512, 1), (1024, 1023), (2048, 0), (2048, 1)]


@pytest.mark.parametrize("n", SHAPES_N)
def test_products_equal_the_spec_bit_for_bit_on_exact_cohorts(P, n):
    """x drawn from the integers in [-8, 8], mu_v = 1, d_v = 2, M' a power of two: every partial sum of either pass is an integer
    far below 2^53, so y must equal the spec whatever the summation order."""
    rng = np.random.default_rng(2000 + n)
    shapes = [(32, 1)] if n > 4100 else SHAPES_V + (EXTRA_V if n == 2504 else [])
    with P.PcoaEngine(n, grm=True) as eng:
        for k, (vu, vx) in enumerate(shapes):
            ref_is_a1 = bool(k & 1)
            codes = exact_cohort(rng, n, vu, vx, ref_is_a1)
            for _ in range(20):                          # (one used row can be orthogonal to a random x)
                x = rng.integers(-8, 9, size=n).astype(np.float64)
                want = spec_grm_matvec(codes, ref_is_a1, x)
                if want.any():
                    break
            assert want.any()
            for form in ((k % 4, (k + 1) % 4) if n == 2504 else range(4) if n <= 65 else (k % 4,)):
                eng.reset()
                feed(eng, codes, ref_is_a1, form, rng)
                assert eng.grm_info() == (vu + vx, vu, store_bytes(n, vu + vx)), (vu, vx, form)
                assert np.array_equal(product(eng, x), want), (vu, vx, form)
        eng.reset()
        assert eng.grm_info()[:2] == (0, 0) and not product(eng, x).any()


def test_a_call_larger_than_a_staging_slot(P):
    """V = 2^17 used rows + 1 unused row at N = 2,504, host rows in one call: more rows than a slot of the host staging ring."""
    n, vu = 2504, 1 << 17
    rng = np.random.default_rng(17)
    base = exact_cohort(rng, n, 1 << 10, 0)
    codes = np.concatenate([base[rng.integers(0, base.shape[0], size=vu)], np.full((1, n), 3, np.uint8)])
    x = rng.integers(-8, 9, size=n).astype(np.float64)
    with P.PcoaEngine(n, grm=True) as eng:
        eng.accumulate_plink_bed(pack_bed(codes))
        assert eng.grm_info() == (vu + 1, vu, store_bytes(n, vu + 1))
        assert np.array_equal(product(eng, x), spec_grm_matvec(codes, False, x, block=8192))


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(tests)r)
from conftest import load_pkg
from test_grm_cpu import exact_cohort, pack_bed, spec_grm_counts, spec_grm_matvec, spec_grm_called_samples
import torch
P = load_pkg()
rng = np.random.default_rng(96)
n, vu, vx = 130, 512, 488
codes = exact_cohort(rng, n, vu, vx)
rows = pack_bed(codes)
x = rng.integers(-8, 9, size=n).astype(np.float64)
with P.PcoaEngine(n, grm=True) as eng:
    for r0 in range(0, vu + vx, 250):
        eng.accumulate_plink_bed(rows[r0:r0 + 250])
    assert eng.grm_info() == (1000, vu, 11 * 96 * 48), eng.grm_info()      # 11 segments of 96 rows of 48 bytes
    assert np.array_equal(eng.grm_counts(), spec_grm_counts(codes, False))
    y = eng.grm_matvec_device(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.array_equal(y, spec_grm_matvec(codes, False, x))
    comps, lam, nz = eng.compute(2)
    assert nz == spec_grm_called_samples(codes, False)
    eng.reset()
    assert eng.grm_info() == (0, 0, 96 * 48)
print("SEGMENTS-OK")
"""


def test_products_across_segment_boundaries():
    """1,000 rows in calls of 250 at N = 130 with segments of 96 rows (the knob is read once per process: a fresh child)."""
    env = dict(os.environ)
    env[SEGMENT_KNOB] = "96"
    res = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests")}], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0 and "SEGMENTS-OK" in res.stdout, res.stdout[-3000:]


# ---- rounded products -------------------------------------------------------------------------------------------------------
ROUNDED = [(33, 70), (260, 1000), (2504, 3000)]


@pytest.fixture(scope="module")
def rounded_cohorts():
    out = {}
    for n, v in ROUNDED:
        rng = np.random.default_rng(n + v)
        out[(n, v)] = (random_codes(rng, v, n, missing=0.05), rng.standard_normal(n))
    return out


@pytest.mark.parametrize("n,v", ROUNDED)
def test_real_products_stay_inside_the_summation_bound(P, rounded_cohorts, n, v):
    """|y - spec| <= (N + V + 16) 2^-52 (W^T diag(d) (W |x|)) / M': the worst-case summation bound over the terms actually added.
    Between two numpy summation orders the ratio to this bound is <= 7e-5 at these shapes."""
    codes, x0 = rounded_cohorts[(n, v)]
    swapped = np.array([3, 1, 2, 0], dtype=np.uint8)[codes]
    worst = 0.0
    with P.PcoaEngine(n, grm=True) as eng:
        eng.accumulate_plink_bed(pack_bed(codes))
        for scale in (1e-3, 1.0, 1e3):
            x = x0 * scale
            want, bound = spec_grm_matvec(codes, False, x), spec_grm_bound(codes, False, x)
            y = product(eng, x)
            worst = max(worst, float(np.max(np.abs(y - want) / bound)))
            assert np.all(np.abs(y - want) <= bound), scale
        # the rows with 00 and 11 exchanged under the same flag: every A(v, i) changes sign, K does not
        eng.reset()
        eng.accumulate_plink_bed(pack_bed(swapped))
        y = product(eng, x0)
        want, bound = spec_grm_matvec(codes, False, x0), spec_grm_bound(codes, False, x0)
        worst = max(worst, float(np.max(np.abs(y - want) / bound)))
        print("N = %d, V = %d: largest |y - spec| / bound = %.3g" % (n, v, worst))
        assert np.all(np.abs(y - want) <= bound)


def test_min_maf(P, rounded_cohorts):
    codes, x = rounded_cohorts[(260, 1000)]
    with P.PcoaEngine(260, grm=True) as eng:
        eng.accumulate_plink_bed(pack_bed(codes))
        y0 = product(eng, x)
        m0 = eng.grm_info()[1]
        eng.grm_set_min_maf(0.05)
        want, bound = spec_grm_matvec(codes, False, x, 0.05), spec_grm_bound(codes, False, x, 0.05)
        m = spec_grm_weights(spec_grm_counts(codes, False), 0.05)[3]
        assert eng.grm_info()[1] == m and 0 < m < m0
        assert np.all(np.abs(product(eng, x) - want) <= bound)
        with pytest.raises(P.PcoaError) as ei:
            eng.grm_set_min_maf(0.5)
        assert ei.value.code == P._lib.PCOA_ERR_INVALID_ARG
        eng.reset()                                       # min_maf survives a reset
        eng.accumulate_plink_bed(pack_bed(codes))
        assert eng.grm_info()[1] == m
        eng.grm_set_min_maf(0.0)
        assert eng.grm_info()[1] == m0 and product(eng, x).tobytes() == y0.tobytes()


# ---- determinism ------------------------------------------------------------------------------------------------------------
def test_results_are_bit_identical_run_to_run_and_across_call_sizes(P):
    n, v = 2504, 5000
    rng = np.random.default_rng(55)
    codes = random_codes(rng, v, n)
    rows = pack_bed(codes)
    x = rng.standard_normal(n)
    results = []
    for cuts in ([0, v], [0, v], [0, 1, 33, 2049, 2050, 4999, v]):
        with P.PcoaEngine(n, grm=True) as eng:
            for a, b in zip(cuts[:-1], cuts[1:]):
                eng.accumulate_plink_bed(rows[a:b])
            y = product(eng, x)
            comps, lam, nz = eng.compute(2)
            results.append((y.tobytes(), product(eng, x).tobytes(), comps.tobytes(), lam.tobytes(), nz))
    assert results[0][0] == results[0][1]
    assert results[0] == results[1] == results[2]


# ---- spectrum ---------------------------------------------------------------------------------------------------------------
def check_spectrum(P, n, codes, eig=None, k=2):
    kd = dense_k(codes, False)
    lam_all, vec_all = np.linalg.eigh(kd)
    lam_f, comps_f = lam_all[::-1][:k], vec_all[:, ::-1][:, :k]
    assert (lam_all[-1] - lam_all[-2]) / lam_all[-1] >= 0.01 and (lam_all[-2] - lam_all[-3]) / lam_all[-1] >= 0.01
    with P.PcoaEngine(n, grm=True, eig=eig) as eng:
        eng.accumulate_plink_bed(pack_bed(codes))
        comps, lam, nz = eng.compute(k)
        t = eng.timings()
    assert nz == spec_grm_called_samples(codes, False)
    assert t["operator_products"] > 0 and t["operator_store_bytes"] > 0 and t["eig_method"] == 1
    assert np.max(np.abs(lam - lam_f) / np.abs(lam_f)) < 1e-6
    assert np.abs(align_sign(comps, comps_f) - comps_f).max() < 1e-6
    for c in range(k):
        assert abs(np.linalg.norm(comps[:, c]) - 1) < 1e-12
        assert np.linalg.norm(kd @ comps[:, c] - lam[c] * comps[:, c]) <= 1e-9 * abs(lam[c])
    for c in range(k):
        for d in range(c):
            assert abs(comps[:, c] @ comps[:, d]) < 1e-10


@pytest.mark.parametrize("n,eig", [(130, None), (260, None), (2504, None), (260, "band")])
def test_balding_nichols_cohorts_give_numpys_eigenpairs_of_k(P, n, eig):
    rng = np.random.default_rng(300 + n)
    codes = balding_nichols(rng, n, 3000)
    codes[:, 7] = 1                              # a sample that is never called: a zero row of K
    check_spectrum(P, n, codes, eig=eig)


def test_a_cohort_of_70000_samples(P):
    """N = 70,000 x V = 256: 4.5 MB of store, and no N x N matrix (39 GB as fp64): the residuals of compute(2) through the spec's
    blocked product, and the HBM the engine takes beside the store."""
    import torch
    n, v = 70000, 256
    rng = np.random.default_rng(7)
    codes = balding_nichols(rng, n, v, fst=0.2)
    free0 = torch.cuda.mem_get_info()[0]
    with P.PcoaEngine(n, grm=True) as eng:
        eng.accumulate_plink_bed(pack_bed(codes))
        comps, lam, nz = eng.compute(2)
        free1 = torch.cuda.mem_get_info()[0]
        info = eng.grm_info()
    assert info == (v, spec_grm_weights(spec_grm_counts(codes, False))[3], store_bytes(n, v)) and nz == spec_grm_called_samples(codes, False)
    assert free0 - free1 - info[2] < 1 << 30
    for c in range(2):
        u = comps[:, c]
        assert abs(np.linalg.norm(u) - 1) < 1e-12
        assert np.linalg.norm(spec_grm_matvec(codes, False, u) - lam[c] * u) <= 1e-9 * abs(lam[c])
    assert lam[0] > lam[1] > 0 and abs(comps[:, 0] @ comps[:, 1]) < 1e-10


# ---- state ------------------------------------------------------------------------------------------------------------------
def test_what_a_grm_ctx_cannot_serve_says_so_and_leaves_it_usable(P):
    import torch
    L = P._lib
    n, v = 130, 300
    rng = np.random.default_rng(9)
    codes = random_codes(rng, v, n)
    rows = pack_bed(codes)
    x = rng.standard_normal(n)
    bits = np.zeros((4, (n + 31) // 32), dtype=np.uint32)
    with pytest.raises(P.PcoaError) as ei:
        P.PcoaEngine(16, grm=True)
    assert ei.value.code == L.PCOA_ERR_INVALID_ARG and "32" in str(ei.value)
    with pytest.raises(P.PcoaError) as ei:
        P.PcoaEngine(n, grm=True, eig="householder")
    assert ei.value.code == L.PCOA_ERR_INVALID_ARG
    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(n) as full, P.PcoaEngine(n, operator=True) as op:
        eng.accumulate_plink_bed(rows)
        y0 = product(eng, x)
        c0 = eng.compute(2)
        xd = torch.from_numpy(x).cuda()
        refused = [
            lambda: eng.accumulate_bits(bits),
            lambda: eng.accumulate_dense(np.zeros((2, n), np.float32)),
            lambda: eng.accumulate_dense_u8(np.zeros((2, n), np.uint8)),
            lambda: eng.accumulate_callsets([[1, 2]]),
            lambda: eng.accumulate_plink_bed_calls(rows, full),
            lambda: eng.gram(),
            lambda: eng.gram_block(0, 0, 2, 2),
            lambda: eng.load_gram(np.zeros((n, n), np.int64)),
            lambda: eng.center(),
            lambda: eng.operator_row_sums(),
            lambda: eng.operator_matvec_device(xd, False),
            lambda: eng.project(full, c0[0], c0[1]),
            lambda: eng.loadings(c0[0], c0[1]),
            lambda: eng.ld_pruner(10, 0.2),
            lambda: eng._check(eng._lib.pcoa_set_similarity(eng._ctx, 1)),
            lambda: eng._check(eng._lib.pcoa_set_call_companion(eng._ctx, full._ctx, 0)),
            lambda: eng._check(eng._lib.pcoa_create_subset(ctypes.byref(ctypes.c_void_p()), eng._ctx, None, 0)),
            lambda: eng._check(eng._lib.pcoa_similar_pairs(eng._ctx, 0.5, None, 0, ctypes.byref(ctypes.c_int64()), None)),
            lambda: eng._check(eng._lib.pcoa_gram_reduce_from(eng._ctx, full._ctx)),
            lambda: eng._check(eng._lib.pcoa_strip_col_sums(eng._ctx, None)),
        ]
        messages = set()
        for k, call in enumerate(refused):
            with pytest.raises(P.PcoaError) as ei:
                call()
            assert ei.value.code == L.PCOA_ERR_STATE and len(str(ei.value)) > 30, (k, str(ei.value))
            messages.add(str(ei.value))
        assert len(messages) >= len(refused) - 2          # their own messages
        assert eng.operator_info() is None
        assert product(eng, x).tobytes() == y0.tobytes()
        c1 = eng.compute(2)
        assert c1[0].tobytes() == c0[0].tobytes() and c1[1].tobytes() == c0[1].tobytes() and c1[2] == c0[2]
        # a ctx that is not a GRM ctx
        for other in (full, op):
            assert other.grm_info() is None
            for call in (lambda: other.grm_set_min_maf(0.1), lambda: other.grm_counts(0, 0), lambda: other.grm_matvec_device(xd)):
                with pytest.raises(P.PcoaError) as ei:
                    call()
                assert ei.value.code == L.PCOA_ERR_STATE
        # M' = 0: the product is zero, compute says so
        eng.reset()
        eng.accumulate_plink_bed(pack_bed(np.full((5, n), 3, np.uint8)))
        assert eng.grm_info()[:2] == (5, 0) and not product(eng, x).any()
        with pytest.raises(P.PcoaError) as ei:
            eng.compute(2)
        assert ei.value.code == L.PCOA_ERR_STATE
        eng.reset()
        eng.accumulate_plink_bed(rows)
        assert product(eng, x).tobytes() == y0.tobytes()


# ---- hosts ------------------------------------------------------------------------------------------------------------------
def host_rows(res):
    assert res.returncode == 0, res.stderr[-2000:]
    rows = [ln.split("\t") for ln in res.stdout.splitlines() if ln.count("\t") == 3]
    return [(r[0], r[1]) for r in rows], np.array([[float(r[2]), float(r[3])] for r in rows])


def test_both_hosts_give_numpys_coordinates_of_k(tmp_path):
    """The tile260 golden as a PLINK fileset through --grm on both hosts: the sample names and order of the stored form, the
    coordinates within 1e-6 of numpy's eigenvectors of the spec's K (sign-aligned), the milestone lines, and the stderr line that
    says what was decomposed -- present with --grm, absent without."""
    from test_grm_cpu import _run_driver, _run_python
    g = load_golden("tile260")
    n = write_golden_plink(g, str(tmp_path / "tile260"))
    path = str(tmp_path / "tile260") + ".bed"
    raw = np.fromfile(path, dtype=np.uint8)[3:].reshape(-1, (n + 3) // 4)
    codes = ((raw[:, :, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(raw.shape[0], -1)[:, :n]
    counts = spec_grm_counts(codes, False)                    # (A2 is the reference allele: the hosts' default)
    lam, vec = np.linalg.eigh(dense_k(codes, False))
    want = vec[:, ::-1][:, :2]
    assert (lam[-1] - lam[-2]) / lam[-1] >= 0.01 and (lam[-2] - lam[-3]) / lam[-1] >= 0.01
    for run in (_run_driver, _run_python):
        stored = run(["--input-path", path])
        grm = run(["--input-path", path, "--grm"])
        ids_s, _ = host_rows(stored)
        ids_g, xy = host_rows(grm)
        assert len(ids_s) == n and ids_g == ids_s
        assert np.abs(align_sign(xy, want) - want).max() < 1e-6
        line = "Standardised genotypes: %d of %d variants used (min MAF 0), store %d bytes" % (
            spec_grm_weights(counts)[3], codes.shape[0], store_bytes(n, codes.shape[0]))
        assert line in grm.stderr and "Standardised genotypes" not in stored.stderr, grm.stderr[-1500:]
        for milestone in ("Matrix size: %d." % n, "Non zero rows in matrix: %d / %d." % (spec_grm_called_samples(codes, False), n)):
            assert milestone in grm.stdout
        maf = run(["--input-path", path, "--grm", "--grm-min-maf", "0.05"])
        assert "Standardised genotypes: %d of %d variants used (min MAF 0.05)" % (spec_grm_weights(counts, 0.05)[3], codes.shape[0]) in maf.stderr

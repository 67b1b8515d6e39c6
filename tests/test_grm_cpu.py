"""CPU tests of the standardised-genotype operator (pcoa_create_grm, --grm): the numpy statement of what it computes (imported
by tests/test_gpu_grm.py), the generator of cohorts on which that statement is exact in fp64, the ABI surface, the command-line
surface of both hosts, which must refuse what a GRM engine cannot serve before any engine exists, and the compile-time resource
check of its kernels."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, load_pkg, write_golden_plink, write_golden_vcf


# ---- the spec (include/pcoa.h, "standardised-genotype PCA") -----------------------------------------------------------------
# A cohort is `codes`, [V][N] uint8 PLINK codes (0 = 00 homozygous A1, 1 = 01 missing, 2 = 10 heterozygous, 3 = 11 homozygous A2)
# and ref_is_a1.
def pack_bed(codes, extra_bytes=0, rng=None):
    """[V][N] codes -> [V][ceil(N / 4) + extra_bytes] uint8 .bed rows (sample s in bits 2 (s % 4) of byte s / 4).  rng: the
    padding slots of the last byte and the extra bytes are random."""
    v, n = codes.shape
    nb = (n + 3) // 4
    full = np.zeros((v, nb * 4), dtype=np.uint8)
    if rng is not None:
        full[:] = rng.integers(0, 4, size=full.shape, dtype=np.uint8)
    full[:, :n] = codes
    q = full.reshape(v, nb, 4)
    rows = q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)
    if extra_bytes:
        tail = (rng.integers(0, 256, size=(v, extra_bytes), dtype=np.uint8) if rng is not None
                else np.zeros((v, extra_bytes), dtype=np.uint8))
        rows = np.concatenate([rows, tail], axis=1)
    return np.ascontiguousarray(rows, dtype=np.uint8)


def dosage(codes, ref_is_a1):
    """(g, c) as uint8: copies of the non-reference allele (0 where not called) and the called indicator."""
    codes = np.asarray(codes)
    hom = 3 if ref_is_a1 else 0
    c = (codes != 1).astype(np.uint8)
    g = (codes == 2).astype(np.uint8) + 2 * (codes == hom).astype(np.uint8)
    return g, c


def spec_grm_counts(codes, ref_is_a1):
    """[V][3] int32: n_v called, h_v heterozygous, o_v homozygous non-reference."""
    codes = np.asarray(codes)
    hom = 3 if ref_is_a1 else 0
    return np.stack([(codes != 1).sum(axis=1), (codes == 2).sum(axis=1), (codes == hom).sum(axis=1)], axis=1).astype(np.int32)


def spec_grm_weights(counts, min_maf=0.0):
    """(mu, d, used, M') from the counts, in the header's expressions."""
    n = counts[:, 0].astype(np.int64)
    a = counts[:, 1].astype(np.int64) + 2 * counts[:, 2].astype(np.int64)
    nf, af = n.astype(np.float64), a.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = np.where(n > 0, af / nf, 0.0)
        used = (n > 0) & (a > 0) & (a < 2 * n) & (np.minimum(a, 2 * n - a).astype(np.float64) >= min_maf * (2.0 * nf))
        d = np.where(used, 1.0 / (mu * (1.0 - 0.5 * mu)), 0.0)
    return mu, d, used, int(used.sum())


def spec_grm_matvec(codes, ref_is_a1, x, min_maf=0.0, block=4096):
    """y = K x = A^T diag(d) A x / M' with A = g - mu c, in blocks of rows so that A is never held whole.  M' = 0: y = 0."""
    x = np.asarray(x, dtype=np.float64)
    mu, d, used, m = spec_grm_weights(spec_grm_counts(codes, ref_is_a1), min_maf)
    y = np.zeros(codes.shape[1], dtype=np.float64)
    if m == 0:
        return y
    for r0 in range(0, codes.shape[0], block):
        g, c = dosage(codes[r0:r0 + block], ref_is_a1)
        gf, cf = g.astype(np.float64), c.astype(np.float64)
        mb = mu[r0:r0 + block]
        t = d[r0:r0 + block] * (gf @ x - mb * (cf @ x))
        y += gf.T @ t - cf.T @ (mb * t)
    return y / m


def spec_grm_bound(codes, ref_is_a1, x, min_maf=0.0, block=4096):
    """The worst-case summation bound of one product, per sample: (N + V + 16) 2^-52 (W^T diag(d) (W |x|))_i / M' with
    W = g + mu c: the magnitudes of the terms actually added (a - mu b cancels, so the bound is stated over the uncentred ones);
    the 16 covers the roundings of mu, d and the combining operations."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    v, n = codes.shape
    mu, d, used, m = spec_grm_weights(spec_grm_counts(codes, ref_is_a1), min_maf)
    y = np.zeros(n, dtype=np.float64)
    if m == 0:
        return y
    for r0 in range(0, v, block):
        g, c = dosage(codes[r0:r0 + block], ref_is_a1)
        w = g.astype(np.float64) + mu[r0:r0 + block, None] * c.astype(np.float64)
        y += w.T @ (d[r0:r0 + block] * (w @ x))
    return (n + v + 16) * 2.0 ** -52 * y / m


def spec_grm_called_samples(codes, ref_is_a1, min_maf=0.0):
    """The samples called at one or more used variants (pcoa_compute's out_nonzero_rows on a GRM ctx)."""
    used = spec_grm_weights(spec_grm_counts(codes, ref_is_a1), min_maf)[2]
    return int(((np.asarray(codes)[used] != 1).sum(axis=0) > 0).sum())


def dense_k(codes, ref_is_a1, min_maf=0.0):
    g, c = dosage(codes, ref_is_a1)
    mu, d, used, m = spec_grm_weights(spec_grm_counts(codes, ref_is_a1), min_maf)
    a = g.astype(np.float64) - mu[:, None] * c.astype(np.float64)
    return (a.T * d) @ a / m


# ---- cohorts ----------------------------------------------------------------------------------------------------------------
def random_codes(rng, v, n, missing=0.05, lo=0.02, hi=0.98):
    """Hardy-Weinberg genotypes at allele frequencies U(lo, hi), missing at rate `missing`; as codes with A2 the reference."""
    p = rng.uniform(lo, hi, size=(v, 1))
    g = (rng.random((v, n)) < p).astype(np.uint8) + (rng.random((v, n)) < p).astype(np.uint8)
    codes = np.array([3, 2, 0], dtype=np.uint8)[g]
    codes[rng.random((v, n)) < missing] = 1
    return codes


def edge_rows(codes):
    """Fixed places of a random cohort get a monomorphic row of each kind, an all-missing row, an all-het row, and sample 1 is
    never called (shapes too small for a row keep what they have)."""
    v = codes.shape[0]
    for row, code in ((0, 0), (1, 3), (2, 1), (3, 2)):
        if row < v:
            codes[row] = code
    if v > 4:
        codes[4, ::2] = 1          # monomorphic among the called
        codes[4, 1::2] = 3
    codes[:, 1] = 1
    return codes


def exact_cohort(rng, n, v_used, v_unused=0, ref_is_a1=False):
    """A cohort on which the spec is independent of summation order: every used row has k homozygous non-reference, k
    homozygous reference and the rest heterozygous or missing samples, so a_v = n_v, mu_v = 1 and d_v = 2 exactly; the unused
    rows are monomorphic or all missing (d_v = 0).  With integer x and M' = v_used a power of two every partial sum of either
    pass is an integer far below 2^53.  Returns codes with the unused rows spread among the used ones."""
    hom, ref = (3, 0) if ref_is_a1 else (0, 3)
    v = v_used + v_unused
    codes = np.empty((v, n), dtype=np.uint8)
    unused = set(rng.choice(v, size=v_unused, replace=False).tolist()) if v_unused else set()
    for r in range(v):
        if r in unused:
            codes[r] = (ref, 1, hom)[r % 3]
            continue
        k = int(rng.integers(1, n // 2 + 1))              # (k = 0 would be a row of A that is all zero)
        row = np.where(rng.random(n - 2 * k) < 0.1, 1, 2).astype(np.uint8)
        row = np.concatenate([np.full(k, hom, np.uint8), np.full(k, ref, np.uint8), row])
        codes[r] = rng.permutation(row)
    return codes


def balding_nichols(rng, n, v, fst=0.1, missing=0.03, proportions=(1, 2, 3)):
    """Three populations in the given proportions; per variant an ancestral frequency U(0.1, 0.9) and per-population frequencies
    Beta(p (1 - F) / F, (1 - p) (1 - F) / F); Hardy-Weinberg genotypes; codes with A2 the reference."""
    parts = np.asarray(proportions, dtype=np.float64)
    edges = np.floor(np.cumsum(parts) / parts.sum() * n + 0.5).astype(int)
    pop = np.searchsorted(edges, np.arange(n), side="right")
    p = rng.uniform(0.1, 0.9, size=v)
    f = rng.beta(p[:, None] * (1 - fst) / fst, (1 - p[:, None]) * (1 - fst) / fst, size=(v, len(parts)))
    pf = f[:, pop]
    g = (rng.random((v, n)) < pf).astype(np.uint8) + (rng.random((v, n)) < pf).astype(np.uint8)
    codes = np.array([3, 2, 0], dtype=np.uint8)[g]
    codes[rng.random((v, n)) < missing] = 1
    return codes


# ---- the spec checks itself -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v,n,ref_is_a1,maf", [(70, 33, False, 0.0), (300, 130, True, 0.0), (300, 130, False, 0.05)])
def test_blocked_spec_equals_the_dense_matrix(v, n, ref_is_a1, maf):
    rng = np.random.default_rng(v + n)
    codes = edge_rows(random_codes(rng, v, n))
    x = rng.standard_normal(n)
    k = dense_k(codes, ref_is_a1, maf)
    assert np.allclose(k, k.T, rtol=0, atol=1e-12)
    y = spec_grm_matvec(codes, ref_is_a1, x, maf, block=37)
    assert np.all(np.abs(y - k @ x) <= spec_grm_bound(codes, ref_is_a1, x, maf))
    counts = spec_grm_counts(codes, ref_is_a1)
    mu, d, used, m = spec_grm_weights(counts, maf)
    # the monomorphic and the all-missing rows are unused; the all-het row has mu = 1 and is used
    assert used[:5].tolist() == [False, False, False, True, False] and mu[3] == 1.0 and d[3] == 2.0 and 0 < m < v
    assert counts[2].tolist() == [0, 0, 0] and counts[3].tolist() == [n - 1, n - 1, 0]
    # every row of A has mean 0 over its called samples: K 1 = 0 up to rounding, no double centring needed
    assert np.all(np.abs(k @ np.ones(n)) <= spec_grm_bound(codes, ref_is_a1, np.ones(n), maf))
    assert spec_grm_called_samples(codes, ref_is_a1, maf) == n - 1


def test_swapping_the_reference_allele_leaves_the_spec_unchanged():
    rng = np.random.default_rng(5)
    codes = edge_rows(random_codes(rng, 200, 67))
    swapped = np.array([3, 1, 2, 0], dtype=np.uint8)[codes]          # 00 <-> 11 in the rows
    x = rng.standard_normal(67)
    # the same rows read with the other allele as reference: g -> 2 c - g, mu -> 2 - mu, A -> -A, d unchanged
    y0, y1 = spec_grm_matvec(codes, False, x), spec_grm_matvec(codes, True, x)
    assert np.all(np.abs(y0 - y1) <= 2 * spec_grm_bound(codes, False, x))
    # the swapped rows with the swapped flag are the same cohort
    assert np.array_equal(spec_grm_matvec(swapped, True, x), y0)


@pytest.mark.parametrize("n,v_used,v_unused,ref_is_a1", [(33, 1, 2, False), (130, 64, 3, True), (1025, 512, 1, False)])
def test_exact_cohort_generator_gives_unit_means_and_an_order_free_spec(n, v_used, v_unused, ref_is_a1):
    rng = np.random.default_rng(n)
    codes = exact_cohort(rng, n, v_used, v_unused, ref_is_a1)
    mu, d, used, m = spec_grm_weights(spec_grm_counts(codes, ref_is_a1))
    assert m == v_used and np.all(mu[used] == 1.0) and np.all(d[used] == 2.0) and np.all(d[~used] == 0.0)
    x = rng.integers(-8, 9, size=n).astype(np.float64)
    want = spec_grm_matvec(codes, ref_is_a1, x)
    # three masked sums per pass, in blocks of 37 rows and another order of the samples: the same bits
    g, c = dosage(codes, ref_is_a1)
    hi, both, called = (g >= 1), (g == 2), (c == 1)
    perm = rng.permutation(n)
    y = np.zeros(n)
    for r0 in range(0, codes.shape[0], 37):
        sl = slice(r0, r0 + 37)
        a = (hi[sl][:, perm] * x[perm]).sum(axis=1) + (both[sl][:, perm] * x[perm]).sum(axis=1)
        b = (called[sl][:, perm] * x[perm]).sum(axis=1)
        t = d[sl] * (a - mu[sl] * b)
        y += (hi[sl] * t[:, None]).sum(axis=0) + (both[sl] * t[:, None]).sum(axis=0) + (called[sl] * (-(mu[sl] * t))[:, None]).sum(axis=0)
    assert np.array_equal(y / m, want)


def test_balding_nichols_cohort_has_the_gaps_the_spectrum_tests_need():
    rng = np.random.default_rng(130)
    codes = balding_nichols(rng, 130, 3000)
    lam = np.linalg.eigvalsh(dense_k(codes, False))[::-1]
    assert (lam[0] - lam[1]) / lam[0] >= 0.01 and (lam[1] - lam[2]) / lam[0] >= 0.01


# ---- the ABI surface --------------------------------------------------------------------------------------------------------
GRM_SYMBOLS = ["pcoa_create_grm", "pcoa_grm_info", "pcoa_grm_set_min_maf", "pcoa_grm_counts", "pcoa_grm_matvec_device"]


def test_grm_symbols_are_declared_bound_and_exported():
    lib = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "pcoa.h")).read()
    for sym in GRM_SYMBOLS:
        assert sym in lib.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % sym, header), sym
    minor = int(re.search(r"#define PCOA_VERSION_MINOR (\d+)", header).group(1))
    assert minor >= 10
    if os.path.exists(lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
        exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
        for sym in GRM_SYMBOLS:
            assert sym in exported, sym


# ---- the kernels: no scratch ------------------------------------------------------------------------------------------------
def test_grm_kernels_do_not_spill_to_scratch():
    """grm_bits.hip keeps 16 fp64 values per lane in registers in both passes (and 32 row partials in the first): an array that
    lands in scratch instead turns every add into a memory access.  hipcc reports it at compile time."""
    import shutil
    import tempfile
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                              "-I", csrc, "-c", os.path.join(csrc, "grm_bits.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True)
    assert res.returncode == 0, res.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", res.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stdout)]
    assert len(names) == len(scratch)
    for family in ("grm_append_kernel", "grm_counts_kernel", "grm_weights_kernel", "grm_ax_kernel", "grm_combine_t_kernel",
                   "grm_at_kernel", "grm_called_kernel", "grm_finish_kernel", "grm_called_finish_kernel"):
        assert any(family in nm for nm in names), "no %s in grm_bits.hip" % family
    for nm, sc in zip(names, scratch):
        assert sc == 0, "%s spills %d bytes/lane" % (nm, sc)


# ---- the hosts: --grm -------------------------------------------------------------------------------------------------------
def _exe():
    exe = os.path.join(ROOT, "spark-examples_amd", "variants_pca_driver")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "spark-examples_amd", "host")])
    return exe


def _run_driver(args):
    return subprocess.run([_exe()] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)


def _run_python(args):
    code = "import sys, importlib; sys.path.insert(0, %r); sys.exit(importlib.import_module('spark-examples_amd.variants_pca').main(%r))" % (ROOT, args)
    return subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                          timeout=300)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("grmcli")
    g = load_golden("kat5")
    write_golden_plink(g, str(d / "kat5"))
    write_golden_vcf(g, str(d / "kat5.vcf"))
    return {"bed": str(d / "kat5.bed"), "vcf": str(d / "kat5.vcf"), "dir": str(d)}


# (extra arguments, what the message must name beside --grm); @bed / @vcf / @out are replaced by paths
REFUSED = [
    (["--gpus", "2"], "gpus"),
    (["--layout", "strips"], "layout"),
    (["--gram", "implicit"], "gram"),
    (["--project-input-path", "@vcf"], "project-input-path"),
    (["--dump-similarity", "@out"], "dump-similarity"),
    (["--similarity-measure", "jaccard"], "similarity-measure"),
    (["--missing-calls", "pairwise"], "missing-calls"),
    (["--outlier-iterations", "1"], "outlier-iterations"),
    (["--related-min-jaccard", "0.5"], "related-min-jaccard"),
    (["--king-cutoff", "0.1"], "king-cutoff"),
    (["--ld-window", "50"], "ld-window"),
    (["--loadings-output-path", "@out"], "loadings-output-path"),
]


def _args(inputs, extra, source="bed"):
    subst = {"@bed": inputs["bed"], "@vcf": inputs["vcf"], "@out": os.path.join(inputs["dir"], "out.tsv")}
    return ["--input-path", inputs[source], "--grm"] + [subst.get(a, a) for a in extra]


@pytest.mark.parametrize("extra,what", REFUSED)
def test_driver_refuses_what_a_grm_engine_cannot_serve(inputs, extra, what):
    res = _run_driver(_args(inputs, extra))
    assert res.returncode != 0 and "--grm" in res.stderr and what in res.stderr, res.stderr
    assert "Matrix size" not in res.stdout and "pcoa_create" not in res.stderr       # no engine was attempted


@pytest.mark.parametrize("extra,what", REFUSED)
def test_python_host_refuses_what_a_grm_engine_cannot_serve(inputs, extra, what):
    res = _run_python(_args(inputs, extra))
    assert res.returncode != 0 and "--grm" in res.stderr and what in res.stderr, res.stderr
    assert "Matrix size" not in res.stdout and "pcoa error" not in res.stderr        # no engine was attempted


def test_both_hosts_refuse_an_input_that_is_not_a_plink_fileset(inputs):
    for run in (_run_driver, _run_python):
        res = run(_args(inputs, [], source="vcf"))
        assert res.returncode != 0 and "--grm" in res.stderr and ".bed" in res.stderr, res.stderr
        assert "Matrix size" not in res.stdout and "pcoa error" not in res.stderr and "pcoa_create" not in res.stderr


def test_grm_is_off_by_default_and_min_maf_needs_it():
    vp = load_pkg("variants_pca")
    assert vp.PcaConf([]).grm is False and vp.PcaConf(["--grm"]).grm is True
    assert vp.PcaConf(["--grm", "--grm-min-maf", "0.05"]).grm_min_maf == 0.05

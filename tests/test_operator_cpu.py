"""CPU tests of the implicit similarity operator (pcoa_create_operator, --gram implicit): the numpy statement of what the
operator computes (imported by tests/test_gpu_operator.py), the command-line surface of both hosts, which must refuse what
the operator cannot serve before any engine exists, and the compile-time resource check of the operator's kernels."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, int_gram, load_golden, load_oracle, load_pkg, write_golden_plink, write_golden_vcf


# ---- the spec: S v = X^T (X v), the row sums, the centred form --------------------------------------------------------------
def unpack_bits(bits, n):
    """[V][W] uint32 bitsets -> [V][n] uint8 (sample i = bit (i & 31) of word i >> 5, include/pcoa.h)."""
    b = np.ascontiguousarray(bits, dtype="<u4")
    return np.unpackbits(b.view(np.uint8).reshape(b.shape[0], -1), axis=1, bitorder="little")[:, :n]


def spec_matvec(x, v, block=4096):
    """S v without S: X^T (X v), X the [V][N] 0/1 matrix (any dtype), in blocks of rows so that no copy of X in float64 is
    ever whole.  For integer v every product and partial sum is an integer below 2^53: the result is then exact."""
    v = np.asarray(v, dtype=np.float64)
    y = np.zeros(x.shape[1], dtype=np.float64)
    for r0 in range(0, x.shape[0], block):
        xb = np.asarray(x[r0:r0 + block], dtype=np.float64)
        y += xb.T @ (xb @ v)
    return y


def spec_row_sums(x, block=4096):
    """rowSums of S (VariantsPca.scala:206) = X^T (X 1): per-variant carrier counts, then their sums per sample.  Integers
    below 2^53 throughout, so the float64 products are exact (asserted); int64."""
    y = np.zeros(x.shape[1], dtype=np.float64)
    for r0 in range(0, x.shape[0], block):
        xb = np.asarray(x[r0:r0 + block], dtype=np.float64)
        y += xb.T @ xb.sum(axis=1)
    out = y.astype(np.int64)
    assert float(x.shape[0]) * x.shape[1] ** 2 < 2.0 ** 53 and np.array_equal(out.astype(np.float64), y)
    return out


def spec_centring(row_sums):
    """(means, matrix mean) as computePca derives them from the row sums (VariantsPca.scala:206-215)."""
    n = float(len(row_sums))
    return np.asarray(row_sums, dtype=np.float64) / n, float(np.asarray(row_sums, dtype=np.int64).sum()) / n / n


def spec_centred_matvec(x, v):
    """B v with B(j, i) = ((S(j, i) - m_j) - m_i) + mm applied AROUND the product: S v - m (1^T v) - 1 (m^T v) + mm (1^T v) 1."""
    v = np.asarray(v, dtype=np.float64)
    m, mm = spec_centring(spec_row_sums(x))
    sv = v.sum()
    return ((spec_matvec(x, v) - m * sv) - m @ v) + mm * sv


def test_spec_is_the_similarity_matrix_of_the_reference():
    """The operator form against the stored form on a cohort small enough to form S: X^T (X v) is int_gram(X) @ v exactly for
    integer v, the row sums are S's, and the centred form is the oracle's centred matrix times v up to rounding."""
    oracle = load_oracle()
    ingest = load_pkg("ingest")
    rng = np.random.default_rng(7)
    for n, nv in ((5, 9), (33, 70), (130, 257), (300, 5000)):
        x = (rng.random((nv, n)) < 0.3).astype(np.float32)
        x[:, n // 2] = 0                                     # a sample nobody carries
        s = int_gram(x)
        v = rng.integers(-8, 9, size=n).astype(np.float64)
        assert np.array_equal(spec_matvec(x, v, block=64), s.astype(np.float64) @ v)
        assert np.array_equal(spec_row_sums(x), s.sum(axis=1))
        assert np.array_equal(unpack_bits(ingest.pack_bits(x), n), x.astype(np.uint8))
        b = oracle.center_matrix(s)[0]
        w = rng.standard_normal(n)
        m, mm = spec_centring(s.sum(axis=1))
        scale = np.abs(s) @ np.abs(w) + (2 * np.abs(m).max() + abs(mm)) * np.abs(w).sum()
        assert np.all(np.abs(spec_centred_matvec(x, w) - b @ w) <= (n + nv + 8) * 2.0 ** -52 * scale)


# ---- the kernels: no scratch ------------------------------------------------------------------------------------------------
def test_operator_kernels_do_not_spill_to_scratch():
    """operator_bits.hip keeps 32 fp64 values per lane in registers in both passes (and 32 row partials in the first): an
    array that lands in scratch instead turns every add into a memory access.  hipcc reports it at compile time."""
    import shutil
    import tempfile
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                              "-I", csrc, "-c", os.path.join(csrc, "operator_bits.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True)
    assert res.returncode == 0, res.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", res.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stdout)]
    assert len(names) == len(scratch)
    for family in ("operator_append_kernel", "operator_xv_kernel", "operator_xt_kernel", "operator_popcount_kernel",
                   "operator_dots_kernel", "operator_finish_kernel", "operator_combine_t_kernel", "operator_row_sums_finish_kernel"):
        assert any(family in nm for nm in names), "no %s in operator_bits.hip" % family
    assert sum("operator_xt_kernel" in nm for nm in names) == 2          # the fp64 pass and its int64 twin
    for nm, sc in zip(names, scratch):
        assert sc == 0, "%s spills %d bytes/lane" % (nm, sc)


# ---- the hosts: --gram stored | implicit ------------------------------------------------------------------------------------
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
    d = tmp_path_factory.mktemp("opcli")
    g = load_golden("kat5")
    write_golden_plink(g, str(d / "kat5"))
    write_golden_vcf(g, str(d / "kat5.vcf"))
    return {"bed": str(d / "kat5.bed"), "vcf": str(d / "kat5.vcf"), "dir": str(d)}


REFUSED_BY_BOTH = [
    (["--gpus", "2"], "gpus"),
    (["--layout", "strips"], "layout"),
    (["--carrier-format", "lists"], "carrier-format"),
]


@pytest.mark.parametrize("extra,what", REFUSED_BY_BOTH + [(["--project-input-path", "@bed"], "project-input-path")])
def test_driver_refuses_what_the_operator_cannot_serve(inputs, extra, what):
    extra = [inputs["bed"] if a == "@bed" else a for a in extra]
    res = _run_driver(["--input-path", inputs["bed"], "--gram", "implicit"] + extra)
    assert res.returncode != 0 and "--gram" in res.stderr and what in res.stderr, res.stderr
    assert "Matrix size" not in res.stdout and "pcoa_create" not in res.stderr       # no engine was attempted


# (the Python host has no --carrier-format: under --gram implicit its rows always travel as bitsets)
@pytest.mark.parametrize("extra,what", REFUSED_BY_BOTH[:2] + [(["--project-input-path", "@bed"], "project-input-path"),
                                                              (["--dump-similarity", "@dump"], "dump-similarity")])
def test_python_host_refuses_what_the_operator_cannot_serve(inputs, extra, what):
    extra = [inputs["bed"] if a == "@bed" else os.path.join(inputs["dir"], "s.npy") if a == "@dump" else a for a in extra]
    res = _run_python(["--input-path", inputs["bed"], "--gram", "implicit"] + extra)
    assert res.returncode != 0 and "--gram" in res.stderr and what in res.stderr, res.stderr
    assert "Matrix size" not in res.stdout and "pcoa error" not in res.stderr        # no engine was attempted


def test_both_hosts_name_the_two_choices_of_gram(inputs):
    for run in (_run_driver, _run_python):
        res = run(["--input-path", inputs["bed"], "--gram", "bogus"])
        assert res.returncode != 0 and "--gram" in res.stderr and "stored" in res.stderr and "implicit" in res.stderr, res.stderr
        assert "Matrix size" not in res.stdout


def test_gram_defaults_to_stored():
    vp = load_pkg("variants_pca")
    assert vp.PcaConf([]).gram == "stored" and vp.PcaConf(["--gram", "implicit"]).gram == "implicit"
    with pytest.raises(SystemExit):
        vp.PcaConf(["--gram", "auto"])


def test_python_host_packs_carrier_lists_into_bitsets_and_refuses_a_repeated_callset():
    """--gram implicit: RDD[Seq[Int]] rows in either form become the bitsets ingest.pack_bits builds; a list that names a
    callset twice cannot be a bitset and is refused with a message that names --gram (before any engine exists: the function
    needs no device)."""
    vp, ingest = load_pkg("variants_pca"), load_pkg("ingest")
    rng = np.random.default_rng(11)
    x = (rng.random((70, 67)) < 0.3).astype(np.float32)
    x[5] = 0
    lists = [list(np.nonzero(r)[0]) for r in x]
    offs = np.concatenate([[0], np.cumsum(x.sum(axis=1, dtype=np.int64))]).astype(np.int64)
    idx = np.nonzero(x)[1].astype(np.int32)
    for form in (lists, (idx, offs)):
        kind, bits = vp.calls_as_bits(form, 67)
        assert kind == "bits" and np.array_equal(bits, ingest.pack_bits(x))
    passthrough = ("bits", ingest.pack_bits(x))
    assert vp.calls_as_bits(passthrough, 67) is passthrough
    with pytest.raises(SystemExit) as ei:
        vp.calls_as_bits([[1, 2], [3, 66, 3]], 67)
    assert "--gram" in str(ei.value) and "twice" in str(ei.value)
    with pytest.raises(IndexError):
        vp.calls_as_bits([[67]], 67)

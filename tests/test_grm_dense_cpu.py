"""CPU tests of reading K out (pcoa_grm_block, --grm-output-path): the numpy statement variants_pca.grm_dense_rule against the
dense K of test_grm_cpu.py, the writer of the GCTA-layout files, the ABI surface, the command-line surface of both hosts, which
must refuse the new flags without --grm before any engine exists, and the compile-time resource check of grm_dense.hip."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, load_pkg
from test_grm_cpu import _args, _run_driver, _run_python, dense_k, dosage, edge_rows, exact_cohort, inputs, random_codes, \
    spec_grm_counts, spec_grm_weights  # noqa: F401  (inputs is a fixture)


@pytest.fixture(scope="module")
def vp():
    return load_pkg("variants_pca")


# ---- the rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v,n", [(70, 33), (300, 130)])
@pytest.mark.parametrize("ref_is_a1", [False, True])
@pytest.mark.parametrize("maf", [0.0, 0.05])
def test_the_rule_is_the_dense_k_and_an_integer_gram_of_the_called_masks(vp, v, n, ref_is_a1, maf):
    rng = np.random.default_rng(v + n)
    codes = edge_rows(random_codes(rng, v, n))
    k, cnt = vp.grm_dense_rule(codes, ref_is_a1, maf, "used")
    assert np.abs(k - dense_k(codes, ref_is_a1, maf)).max() <= 1e-12
    assert np.array_equal(k, k.T)
    used = spec_grm_weights(spec_grm_counts(codes, ref_is_a1), maf)[2]
    c = dosage(codes[used], ref_is_a1)[1].astype(np.int64)
    assert np.array_equal(cnt, c.T @ c) and cnt.dtype == np.int64
    kp, cnt_p = vp.grm_dense_rule(codes, ref_is_a1, maf, "pairwise")
    assert np.array_equal(cnt_p, cnt) and np.array_equal(kp, kp.T)
    # sample 1 is never called: a zero row, column and diagonal under both divisors
    for m in (k, kp):
        assert not m[1].any() and not m[:, 1].any()
    with pytest.raises(ValueError):
        vp.grm_dense_rule(codes, ref_is_a1, maf, "mean")
    with pytest.raises(ValueError):
        vp.grm_dense_rule(np.full((4, n), 3, np.uint8), ref_is_a1, maf)     # M' = 0


def test_pairwise_is_used_times_m_over_n_where_nothing_is_missing(vp):
    rng = np.random.default_rng(3)
    codes = random_codes(rng, 120, 40, missing=0.0)
    m = spec_grm_weights(spec_grm_counts(codes, False))[3]
    k, cnt = vp.grm_dense_rule(codes, False, 0.0, "used")
    kp, _ = vp.grm_dense_rule(codes, False, 0.0, "pairwise")
    assert np.all(cnt == m)
    assert np.allclose(kp, k * m / cnt, rtol=4 * 2.0 ** -52, atol=0)


@pytest.mark.parametrize("n,v_used,v_unused,ref_is_a1", [(33, 4, 3, False), (130, 64, 2, True)])
def test_on_an_exact_cohort_num_is_an_integer_and_the_order_of_the_variants_is_free(vp, n, v_used, v_unused, ref_is_a1):
    rng = np.random.default_rng(n)
    codes = exact_cohort(rng, n, v_used, v_unused, ref_is_a1)
    perm = rng.permutation(codes.shape[0])
    for divisor in ("used", "pairwise"):
        k, cnt = vp.grm_dense_rule(codes, ref_is_a1, 0.0, divisor)
        k2, cnt2 = vp.grm_dense_rule(codes[perm], ref_is_a1, 0.0, divisor)
        assert k.tobytes() == k2.tobytes() and np.array_equal(cnt, cnt2)
    num = vp.grm_dense_rule(codes, ref_is_a1, 0.0, "used")[0] * v_used
    assert np.array_equal(num, np.rint(num)) and np.abs(num).max() > 0


# ---- the writer -------------------------------------------------------------------------------------------------------------
def test_the_writer_against_a_hand_built_case(vp, tmp_path):
    k = np.array([[1.0, 0.0, 0.0], [0.25, 1.5, 0.0], [-0.125, 1.0 / 3.0, 2.0]])
    cnt = np.array([[7, 0, 0], [6, 7, 0], [5, 4, 6]], dtype=np.int32)
    ids = [("setA", "s0"), ("setA", "s1"), ("setB", "s2")]
    prefix = str(tmp_path / "out")
    # two bands: rows 0 .. 1 with columns 0 .. 1, row 2 with columns 0 .. 2
    nbytes = vp.write_grm_files(prefix, ids, [(0, k[0:2, 0:2], cnt[0:2, 0:2]), (2, k[2:3, 0:3], cnt[2:3, 0:3])])
    order = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]
    want_k = b"".join(np.float32(k[i, j]).tobytes() for i, j in order)
    want_n = b"".join(np.float32(cnt[i, j]).tobytes() for i, j in order)
    assert open(prefix + ".grm.bin", "rb").read() == want_k and len(want_k) == 24
    assert open(prefix + ".grm.N.bin", "rb").read() == want_n
    assert open(prefix + ".grm.id", "rb").read() == b"setA\ts0\nsetA\ts1\nsetB\ts2\n"
    assert nbytes == 48
    assert np.frombuffer(want_k, dtype="<f4")[4] == np.float32(1.0 / 3.0)


# ---- the ABI surface --------------------------------------------------------------------------------------------------------
DENSE_SYMBOLS = ["pcoa_grm_block", "pcoa_get_grm_block_stats"]


def test_dense_symbols_and_the_stats_struct_are_declared_bound_and_exported():
    lib = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "pcoa.h")).read()
    for sym in DENSE_SYMBOLS:
        assert sym in lib.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % sym, header), sym
    assert int(re.search(r"#define PCOA_VERSION_MINOR (\d+)", header).group(1)) >= 12
    assert re.search(r"#define PCOA_GRM_DIVISOR_USED\s+0\b", header) and re.search(r"#define PCOA_GRM_DIVISOR_PAIRWISE\s+1\b", header)
    assert (lib.PCOA_GRM_DIVISOR_USED, lib.PCOA_GRM_DIVISOR_PAIRWISE) == (0, 1)
    body = re.search(r"typedef struct pcoa_grm_block_stats \{(.*?)\} pcoa_grm_block_stats;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"\b(double|int64_t)\s+(\w+);", body)
    import ctypes
    kinds = {"double": ctypes.c_double, "int64_t": ctypes.c_int64}
    assert [(nm, kinds[t]) for t, nm in declared] == list(lib.PcoaGrmBlockStats._fields_)
    assert [nm for _, nm in declared] == ["grm_block_seconds", "grm_block_calls", "grm_block_flops"]
    assert not any("Not built" in ln and "reading K out" in ln for ln in header.splitlines())
    assert "; reading K out." not in open(os.path.join(ROOT, "DESIGN.md")).read()
    if os.path.exists(lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
        exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
        for sym in DENSE_SYMBOLS:
            assert sym in exported, sym


# ---- the kernels: no scratch ------------------------------------------------------------------------------------------------
def test_dense_kernels_do_not_spill_to_scratch():
    """A tile on the diagonal holds 64 VGPRs of accumulators for the two forms and 32 more with the pair counts: an accumulator
    in scratch turns the matrix-core loop into a memory loop.  hipcc reports it at compile time, for every instantiation."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                              "-I", csrc, "-c", os.path.join(csrc, "grm_dense.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True)
    assert res.returncode == 0, res.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", res.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stdout)]
    assert len(names) == len(scratch)
    assert sum("grm_dense_kernel" in nm for nm in names) == 3 and any("grm_dense_finish_kernel" in nm for nm in names), names
    for nm, sc in zip(names, scratch):
        assert sc == 0, "%s spills %d bytes/lane" % (nm, sc)
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64(" in open(os.path.join(csrc, "grm_dense.hip")).read()


# ---- the hosts: --grm-output-path -------------------------------------------------------------------------------------------
# (arguments behind --input-path X, what the message must name)
REFUSED = [
    (["--grm-output-path", "@out"], ["--grm-output-path", "--grm"]),
    (["--grm-output-divisor", "used"], ["--grm-output-divisor", "--grm"]),
    (["--grm", "--grm-output-path", "@out", "--grm-output-divisor", "mean"], ["--grm-output-divisor", "mean"]),
    (["--grm", "--grm-output-divisor", "pairwise"], ["--grm-output-divisor", "--grm-output-path"]),
    (["--grm", "--grm-output-path", "@out", "--dump-similarity", "@out"], ["--grm", "dump-similarity"]),
]


@pytest.mark.parametrize("run", [_run_driver, _run_python], ids=["driver", "python"])
@pytest.mark.parametrize("extra,what", REFUSED)
def test_both_hosts_refuse_before_any_engine_exists(inputs, run, extra, what):
    args = _args(inputs, extra)
    args.remove("--grm")                       # (_args puts one in front; the cases carry their own)
    res = run(args)
    assert res.returncode != 0, res.stdout
    for word in what:
        assert word in res.stderr, res.stderr
    assert "Matrix size" not in res.stdout and "pcoa_create" not in res.stderr and "pcoa error" not in res.stderr
    assert not os.path.exists(os.path.join(inputs["dir"], "out.tsv.grm.bin"))


def test_the_new_flags_are_off_by_default(vp):
    conf = vp.PcaConf(["--grm"])
    assert conf.grm_output_path is None and conf.grm_output_divisor is None
    conf = vp.PcaConf(["--grm", "--grm-output-path", "x", "--grm-output-divisor", "pairwise"])
    assert (conf.grm_output_path, conf.grm_output_divisor) == ("x", "pairwise")
    assert vp.GRM_OUTPUT_DIVISORS == ("used", "pairwise") and vp.GRM_OUTPUT_BAND_ROWS == 1024

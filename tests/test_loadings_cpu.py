"""CPU tests of the per-variant loadings: the numpy statement of the rule satisfies the two identities that define a left
singular vector, the hosts refuse what --loadings-output-path cannot serve before any device work, the output formatter, and
the kernels' resources.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden, load_pkg, write_golden_plink, write_golden_vcf
from loadings_cohort import centred_eig, decode_bed, encode_bed, identity_defects, loadings_rule, pack_rows, planted_cohort
from test_operator_cpu import _run_driver, _run_python

FLAG = "--loadings-output-path"


def test_the_rule_gives_the_left_singular_vectors_of_the_planted_cohort():
    """W^T W = I and (X J)^T W diag(lambda^-1/2) = U.  eigh returns U orthonormal, and B's pairs, to a few N eps; both defects
    are that error scaled by lambda_1 / lambda_3 < 1.1 on this cohort: 1e-12 is N eps times twenty."""
    x = planted_cohort()
    assert x.shape == (4096, 200)
    u, lam = centred_eig(x, 3)
    assert 2500 < lam[2] <= lam[1] <= lam[0] < 3500 and lam[2] / lam[0] > 0.9   # three planted axes of about equal weight
    w = np.asarray(loadings_rule(x, u, lam), dtype=np.float64)
    ortho, back = identity_defects(x, u, lam, w)
    print("lambda = %s, |W^T W - I| = %.3e, |(XJ)^T W / sqrt(lambda) - U| = %.3e" % (lam, ortho, back))
    assert ortho <= 1e-12 and back <= 1e-12
    # without the centring the identity does not hold: the rule's J is not decoration
    w0 = np.asarray(loadings_rule(x, u, lam, centre=False), dtype=np.float64)
    assert np.abs(w0 - w).max() > 1e-3 or np.abs(u.mean(axis=0)).max() < 1e-12


def test_the_encoders_of_the_tests_agree_with_each_other():
    rng = np.random.default_rng(5)
    for n in (6, 31, 33, 70):
        x = (rng.random((9, n)) < 0.3).astype(np.uint8)
        missing = rng.random((9, n)) < 0.1
        for a1 in (False, True):
            bed = encode_bed(x, n, missing=missing, ref_is_a1=a1, rng=rng)
            assert bed.shape == (9, (n + 3) // 4)
            assert np.array_equal(decode_bed(bed, n, ref_is_a1=a1), x & ~missing)
        bits = pack_rows(x, n, pad_words=2, garbage=rng)
        words = (n + 31) // 32
        back = np.unpackbits(bits[:, :words].copy().view(np.uint8), axis=1, bitorder="little")
        assert np.array_equal(back[:, :n], x) and (back[:, n:] == 1).all() and (bits[:, words:] == 0xffffffff).all()


# ---- host logic -------------------------------------------------------------------------------------------------------------
REFUSED = [
    (["--gpus", "2"], "--gpus"),
    (["--layout", "strips"], "--layout strips"),
    (["--project-input-path", "other.vcf"], "--project-input-path"),
    (["--outlier-iterations", "2"], "--outlier-iterations"),
    (["--related-min-jaccard", "0.5", "--remove-related"], "--remove-related"),
    (["--similarity-measure", "jaccard"], "--similarity-measure"),
    (["--similarity-measure", "cosine"], "--similarity-measure"),
]


@pytest.mark.parametrize("gram", ["stored", "implicit"])
@pytest.mark.parametrize("extra,what", REFUSED)
def test_both_hosts_refuse_before_any_device_work(extra, what, gram, tmp_path):
    """The input does not exist: a host that got as far as reading it, or as creating an engine, fails differently."""
    args = ["--input-path", str(tmp_path / "absent.bed"), FLAG, str(tmp_path / "w.tsv"), "--gram", gram] + extra
    for run in (_run_driver, _run_python):
        res = run(args)
        assert res.returncode != 0, res.stdout
        assert "VariantsPcaDriver:" in res.stderr and not os.path.exists(str(tmp_path / "w.tsv"))
        if gram == "stored":
            assert FLAG in res.stderr and what in res.stderr, res.stderr
        else:   # (--gram implicit refuses most of these itself, first, by its own rules: either refusal names its flag)
            assert FLAG in res.stderr or "--gram implicit" in res.stderr, res.stderr


def test_compiled_host_refuses_a_stored_s_over_a_vcf(tmp_path):
    g = load_golden("kat5")
    write_golden_vcf(g, str(tmp_path / "kat5.vcf"))
    res = _run_driver(["--input-path", str(tmp_path / "kat5.vcf"), "--all-references", FLAG, str(tmp_path / "w.tsv")])
    assert res.returncode != 0 and FLAG in res.stderr and "--gram implicit" in res.stderr, res.stderr
    write_golden_plink(g, str(tmp_path / "kat5"))
    res = _run_driver(["--input-path", str(tmp_path / "kat5.bed"), "--all-references", "--no-stream", FLAG, str(tmp_path / "w.tsv")])
    assert res.returncode != 0 and FLAG in res.stderr and "--gram implicit" in res.stderr, res.stderr
    res = _run_driver(["--input-path", str(tmp_path / "kat5.bed"), "--all-references", "--parse-only", FLAG, str(tmp_path / "w.tsv")])
    assert res.returncode != 0 and FLAG in res.stderr and "--parse-only" in res.stderr, res.stderr


def test_python_host_refuses_a_repeated_callset_by_the_flags_name():
    vp = load_pkg("variants_pca")
    with pytest.raises(SystemExit) as e:
        vp.calls_as_bits([[0, 1], [2, 2, 3]], 5, flag=FLAG, instead="carrier lists that are sets")
    assert FLAG in str(e.value) and "twice" in str(e.value)
    with pytest.raises(SystemExit) as e:      # the --gram implicit message is what it was
        vp.calls_as_bits([[2, 2]], 5)
    assert "--gram implicit" in str(e.value) and "--gram stored" in str(e.value)
    kind, bits = vp.calls_as_bits([[0, 1], [4]], 5, flag=FLAG)
    assert kind == "bits" and bits.tolist() == [[3], [16]]


def test_formatter_and_line_order(tmp_path):
    vp = load_pkg("variants_pca")
    w = np.array([[0.25, -1.5e-7, 12345678.0], [0.0, 1.0 / 3.0, -2.0], [1e-3, 2.5e-300, 100.0]])
    meta = [("17", 41196312, "rs1"), ("17", 41196319, "."), ("2", 7, "id;with,marks")]
    path = str(tmp_path / "w.tsv")
    vp.write_loadings(path, meta, w)
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == 4
    assert lines[0] == "0\t17\t41196312\trs1\t0.25\t-1.5E-7\t1.2345678E7"
    assert lines[1] == "1\t17\t41196319\t.\t0.0\t0.3333333333333333\t-2.0"
    assert lines[2] == "2\t2\t7\tid;with,marks\t0.001\t2.5E-300\t100.0"
    vp.write_loadings(path, None, w[:2, :1])          # an input without variant records
    assert open(path).read() == "0\t.\t.\t.\t0.25\n1\t.\t.\t.\t0.0\n"
    with pytest.raises(RuntimeError):
        vp.write_loadings(path, meta[:2], w)


@pytest.mark.parametrize("kind", ["vcf", "plink"])
def test_ingest_records_one_entry_per_row_and_only_when_asked(kind, tmp_path):
    """Contig, position and id are recorded during ingest only with the flag; one entry per row that reaches the engine."""
    ingest = load_pkg("ingest")
    g = load_golden("kat5")
    if kind == "vcf":
        write_golden_vcf(g, str(tmp_path / "kat5.vcf"))
        meta = []
        _, _, data = ingest.load_vcf(str(tmp_path / "kat5.vcf"), None, variant_meta=meta)
        rows = len(data[0][2]) - 1
        assert ingest.load_vcf(str(tmp_path / "kat5.vcf"), None)[2][0][2].tolist() == data[0][2].tolist()
        assert all(m[0] == "17" and m[2] == "." for m in meta)
    else:
        write_golden_plink(g, str(tmp_path / "kat5"))
        meta = []
        _, _, data = ingest.load_plink(str(tmp_path / "kat5.bed"), None, as_bed=True, variant_meta=meta)
        rows = int(data[0][2].sum())
        assert all(m[0] == "17" and m[2].startswith("rs") for m in meta)
    assert rows > 0 and len(meta) == rows
    assert [m[1] for m in meta] == sorted(m[1] for m in meta) and all(isinstance(m[1], int) for m in meta)


# ---- the kernels' resources ---------------------------------------------------------------------------------------------------
def test_no_loadings_kernel_spills_and_the_record_is_current():
    """Every instantiation (K = 1, 2, 4, 8 components x 8, 16, 32, 64 lanes per row) compiles for gfx950 without scratch and with
    at least two waves per SIMD, and profiles/r13a_loadings_kernel_resources.txt lists each of them."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import tempfile
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                              "-c", os.path.join(csrc, "loadings.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True)
    assert res.returncode == 0, res.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", res.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stdout)]
    occupancy = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", res.stdout)]
    assert len(names) == 16 and len(scratch) == 16 and len(occupancy) == 16
    assert all("loadings_kernel" in nm for nm in names)
    assert scratch == [0] * 16 and min(occupancy) >= 2
    record = open(os.path.join(ROOT, "profiles", "r13a_loadings_kernel_resources.txt")).read()
    for nm in names:
        assert nm in record, nm

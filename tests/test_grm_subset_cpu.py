"""CPU tests of the sample subsets of a GRM store (pcoa_create_grm_subset, pcoa_grm_rows, --grm-keep-samples / --grm-remove-samples
/ --grm-outlier-iterations / --grm-project-removed): the numpy statement on the packed bytes agrees with slicing unpacked codes,
the planted cohort of the outlier rounds does what the GPU test relies on, the ABI surface, the kernel's resources, and the
command-line surface of both hosts, which refuse a wrong combination or a wrong list before any engine exists."""
import os
import re
import subprocess

import numpy as np
import pytest

import grm_subset_cohort as C
from conftest import ROOT, load_pkg
from test_grm_cpu import _run_driver, _run_python, balding_nichols, dense_k, edge_rows, exact_cohort, inputs, pack_bed, \
    random_codes  # noqa: F401  (inputs: the fixture with a PLINK fileset and a VCF)


# ---- the spec ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 16, 17, 33, 64, 130, 1025])
def test_spec_on_packed_bytes_equals_slicing_the_unpacked_codes(n):
    rng = np.random.default_rng(n)
    cohorts = [random_codes(rng, 9, n, missing=0.2)]
    if n >= 2:
        cohorts += [edge_rows(random_codes(rng, 9, n, missing=0.2)), exact_cohort(rng, n, 4, 3), balding_nichols(rng, n, 6)]
    for codes in cohorts:
        rows = pack_bed(codes, 2, rng)                                   # garbage in the padding slots and two extra bytes
        assert np.array_equal(C.unpack_rows(rows, n), codes)
        for ref_is_a1 in (True, False):
            store = C.store_rows(rows, n, ref_is_a1)
            assert store.shape == (codes.shape[0], (n + 3) // 4)
            assert np.array_equal(store, pack_bed(codes if ref_is_a1 else C.SWAP[codes]))       # tail slots 00
            for name, keep in C.keep_patterns(n, int(ref_is_a1)).items():
                got = C.spec_grm_subset_rows(store, n, keep)
                want = pack_bed((codes if ref_is_a1 else C.SWAP[codes])[:, keep]) if keep.size else np.zeros((codes.shape[0], 0), np.uint8)
                assert np.array_equal(got, want), (name, ref_is_a1)
                if name == "identity":
                    assert np.array_equal(got, store)


@pytest.mark.parametrize("n", [32, 33, 130, 4100])
def test_keep_patterns_are_legal_lists_of_the_kinds_the_issue_names(n):
    pats = C.keep_patterns(n)
    assert sorted(pats) == sorted(["identity", "first_dropped", "last_dropped", "one_mid_word", "every_second", "one_per_16", "block",
                                   "random_3pct", "random_50pct"])
    for name, keep in pats.items():
        assert keep.dtype == np.int32 and keep.size >= 1 and keep[0] >= 0 and keep[-1] < n and np.all(np.diff(keep) > 0), name
    assert pats["identity"].size == n and pats["first_dropped"][0] == 1 and pats["last_dropped"][-1] == n - 2
    gone = np.setdiff1d(np.arange(n), pats["one_mid_word"])
    assert gone.size == 1 and gone[0] % 16 not in (0, 15)                 # mid-word
    assert np.all(np.diff(pats["one_per_16"]) == 16)                      # every output word reads 16 source words
    gone = np.setdiff1d(np.arange(n), pats["block"])
    assert gone.size >= 1 and np.all(np.diff(gone) == 1)


def test_the_planted_cohort_loses_exactly_its_three_samples_in_round_one():
    """numpy's eigh of the dense K and the hosts' rule at 6 sigma: round 1 removes the three all-het samples and nobody else,
    round 2 -- frequencies re-estimated on the survivors -- removes nothing.  The margins are wide: 8.8 sigma against at most
    3.5, so the device's eigenvectors make the same decisions."""
    vp = load_pkg("variants_pca")
    codes, planted = C.planted_outlier_cohort()
    kept = np.arange(codes.shape[1])
    out = []
    for _ in range(2):
        lam, u = np.linalg.eigh(dense_k(codes[:, kept], False))
        comps = u[:, ::-1][:, :2].T
        z = np.abs(comps - comps.mean(axis=1, keepdims=True)) / comps.std(axis=1, keepdims=True)
        removed = vp.outlier_rule(comps, 6.0)
        out.append((kept[removed], z))
        kept = kept[~removed]
    assert np.array_equal(out[0][0], planted) and out[1][0].size == 0
    z1, z2 = out[0][1], out[1][1]
    assert z1[1, planted].min() > 8.0 and np.delete(z1, planted, axis=1).max() < 4.0 and z2.max() < 4.0
    assert kept.size == codes.shape[1] - 3 >= max(vp.GRM_MIN_COHORT, 3)


# ---- the ABI surface --------------------------------------------------------------------------------------------------------
GRM_SUBSET_SYMBOLS = ["pcoa_create_grm_subset", "pcoa_grm_rows", "pcoa_get_grm_subset_stats"]


def test_grm_subset_symbols_are_declared_bound_and_exported():
    lib = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "pcoa.h")).read()
    for sym in GRM_SUBSET_SYMBOLS:
        assert sym in lib.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % sym, header), sym
    assert int(re.search(r"#define PCOA_VERSION_MINOR (\d+)", header).group(1)) >= 14
    assert re.search(r"#define PCOA_GRM_SUBSET_PANEL 0\b", header) and re.search(r"#define PCOA_GRM_SUBSET_STUDY 1\b", header)
    assert (lib.PCOA_GRM_SUBSET_PANEL, lib.PCOA_GRM_SUBSET_STUDY) == (0, 1)
    assert [f[0] for f in lib.PcoaGrmSubsetStats._fields_] == re.findall(r"^\s+(?:int64_t|double) (grm_subset_\w+);", header, flags=re.M)
    assert "DESIGN.md 4.20" in header
    eng = load_pkg("engine").PcoaEngine
    for method in ("grm_subset", "grm_rows", "grm_subset_stats"):
        assert callable(getattr(eng, method))
    if os.path.exists(lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
        exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
        for sym in GRM_SUBSET_SYMBOLS:
            assert sym in exported, sym


def test_grm_subset_kernel_does_not_spill_to_scratch():
    """The gather keeps 16 source indices and a tile of loaded and assembled words per lane, all indexed at compile time: an array
    that lands in scratch turns every extract into a memory access.  hipcc reports it at compile time.  The row tile the GPU
    tests put their row counts around is the source's."""
    import shutil
    import tempfile
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    source = open(os.path.join(csrc, "grm_subset.hip")).read()
    assert re.search(r"constexpr int kGrmSubsetTileRows = 8;", source)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                              "-I", csrc, "-c", os.path.join(csrc, "grm_subset.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True)
    assert res.returncode == 0, res.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", res.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stdout)]
    assert len(names) == len(scratch)
    assert any("grm_subset_kernel" in nm for nm in names), "no grm_subset_kernel in grm_subset.hip"
    for nm, sc in zip(names, scratch):
        assert sc == 0, "%s spills %d bytes/lane" % (nm, sc)


# ---- the hosts --------------------------------------------------------------------------------------------------------------
# (arguments behind --input-path BED, with or without --grm; the two things the message must name).  @list: a file with two
# sample names of the fileset; @unknown: one that is no sample; @twice: one name two times; @out: a path that must not appear
REFUSED = [
    (["--grm-keep-samples", "@list"], "--grm-keep-samples", "--grm "),
    (["--grm-remove-samples", "@list"], "--grm-remove-samples", "--grm "),
    (["--grm-outlier-iterations", "2"], "--grm-outlier-iterations", "--grm "),
    (["--grm-outlier-sigma", "5"], "--grm-outlier-sigma", "--grm "),
    (["--grm-project-removed"], "--grm-project-removed", "--grm "),
    (["--grm", "--grm-keep-samples", "@list", "--grm-remove-samples", "@list"], "--grm-keep-samples", "--grm-remove-samples"),
    (["--grm", "--grm-remove-samples", "@unknown"], "--grm-remove-samples", "NOBODY"),
    (["--grm", "--grm-keep-samples", "@unknown"], "--grm-keep-samples", "NOBODY"),
    (["--grm", "--grm-remove-samples", "@twice"], "--grm-remove-samples", "twice"),
    (["--grm", "--grm-keep-samples", "@twice"], "--grm-keep-samples", "twice"),
    (["--grm", "--grm-outlier-iterations", "-1"], "--grm-outlier-iterations", ">= 0"),
    (["--grm", "--grm-outlier-iterations", "1", "--grm-outlier-sigma", "nan"], "--grm-outlier-sigma", "finite"),
    (["--grm", "--grm-outlier-iterations", "1", "--grm-outlier-sigma", "inf"], "--grm-outlier-sigma", "finite"),
    (["--grm", "--grm-outlier-iterations", "1", "--grm-outlier-sigma", "0"], "--grm-outlier-sigma", "finite"),
    (["--grm", "--grm-outlier-iterations", "1", "--outlier-iterations", "1"], "--grm", "outlier-iterations"),
]


@pytest.fixture(scope="module")
def lists(inputs):  # noqa: F811
    with open(inputs["bed"][:-4] + ".fam") as f:
        names = [ln.split()[1] for ln in f if ln.strip()]
    out = {}
    for tag, lines in (("@list", names[:2]), ("@unknown", [names[0], "NOBODY"]), ("@twice", [names[1], names[0], names[1]])):
        out[tag] = os.path.join(inputs["dir"], tag[1:] + ".txt")
        with open(out[tag], "w") as f:
            f.write("".join(ln + "\n" for ln in lines))
    out["@out"] = os.path.join(inputs["dir"], "subset_out")
    return out


@pytest.mark.parametrize("run", [_run_driver, _run_python], ids=["cpp", "py"])
@pytest.mark.parametrize("extra,first,second", REFUSED)
def test_hosts_refuse_before_any_engine_exists(inputs, lists, run, extra, first, second):  # noqa: F811
    res = run(["--input-path", inputs["bed"], "--grm-output-path", lists["@out"]][:2 + 2 * ("--grm" in extra)] + [lists.get(a, a) for a in extra])
    assert res.returncode != 0 and first in res.stderr and second in res.stderr, res.stderr
    assert "Matrix size" not in res.stdout and "pcoa_create" not in res.stderr and "pcoa error" not in res.stderr
    assert not os.path.exists(lists["@out"] + ".grm.id")


@pytest.mark.parametrize("run", [_run_driver, _run_python], ids=["cpp", "py"])
def test_hosts_refuse_a_list_that_leaves_too_small_a_cohort(inputs, lists, run):  # noqa: F811
    """A GRM engine starts at 32 samples: keeping two is refused with the flag's name, before any engine exists."""
    res = run(["--input-path", inputs["bed"], "--grm", "--grm-keep-samples", lists["@list"]])
    assert res.returncode != 0 and "--grm-keep-samples" in res.stderr and "32" in res.stderr, res.stderr
    assert "Matrix size" not in res.stdout and "pcoa_create" not in res.stderr and "pcoa error" not in res.stderr


def test_the_flags_parse_and_default_off():
    vp = load_pkg("variants_pca")
    conf = vp.PcaConf([])
    assert conf.grm_keep_samples is None and conf.grm_remove_samples is None and conf.grm_outlier_iterations == 0
    assert conf.grm_outlier_sigma is None and conf.grm_project_removed is False and vp.GRM_OUTLIER_SIGMA == 6.0
    conf = vp.PcaConf(["--input-path", "x.bed", "--grm", "--grm-remove-samples", "x.txt", "--grm-outlier-iterations", "3", "--grm-outlier-sigma", "4.5",
                       "--grm-project-removed"])
    assert conf.grm_remove_samples == "x.txt" and conf.grm_outlier_iterations == 3 and conf.grm_outlier_sigma == 4.5
    assert conf.grm_project_removed is True
    vp.check_grm_conf(conf)
    conf = vp.PcaConf(["--input-path", "x.bed", "--grm", "--grm-outlier-iterations", "1"])
    vp.check_grm_conf(conf)
    assert conf.grm_outlier_sigma == 6.0
    usage = subprocess.run([os.path.join(ROOT, "spark-examples_amd", "variants_pca_driver"), "--help"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, universal_newlines=True).stdout \
        if os.path.exists(os.path.join(ROOT, "spark-examples_amd", "variants_pca_driver")) else None
    if usage is not None:
        for flag in ("--grm-keep-samples", "--grm-remove-samples", "--grm-outlier-iterations", "--grm-outlier-sigma", "--grm-project-removed"):
            assert flag in usage, flag

"""CPU tests of the KING-robust kinship screen on the 2-bit store of a GRM engine (pcoa_grm_king_block, pcoa_grm_king_pairs): the
numpy statement variants_pca.grm_king_rule against a plain double loop over pairs and against king_counts of the five plane
Grams, the four-product identity the count kernel rests on, grm_king_pairs_rule against king_pairs_rule with a tie at the
cutoff, the ABI surface, the compile-time resource check of grm_king.hip, the command-line surface of both hosts, which must
refuse the new flags before any engine exists and in the same words, and the writer of the pair file."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import king_cohort as K
from conftest import ROOT, load_pkg
from test_grm_cpu import _args, _run_driver, _run_python, edge_rows, inputs, random_codes  # noqa: F401  (inputs is a fixture)


@pytest.fixture(scope="module")
def vp():
    return load_pkg("variants_pca")


def grams_of(vp, code):
    return [K.gram(p) for p in vp.king_planes(code)]


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def loop_rule(codes):
    v, n = codes.shape
    hethet = np.zeros((n, n), dtype=np.int64)
    ibs0 = np.zeros((n, n), dtype=np.int64)
    het_sum = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        for j in range(n):
            a, b = codes[:, i], codes[:, j]
            hethet[i, j] = int(((a == 2) & (b == 2)).sum())
            ibs0[i, j] = int((((a == 0) & (b == 3)) | ((a == 3) & (b == 0))).sum())
            het_sum[i, j] = int(((a == 2) & (b != 1)).sum() + ((a != 1) & (b == 2)).sum())
    return hethet, ibs0, het_sum


@pytest.mark.parametrize("v,n", [(1, 5), (70, 33), (300, 40)])
def test_the_rule_is_a_plain_double_loop(vp, v, n):
    rng = np.random.default_rng(v + n)
    codes = edge_rows(random_codes(rng, v, n, missing=0.15))
    got = vp.grm_king_rule(codes)
    want = loop_rule(codes)
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w)
    # the diagonal identities, and the symmetry
    h = (codes == 2).sum(axis=0)
    assert np.array_equal(np.diagonal(got[0]), h) and not np.diagonal(got[1]).any() and np.array_equal(np.diagonal(got[2]), 2 * h)
    for g in got:
        assert np.array_equal(g, g.T)
    # a mask of counted rows is the rule on those rows; the two homozygotes may change places
    counted = rng.random(v) < 0.5
    for g, w in zip(vp.grm_king_rule(codes, counted), vp.grm_king_rule(codes[counted])):
        assert np.array_equal(g, w)
    swapped = np.array([3, 1, 2, 0], dtype=np.uint8)[codes]
    for g, w in zip(vp.grm_king_rule(swapped), got):
        assert np.array_equal(g, w)
    with pytest.raises(ValueError):
        vp.grm_king_rule(codes, counted[:-1] if v > 1 else np.zeros(2, bool))
    with pytest.raises(ValueError):
        vp.grm_king_rule(np.full((2, 3), 4))


@pytest.mark.parametrize("n,v", [(70, 3000), (260, 2000)])
def test_the_rule_equals_the_counts_of_the_five_plane_grams(vp, n, v):
    code = K.codes(n, v)
    _, h, hethet, ibs0, het_sum = vp.king_counts(grams_of(vp, code))
    got = vp.grm_king_rule(code)
    assert np.array_equal(got[0], hethet) and np.array_equal(got[1], ibs0) and np.array_equal(got[2], het_sum)   # diagonal included
    assert np.array_equal(np.diagonal(got[0]), h)


@pytest.mark.parametrize("v,n", [(66, 33), (515, 65)])
def test_the_four_product_identity(vp, v, n):
    """The count kernel contracts four symmetric products with one int8 operand each and combines them in its epilogue."""
    rng = np.random.default_rng(5 * v + n)
    codes = edge_rows(random_codes(rng, v, n, missing=0.2))
    h = (codes == 2).astype(np.int64)
    c = (codes != 1).astype(np.int64)
    x = (codes == 3).astype(np.int64) - (codes == 0).astype(np.int64)
    hh, cc, qq, xx = h.T @ h, c.T @ c, (h + c).T @ (h + c), x.T @ x
    assert set(np.unique(h + c)) <= {0, 1, 2} and set(np.unique(x)) <= {-1, 0, 1}
    twice = 2 * cc + 2 * hh - qq - xx
    assert not (twice & 1).any()
    hethet, ibs0, het_sum = vp.grm_king_rule(codes)
    assert np.array_equal(hh, hethet) and np.array_equal(qq - hh - cc, het_sum) and np.array_equal(twice // 2, ibs0)


def tie_codes():
    """Sample 1 is a copy of sample 0 with every call made: num = hethet, het_sum = 2 hethet, the kinship is exactly 0.5.  Sample
    3 is a copy of sample 2 with one het turned into a homozygote: just below 0.5."""
    rng = np.random.default_rng(50)
    codes = random_codes(rng, 400, 40, missing=0.0)
    codes[:, 1] = codes[:, 0]
    codes[:, 3] = codes[:, 2]
    codes[np.flatnonzero(codes[:, 2] == 2)[0], 3] = 0
    return codes


def test_pairs_rule_equals_the_plane_rule_with_a_tie_at_the_cutoff(vp):
    for code in (K.codes(70, 3000), edge_rows(random_codes(np.random.default_rng(9), 300, 130))):
        grams = grams_of(vp, code)
        for x in (0.0442, 0.0884, K.CUTOFF, 0.354, 0.5):
            got, want = vp.grm_king_pairs_rule(code, x), vp.king_pairs_rule(grams, x)
            assert got.dtype == vp.KING_PAIR_DTYPE and got.tobytes() == want.tobytes(), x
    planted = vp.grm_king_pairs_rule(K.codes(70, 3000), K.CUTOFF)
    assert [(int(p["i"]), int(p["j"])) for p in planted] == K.planted_pairs(70)
    codes = tie_codes()
    got = vp.grm_king_pairs_rule(codes, 0.5)
    assert got.tobytes() == vp.king_pairs_rule(grams_of(vp, codes), 0.5).tobytes()
    assert [(int(p["i"]), int(p["j"])) for p in got] == [(0, 1)]                        # >= reports the tie, and only the tie
    assert int(got["ibs0"][0]) == 0 and int(got["het_sum"][0]) == 2 * int(got["hethet"][0]) > 0


# ---- the ABI surface --------------------------------------------------------------------------------------------------------
KING_SYMBOLS = ["pcoa_grm_king_block", "pcoa_grm_king_pairs", "pcoa_get_grm_king_stats"]


def test_symbols_the_record_and_the_stats_struct_are_declared_bound_and_exported(vp):
    lib = load_pkg("_lib")
    P = load_pkg()
    header = open(os.path.join(ROOT, "include", "pcoa.h")).read()
    for sym in KING_SYMBOLS:
        assert sym in lib.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % sym, header), sym
    assert int(re.search(r"#define PCOA_VERSION_MINOR (\d+)", header).group(1)) >= 18
    # the record is pcoa_king_pair, unchanged: 32 bytes, the same fields in the header, ctypes and both numpy dtypes
    rec = re.search(r"typedef struct pcoa_king_pair \{(.*?)\} pcoa_king_pair;", header, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", rec).strip() == "int32_t i, j; int64_t hethet, ibs0, het_sum;"
    assert "pcoa_king_pair* out_pairs" in header[header.index("int pcoa_grm_king_pairs("):]
    assert ctypes.sizeof(lib.PcoaKingPair) == 32
    for dt in (vp.KING_PAIR_DTYPE, P.PcoaEngine.KING_PAIR_DTYPE):
        assert dt.itemsize == 32 and dt.names == ("i", "j", "hethet", "ibs0", "het_sum")
        assert [dt.fields[f][1] for f in dt.names] == [getattr(lib.PcoaKingPair, f).offset for f in dt.names] == [0, 4, 8, 16, 24]
    body = re.search(r"typedef struct pcoa_grm_king_stats \{(.*?)\} pcoa_grm_king_stats;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"\b(double|int64_t)\s+(\w+);", body)
    kinds = {"double": ctypes.c_double, "int64_t": ctypes.c_int64}
    assert [(nm, kinds[t]) for t, nm in declared] == list(lib.PcoaGrmKingStats._fields_)
    assert [nm for _, nm in declared] == ["grm_king_seconds", "grm_king_screen_seconds", "grm_king_calls", "grm_king_bands",
                                          "grm_king_macs", "grm_king_bytes", "grm_king_block_calls"]
    for name in ("grm_king_block", "grm_king_pairs", "grm_king_stats"):
        assert callable(getattr(P.PcoaEngine, name))
    # the item has left the lists of what is not built
    assert not any("Not built" in ln and "KING screen" in ln for ln in header.splitlines())
    assert "a KING screen over the 2-bit store, " not in header and "a KING screen that feeds a GRM engine in one run. */" not in header
    if os.path.exists(lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
        exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
        for sym in KING_SYMBOLS:
            assert sym in exported, sym


# ---- the kernels: no scratch ------------------------------------------------------------------------------------------------
def test_kernels_do_not_spill_to_scratch_and_need_no_lds_for_the_counts():
    """The count kernel holds 64 int32 accumulators, the 32 store words of a k-step and the eight operand fragments in
    registers; in scratch every k-step would go to memory twice.  hipcc reports it at compile time, for every instantiation."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                              "-I", csrc, "-c", os.path.join(csrc, "grm_king.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True)
    assert res.returncode == 0, res.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", res.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stdout)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", res.stdout)]
    assert len(names) == len(scratch) == len(lds)
    for kernel, count in (("grm_king_counts_kernel", 2), ("grm_king_screen_count_kernel", 1), ("grm_king_screen_write_kernel", 1)):
        assert sum(kernel in nm for nm in names) == count, names
    for nm, sc, ld in zip(names, scratch, lds):
        assert sc == 0, "%s spills %d bytes/lane" % (nm, sc)
        if "grm_king_counts_kernel" in nm:
            assert ld == 0, "%s uses %d bytes of LDS" % (nm, ld)
    src = open(os.path.join(csrc, "grm_king.hip")).read()
    assert src.count("atomicAdd(") == 1 and "atomicAdd(entries_read" in src      # the one atomic is the integer byte counter
    assert src.count("__builtin_amdgcn_mfma_i32_32x32x32_i8(") == 4              # one contraction per product


# ---- the hosts --------------------------------------------------------------------------------------------------------------
# (arguments behind --input-path X, what the message must name)
PAIR = ["--grm", "--grm-king-cutoff", "0.177"]
REFUSED = [
    (["--grm-king-cutoff", "0.177"], ["--grm-king-cutoff", "--grm"]),
    (["--grm-king-rows", "all"], ["--grm-king-rows", "--grm"]),
    (["--grm-king-output-path", "@out"], ["--grm-king-output-path", "--grm"]),
    (["--grm-king-max-pairs", "5"], ["--grm-king-max-pairs", "--grm"]),
    (["--grm-king-remove"], ["--grm-king-remove", "--grm"]),
    (["--grm", "--grm-king-rows", "all"], ["--grm-king-rows", "--grm-king-cutoff X"]),
    (["--grm", "--grm-king-output-path", "@out"], ["--grm-king-output-path", "--grm-king-cutoff X"]),
    (["--grm", "--grm-king-max-pairs", "5"], ["--grm-king-max-pairs", "--grm-king-cutoff X"]),
    (["--grm", "--grm-king-remove"], ["--grm-king-remove", "--grm-king-cutoff X"]),
    (["--grm", "--grm-king-cutoff", "nan"], ["--grm-king-cutoff", "(0, 0.5]"]),
    (["--grm", "--grm-king-cutoff", "inf", "--grm-king-output-path", "@out"], ["--grm-king-cutoff", "(0, 0.5]"]),
    (["--grm", "--grm-king-cutoff", "0"], ["--grm-king-cutoff", "(0, 0.5]"]),
    (["--grm", "--grm-king-cutoff", "0.51"], ["--grm-king-cutoff", "(0, 0.5]"]),
    (PAIR + ["--grm-king-rows", "some"], ["--grm-king-rows", "some"]),
    (PAIR + ["--grm-king-max-pairs", "-1"], ["--grm-king-max-pairs", ">= 0"]),
    (PAIR + ["--grm-king-remove", "--grm-cutoff", "0.05", "--grm-cutoff-remove"], ["--grm-king-remove", "--grm-cutoff-remove"]),
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
    assert not os.path.exists(os.path.join(inputs["dir"], "out.tsv"))


def test_both_hosts_refuse_in_the_same_words(inputs):
    for extra, _ in REFUSED:
        args = _args(inputs, extra)
        args.remove("--grm")
        a, b = _run_driver(args), _run_python(args)
        line = lambda res: [ln for ln in res.stderr.splitlines() if "--grm-king" in ln][-1]
        assert line(a).split("VariantsPcaDriver: ")[-1] == line(b).split("VariantsPcaDriver: ")[-1], extra


def test_the_new_flags_are_off_by_default(vp):
    conf = vp.PcaConf(["--grm"])
    assert conf.grm_king_cutoff is None and conf.grm_king_rows is None and conf.grm_king_output_path is None
    assert conf.grm_king_remove is False and conf.grm_king_max_pairs == 1 << 20 and not conf.grm_king_max_pairs_given
    conf = vp.PcaConf(["--grm", "--grm-king-cutoff", "0.177", "--grm-king-rows", "all", "--grm-king-output-path", "x",
                       "--grm-king-max-pairs", "7", "--grm-king-remove"])
    assert (conf.grm_king_cutoff, conf.grm_king_rows, conf.grm_king_output_path, conf.grm_king_max_pairs, conf.grm_king_remove) == \
        (0.177, "all", "x", 7, True)


def test_the_pair_file_byte_for_byte(vp, tmp_path):
    pairs = np.zeros(2, dtype=vp.KING_PAIR_DTYPE)
    pairs["i"], pairs["j"] = [0, 2], [1, 3]
    pairs["hethet"], pairs["ibs0"], pairs["het_sum"] = [10, 12], [0, 2], [20, 32]
    path = str(tmp_path / "king.tsv")
    vp.write_king_pairs(path, pairs, ["a", "b b", "c", "d"])
    assert open(path, "rb").read() == (b"name_i\tname_j\thethet\tibs0\thet_sum\tkinship\n"
                                       b"a\tb b\t10\t0\t20\t0.5\n"
                                       b"c\td\t12\t2\t32\t0.25\n")

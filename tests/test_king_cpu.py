"""CPU tests of the KING-robust kinship screen (pcoa_king_*, --king-cutoff): the numpy rule against a triple loop over genotype
codes, the threshold, the decode restated in numpy, the cohort the GPU tests hand to the engine and the hosts
(tests/king_cohort.py), the CLI surface of both hosts with no engine attempted, the header and the binding, and the kernels'
resource report.  Every comparison is exact."""
import ctypes
import io
import os
import re
import shutil
import subprocess
import tempfile
from contextlib import redirect_stdout

import numpy as np
import pytest

import king_cohort as K
from conftest import ROOT, load_pkg


@pytest.fixture(scope="module")
def vp():
    return load_pkg("variants_pca")


def grams_of(vp, code):
    return [K.gram(p) for p in vp.king_planes(code)]


# ---- king_counts against a triple loop --------------------------------------------------------------------------------------------
def loop_counts(code):
    """(V, h, hethet, ibs0, het_sum) by definition: a loop over the pairs and their variants' codes."""
    v, n = code.shape
    h = np.array([int((code[:, i] == 2).sum()) for i in range(n)], dtype=np.int64)
    hethet = np.zeros((n, n), dtype=np.int64)
    ibs0 = np.zeros((n, n), dtype=np.int64)
    het_sum = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        for j in range(n):
            for r in range(v):
                a, b = int(code[r, i]), int(code[r, j])
                if a == 1 or b == 1:                    # not jointly called
                    continue
                hethet[i, j] += a == 2 and b == 2
                ibs0[i, j] += (a == 0 and b == 3) or (a == 3 and b == 0)
                het_sum[i, j] += (a == 2) + (b == 2)
    return v, h, hethet, ibs0, het_sum


def small_codes(n, v, seed):
    """Codes with every class, one sample all-missing (het_sum = 0 against everybody: the guard) and two samples that are
    never missing at the same variant as each other (G_M = 0 off the diagonal)."""
    rng = np.random.default_rng(seed)
    code = rng.choice(np.arange(4, dtype=np.uint8), size=(v, n), p=[0.35, 0.15, 0.3, 0.2])
    code[:, 4] = 1
    both = (code[:, 0] == 1) & (code[:, 1] == 1)
    code[both, 1] = 2
    return code


@pytest.mark.parametrize("n,v", [(70, 60), (260, 25)])
def test_king_counts_against_a_triple_loop(vp, n, v):
    code = small_codes(n, v, n)
    g = grams_of(vp, code)
    assert g[1][0, 1] == 0 and g[1][0, 0] > 0 and g[1][1, 1] > 0          # M = 0 off the diagonal for the pair (0, 1)
    got = vp.king_counts(g)
    want = loop_counts(code)
    assert got[0] == want[0] == v
    for a, b in zip(got[1:], want[1:]):
        assert a.dtype == np.int64 and np.array_equal(a, b)
    assert (got[4][4, :] == 0).all()                                      # the all-missing sample shares no called site
    pairs = vp.king_pairs_rule(g, 1e-9)
    assert pairs.dtype == vp.KING_PAIR_DTYPE and pairs.dtype.itemsize == 32
    assert not ((pairs["i"] == 4) | (pairs["j"] == 4)).any()              # het_sum > 0 guards the empty pair
    brute = [(i, j) for i in range(n) for j in range(i + 1, n)
             if want[4][i, j] > 0 and float(want[2][i, j] - 2 * want[3][i, j]) >= 1e-9 * float(want[4][i, j])]
    assert [(int(p["i"]), int(p["j"])) for p in pairs] == brute


def test_the_all_missing_sample_has_no_joint_site(vp):
    code = small_codes(12, 40, 3)
    _, _, hethet, ibs0, het_sum = vp.king_counts(grams_of(vp, code))
    assert (het_sum[4] == 0).all() and (hethet[4] == 0).all() and (ibs0[4] == 0).all()


def test_king_counts_names_the_inconsistency(vp):
    code = small_codes(12, 40, 5)
    g = grams_of(vp, code)
    short = [m.copy() for m in g]
    short[3] = K.gram(vp.king_planes(code[:-1])[3])                       # R fed one row fewer
    with pytest.raises(ValueError, match="V = r_i"):
        vp.king_counts(short)
    with pytest.raises(ValueError, match="not fed the same rows"):
        vp.king_counts([g[0], g[3], g[2], g[1], g[4]])                    # R and M swapped
    with pytest.raises(ValueError):
        vp.king_counts(g[:4])


# ---- the threshold ----------------------------------------------------------------------------------------------------------------
def threshold_codes():
    """Three samples over V = 40 variants, no missing call.  Samples 0 and 1: 12 variants het / het, 4 het / hom, 4 hom / het,
    2 opposite homozygotes, 18 identical homozygotes: hethet = 12, ibs0 = 2, het_sum = 16 + 16 = 32, so
    num / het_sum = (12 - 2 * 2) / 32 = 0.25 exactly.  Sample 2 is homozygous A1 everywhere."""
    code = np.zeros((40, 3), dtype=np.uint8)
    code[:12, 0] = 2; code[:12, 1] = 2                                    # 12 het / het
    code[12:16, 0] = 2; code[12:16, 1] = 3                                # 4 het / hom
    code[16:20, 0] = 0; code[16:20, 1] = 2                                # 4 hom / het
    code[20:22, 0] = 0; code[20:22, 1] = 3                                # 2 opposite homozygotes
    code[22:, 0] = 3; code[22:, 1] = 3
    return code


def test_king_pairs_rule_on_the_threshold(vp):
    code = threshold_codes()
    g = grams_of(vp, code)
    v, h, hethet, ibs0, het_sum = vp.king_counts(g)
    assert (v, int(hethet[0, 1]), int(ibs0[0, 1]), int(het_sum[0, 1])) == (40, 12, 2, 32) and list(h) == [16, 16, 0]
    at = vp.king_pairs_rule(g, 0.25)
    assert [(int(p["i"]), int(p["j"]), int(p["hethet"]), int(p["ibs0"]), int(p["het_sum"])) for p in at] == [(0, 1, 12, 2, 32)]
    assert list(vp.king_kinship(at)) == [0.25]
    assert vp.king_pairs_rule(g, np.nextafter(0.25, 1.0)).size == 0
    assert vp.king_pairs_rule(np.zeros((5, 4, 4), dtype=np.int64), 1e-9).size == 0   # het_sum = 0 everywhere


# ---- the decode, restated in numpy ------------------------------------------------------------------------------------------------
def decode_rows(rows, n):
    """What plink_bed_to_king_planes_kernel writes: five uint32 [V][ceil(n / 32)] bitset arrays from raw .bed rows, samples
    >= n masked in every plane."""
    v = rows.shape[0]
    words = (n + 31) // 32
    two = np.zeros((v, words * 32), dtype=np.uint8)
    for k in range(4):
        cols = np.arange(k, min(rows.shape[1] * 4, words * 32), 4)
        two[:, cols] = (rows[:, cols // 4] >> (2 * k)) & 3
    live = np.arange(words * 32) < n
    out = []
    for plane in ((two == 2), (two == 1), (two == 2) | (two == 1), (two == 0), (two == 3)):
        bits = (plane & live[None, :]).reshape(v, words, 32)
        out.append((bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32))
    return out


@pytest.mark.parametrize("n", [5, 63, 65, 130])
def test_the_decode_masks_the_padding_in_every_plane(vp, n):
    assert n % 4 != 0 and n % 32 != 0
    rng = np.random.default_rng(n)
    code = rng.integers(0, 4, size=(9, n)).astype(np.uint8)
    rows = K.bed_rows(code)
    assert rows.shape[1] == (n + 3) // 4 and (rows[:, -1] >> (2 * (n % 4))).max() == 0   # the padding codes are 00
    planes = decode_rows(rows, n)
    I = load_pkg("ingest")
    for got, want in zip(planes, vp.king_planes(code)):
        assert np.array_equal(got, I.pack_bits(want))
    assert sum(int(np.unpackbits(p.view(np.uint8)).sum()) for p in (planes[0], planes[1], planes[3], planes[4])) == 9 * n
    unmasked = decode_rows(np.concatenate([rows, np.zeros((9, 8), dtype=np.uint8)], axis=1), n)   # a wide pitch: the same bits
    for a, b in zip(planes, unmasked):
        assert np.array_equal(a, b)


# ---- the cohort -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,v", K.SIZES)
def test_the_king_cohort_discriminates_and_jaccard_does_not(vp, n, v):
    code = K.codes(n, v)
    assert len(K.planted_pairs(n)) == 10 and set(np.unique(code)) == {0, 1, 2, 3}
    lo, other = K.margins(vp, code)                                       # asserts the 5 % margins itself
    print("n = %d, v = %d: planted kinship >= %.3f, largest other %.3f" % (n, v, lo, other))
    assert (round(lo, 3), round(other, 3)) == K.KNOWN[n]
    pairs = vp.king_pairs_rule([K.gram(p) for p in vp.king_planes(code)], K.CUTOFF)
    assert [(int(p["i"]), int(p["j"])) for p in pairs] == K.planted_pairs(n)
    j_planted, j_other = K.jaccard_extremes(code)
    print("carrier Jaccard: smallest planted %.3f, largest other %.3f" % (j_planted, j_other))
    assert j_other > j_planted                                            # no --related-min-jaccard separates them


# ---- the CLI surface of both hosts: no engine attempted ---------------------------------------------------------------------------
BED = ["--input-path", "cohort.bed"]
ON = BED + ["--king-cutoff", "0.177"]
REFUSED = [
    (["--input-path", "cohort.vcf", "--king-cutoff", "0.177"], "--king-cutoff", "single .bed / .bim / .fam"),
    (["--input-path", "a.bed", "b.bed", "--king-cutoff", "0.177"], "--king-cutoff", "single .bed / .bim / .fam"),
    (ON + ["--min-allele-frequency", "0.1"], "--king-cutoff", "single .bed / .bim / .fam"),
    (ON + ["--gram", "implicit"], "--king-cutoff", "cannot take --gram implicit"),
    (ON + ["--layout", "strips"], "--king-cutoff", "cannot take --layout strips"),
    (ON + ["--gpus", "2"], "--king-cutoff", "cannot take --gpus 2"),
    (ON + ["--ld-window", "50"], "--king-cutoff", "cannot take --ld-window"),
    (ON + ["--related-min-jaccard", "0.5"], "--king-cutoff", "cannot take --related-min-jaccard"),
    (ON + ["--project-input-path", "other.bed"], "--king-cutoff", "cannot take --project-input-path"),
    (BED + ["--king-output-path", "pairs.tsv"], "--king-output-path", "needs --king-cutoff"),
    (BED + ["--king-max-pairs", "10"], "--king-max-pairs", "needs --king-cutoff"),
    (BED + ["--king-remove"], "--king-remove", "needs --king-cutoff"),
    (BED + ["--king-cutoff", "nan"], "--king-cutoff", "(0, 0.5]"),
    (BED + ["--king-cutoff", "0"], "--king-cutoff", "(0, 0.5]"),
    (BED + ["--king-cutoff", "0.51"], "--king-cutoff", "(0, 0.5]"),
    (BED + ["--king-cutoff", "-0.1"], "--king-cutoff", "(0, 0.5]"),
    (BED + ["--king-cutoff", "inf"], "--king-cutoff", "(0, 0.5]"),
    (ON + ["--king-max-pairs", "-1"], "--king-max-pairs", "must be >= 0"),
]
DRIVER_ONLY = [
    (ON + ["--no-stream"], "--king-cutoff", "cannot take --no-stream"),
    (ON + ["--parse-only"], "--king-cutoff", "cannot take --parse-only"),
    (ON + ["--plink-decode", "host"], "--king-cutoff", "cannot take --plink-decode host"),
]
NOT_A_NUMBER = [
    (BED + ["--king-cutoff", "abc"], "--king-cutoff takes a number", "argument --king-cutoff: invalid float value"),
    (ON + ["--king-max-pairs", "7x"], "--king-max-pairs takes an integer", "argument --king-max-pairs: invalid int value"),
]


def driver_message(res):
    return [line for line in res.stderr.splitlines() if line.startswith("VariantsPcaDriver: ")][-1]


@pytest.mark.parametrize("extra,flag,what", REFUSED)
def test_both_hosts_refuse_what_the_screen_cannot_serve_with_the_same_text(vp, extra, flag, what, capsys):
    """No file named here exists: a host that reads one before it refuses fails on the missing file instead."""
    res = K.run_driver(extra)
    assert res.returncode != 0 and flag in res.stderr and what in res.stderr, res.stderr
    assert "Matrix size" not in res.stdout and "pcoa_create" not in res.stderr
    with pytest.raises(SystemExit) as ei:                                 # in process: check_king_conf runs before a file is read
        vp.main(extra)
    assert str(ei.value) == driver_message(res)
    assert "Matrix size" not in capsys.readouterr().out


@pytest.mark.parametrize("extra,flag,what", DRIVER_ONLY)
def test_driver_refuses_its_own_three(extra, flag, what):
    res = K.run_driver(extra)
    assert res.returncode != 0 and flag in res.stderr and what in res.stderr, res.stderr
    assert "Matrix size" not in res.stdout and "pcoa_create" not in res.stderr


@pytest.mark.parametrize("extra,driver_says,python_says", NOT_A_NUMBER)
def test_both_hosts_refuse_a_value_that_is_no_number(vp, extra, driver_says, python_says, capsys):
    res = K.run_driver(extra)
    assert res.returncode != 0 and driver_says in res.stderr and "Matrix size" not in res.stdout, res.stderr
    with pytest.raises(SystemExit) as ei:
        vp.PcaConf(extra)
    assert ei.value.code != 0 and python_says in capsys.readouterr().err


def test_the_screen_is_off_by_default(vp):
    conf = vp.PcaConf([])
    assert conf.king_cutoff is None and conf.king_max_pairs == 1048576 and conf.king_remove is False
    assert conf.king_output_path is None
    vp.check_king_conf(conf)                                              # nothing to refuse
    conf = vp.PcaConf(BED + ["--king-cutoff", "0.0884", "--king-max-pairs", "99", "--king-remove", "--king-output-path", "p.tsv"])
    assert (conf.king_cutoff, conf.king_max_pairs, conf.king_remove, conf.king_output_path) == (0.0884, 99, True, "p.tsv")
    vp.check_king_conf(conf)
    vp.check_king_conf(vp.PcaConf(BED + ["--king-cutoff", "0.5"]))        # the closed end of (0, 0.5]
    for also in (["--missing-calls", "pairwise"], ["--similarity-measure", "jaccard"], ["--outlier-iterations", "2"]):
        vp.check_king_conf(vp.PcaConf(ON + also))                         # what --king-remove composes with
    usage = subprocess.run([K.driver_exe(), "--help"], stdout=subprocess.PIPE, universal_newlines=True).stdout
    for flag in ("--king-cutoff", "--king-output-path", "--king-max-pairs", "--king-remove"):
        assert flag in usage


def test_python_host_screen_over_a_stand_in_engine(vp, tmp_path):
    """screenKing with stand-ins: planes whose king_pairs is the numpy rule, an engine whose subset is numpy's.  The stderr
    line, the pair file, the kept cohort, the planes closed right after the screen, and the stops."""
    code = np.concatenate([threshold_codes(), np.zeros((40, 2), dtype=np.uint8)], axis=1)
    code[:, 3] = code[:, 1]                                               # sample 3 duplicates sample 1
    grams = grams_of(vp, code)
    closed = []

    class Planes(object):
        def king_pairs(self, x, capacity):
            v, h, _, _, _ = vp.king_counts(grams)
            pairs = vp.king_pairs_rule(grams, x)
            return pairs[:capacity], pairs.size, v, h

        def close(self):
            closed.append("planes")

    class Standin(object):
        def __init__(self, n):
            self.n = n

        def subset(self, keep):
            return Standin(len(keep))

        def timings(self):
            return {"gram_kernel_seconds": 0.25}

        def close(self):
            closed.append(self.n)

    ids = ["set-%d" % i for i in range(5)]
    names = dict((cid, K.name_of(i)) for i, cid in enumerate(ids))
    indexes = dict((cid, i) for i, cid in enumerate(ids))

    def run(args):
        del closed[:]
        with redirect_stdout(io.StringIO()):
            driver = vp.VariantsPcaDriver(vp.PcaConf(BED + args), indexes, names, [])
        err = io.StringIO()
        return driver, driver.screenKing(Standin(5), Planes(), err=err), err.getvalue()

    out = str(tmp_path / "pairs.tsv")
    driver, eng, err = run(["--king-cutoff", "0.25", "--king-output-path", out])
    assert err == "KING pairs: 3 at kinship >= 0.25; removed 0 sample(s)\n"
    assert eng.n == 5 and driver.kept is None and closed == ["planes"]
    assert open(out).read() == ("name_i\tname_j\thethet\tibs0\thet_sum\tkinship\nS0000\tS0001\t12\t2\t32\t0.25\n"
                                "S0000\tS0003\t12\t2\t32\t0.25\nS0001\tS0003\t16\t0\t32\t0.5\n")
    driver, eng, err = run(["--king-cutoff", "0.25", "--king-remove"])
    assert err == "KING pairs: 3 at kinship >= 0.25; removed 2 sample(s): S0001, S0003\n"
    assert eng.n == 3 and list(driver.kept) == [0, 2, 4] and closed == ["planes", 5] and driver.engine is eng
    assert driver.gram_seconds_before == 0.25
    driver, eng, err = run(["--king-cutoff", "0.3"])
    assert err == "KING pairs: 1 at kinship >= 0.3; removed 0 sample(s)\n"
    with pytest.raises(SystemExit) as ei:
        run(["--king-cutoff", "0.25", "--king-max-pairs", "1"])
    assert "3 pairs" in str(ei.value) and "--king-max-pairs" in str(ei.value) and "--king-cutoff" in str(ei.value)
    assert closed == ["planes"]                                           # also on the way out
    with pytest.raises(SystemExit) as ei:                                 # 3 of 5 left, three components need 4
        run(["--king-cutoff", "0.25", "--king-remove", "--num-pc", "3"])
    assert "--king-remove" in str(ei.value) and "--king-cutoff" in str(ei.value)


# ---- header and binding -----------------------------------------------------------------------------------------------------------
def test_the_king_entries_are_declared_exported_and_bound():
    L = load_pkg("_lib")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcoa.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+pcoa_accumulate_plink_bed_king\s*\(\s*pcoa_ctx\s*\*\s*const\s*\*\s*planes\s*,\s*const\s+uint8_t\s*\*\s*"
                     r"bed_rows\s*,\s*int64_t\s+n_variants\s*,\s*int64_t\s+row_bytes\s*,\s*int\s+is_device_ptr\s*\)\s*;", header)
    assert re.search(r"\bint\s+pcoa_king_pairs\s*\(\s*pcoa_ctx\s*\*\s*const\s*\*\s*planes\s*,\s*double\s+min_kinship\s*,\s*pcoa_king_pair\s*"
                     r"\*\s*out_pairs\s*,\s*int64_t\s+capacity\s*,\s*int64_t\s*\*\s*n_found_out\s*,\s*int64_t\s*\*\s*n_variants_out\s*,"
                     r"\s*int64_t\s*\*\s*out_het\s*\)\s*;", header)
    assert re.search(r"\bint\s+pcoa_get_king_stats\s*\(\s*pcoa_ctx\s*\*\s*plane0\s*,\s*pcoa_king_stats\s*\*\s*out\s*,\s*size_t\s+out_size\s*\)\s*;",
                     header)
    assert re.search(r"typedef\s+struct\s+pcoa_king_pair\s*\{\s*int32_t\s+i\s*,\s*j\s*;\s*int64_t\s+hethet\s*,\s*ibs0\s*,\s*het_sum\s*;\s*\}"
                     r"\s*pcoa_king_pair\s*;", header)
    for k, name in enumerate(("HET", "MISSING", "HET_OR_MISSING", "HOM_A1", "HOM_A2", "PLANES")):
        assert re.search(r"#define\s+PCOA_KING_%s\s+%d\b" % (name, k), header) and getattr(L, "PCOA_KING_" + name) == k
    lib = L.load()
    for name in ("pcoa_accumulate_plink_bed_king", "pcoa_king_pairs", "pcoa_get_king_stats"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    eng, vpm = load_pkg().PcoaEngine, load_pkg("variants_pca")
    for name in ("accumulate_plink_bed_king", "king_pairs", "king_stats"):
        assert hasattr(eng, name)
    assert [f[0] for f in L.PcoaKingStats._fields_] == ["king_seconds", "king_bytes", "king_calls"]
    assert ctypes.sizeof(L.PcoaKingPair) == 32 and vpm.KING_PAIR_DTYPE.itemsize == 32 and eng.KING_PAIR_DTYPE == vpm.KING_PAIR_DTYPE
    assert len(vpm.KING_PLANES) == L.PCOA_KING_PLANES
    assert "Extends:" in open(os.path.join(ROOT, "include", "pcoa.h")).read().split("KING-robust kinship screen")[1].split("#define")[0]


def test_struct_sizes_match_the_header(tmp_path):
    L = load_pkg("_lib")
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to compile the layout check"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pcoa.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pcoa_king_pair), offsetof(pcoa_king_pair, j),\n'
                   '         offsetof(pcoa_king_pair, hethet), offsetof(pcoa_king_pair, ibs0), offsetof(pcoa_king_pair, het_sum),\n'
                   '         sizeof(pcoa_king_stats), offsetof(pcoa_king_stats, king_bytes), sizeof(pcoa_timings));\n  return 0;\n}\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(t) for t in subprocess.check_output([exe]).split()]
    assert got == [32, 4, 8, 16, 24, ctypes.sizeof(L.PcoaKingStats), L.PcoaKingStats.king_bytes.offset, ctypes.sizeof(L.PcoaTimings)]
    assert (L.PcoaKingPair.j.offset, L.PcoaKingPair.hethet.offset, L.PcoaKingPair.ibs0.offset, L.PcoaKingPair.het_sum.offset) == (4, 8, 16, 24)


def test_a_null_planes_array_is_refused():
    L = load_pkg("_lib")
    lib = L.load()
    found = ctypes.c_int64(-5)
    assert lib.pcoa_king_pairs(None, 0.177, None, 0, ctypes.byref(found), None, None) == L.PCOA_ERR_INVALID_ARG
    assert found.value == -5 and b"pcoa_king_pairs: planes is NULL" in lib.pcoa_last_error(None)
    assert lib.pcoa_accumulate_plink_bed_king(None, None, 0, 1, 0) == L.PCOA_ERR_INVALID_ARG
    assert b"pcoa_accumulate_plink_bed_king: planes is NULL" in lib.pcoa_last_error(None)
    empty = (ctypes.c_void_p * L.PCOA_KING_PLANES)()
    assert lib.pcoa_king_pairs(empty, 0.177, None, 0, ctypes.byref(found), None, None) == L.PCOA_ERR_INVALID_ARG
    assert found.value == -5 and b"planes[0] (PCOA_KING_HET) is NULL" in lib.pcoa_last_error(None)
    assert lib.pcoa_get_king_stats(None, None, 0) == L.PCOA_ERR_INVALID_ARG


# ---- the kernels: no scratch, resources recorded ----------------------------------------------------------------------------------
KERNELS = (("plink_bed_to_king_planes_kernel", 1), ("king_diag_kernel", 1), ("king_count_kernel", 2), ("king_write_kernel", 2))
RECORD = os.path.join(ROOT, "profiles", "r16a_king_kernel_resources.txt")
FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", r"ScratchSize \[bytes/lane\]", r"Occupancy \[waves/SIMD\]", r"LDS Size \[bytes/block\]")


@pytest.fixture(scope="module")
def resource_report():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"      # (what built the library; without it these tests fail)
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                              "-I", csrc, "-c", os.path.join(csrc, "king.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True)
    assert res.returncode == 0, res.stdout[-2000:]
    return res.stdout


def _resources(text):
    """{kernel: {field: value}} from the compiler's remarks or from the record (the same lines without the remark's prefix)."""
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        for f in FIELDS:
            m = re.search(f + r": (\d+)", line)
            if m and name:
                out[name][f] = int(m.group(1))
    return out


def test_king_kernels_do_not_spill_to_scratch(resource_report):
    """king.hip keeps a lane's four h_j and hm_j and two rows of FIVE matrices in registers; hipcc reports at compile time
    whether any of it went to scratch."""
    names = re.findall(r"Function Name: (\S+)", resource_report)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", resource_report)]
    assert len(names) == len(scratch) == 6            # decode, diagonal, count and write x (16-byte | dword loads)
    for kernel, count in KERNELS:
        assert sum(kernel in nm for nm in names) == count, names
    assert scratch == [0] * 6


def test_the_resource_record_is_current(resource_report):
    now = _resources(resource_report)
    recorded = _resources(open(RECORD).read())
    assert len(now) == 6 and all(len(v) == len(FIELDS) for v in now.values())
    assert recorded == now, "profiles/r16a_king_kernel_resources.txt is not what hipcc reports for king.hip today"


def test_no_existing_kernel_unit_was_touched():
    """The new kernels live in a unit of their own: pairs.hip and complete.hip have no kernel of this family."""
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    for unit in ("pairs.hip", "complete.hip", "gram_aux.hip"):
        assert "king" not in open(os.path.join(csrc, unit)).read().lower()

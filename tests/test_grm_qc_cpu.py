"""CPU tests of the variant and sample QC of a GRM engine: the exact statement of the Hardy-Weinberg test in
tests/grm_qc_cohort.py against brute-force enumeration, the ABI surface, the command-line surface of both hosts, which must
refuse the flags without --grm before any engine exists, the compile-time resources of the kernels, and that the cohorts of
tests/test_gpu_grm_qc.py tell the right rule from two plausible wrong ones."""
import itertools
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import grm_qc_cohort as Q
from conftest import ROOT, load_golden, load_pkg, write_golden_plink
from test_grm_cpu import edge_rows, random_codes, spec_grm_counts


# ---- the exact test against enumeration ---------------------------------------------------------------------------------------
def brute_het_distribution(n, rare):
    """{k: arrangements}: the 2n allele slots of n samples with `rare` of them holding the rarer allele, every arrangement equally
    likely; k = the samples that hold one copy."""
    dist = {}
    for slots in itertools.combinations(range(2 * n), rare):
        per = [0] * n
        for s in slots:
            per[s // 2] += 1
        k = sum(1 for c in per if c == 1)
        dist[k] = dist.get(k, 0) + 1
    return dist


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_spec_hwe_exact_equals_enumeration(n):
    for rare in range(0, n + 1):
        dist = brute_het_distribution(n, rare)
        total = sum(dist.values())
        for h in dist:
            hom_rare = (rare - h) // 2
            want = Fraction(sum(c for c in dist.values() if c <= dist[h]), total)
            for o in (hom_rare, n - h - hom_rare):           # the rarer allele as the non-reference one, and the other way round
                assert Q.spec_hwe_exact(n, h, o) == want, (n, h, o)
    assert Q.spec_hwe_exact(0, 0, 0) == 1 and Q.spec_hwe_exact(n, 0, 0) == 1 and Q.spec_hwe_exact(n, 0, n) == 1


def test_the_tie_rule_counts_exact_ties_and_nothing_else():
    # n = 4, R = 4: P(0) : P(2) : P(4) = 3 : 24 : 8 -- no tie; n = 3, R = 3: P(1) : P(3) = 9 : ... check by enumeration instead
    found = 0
    for n in range(2, 9):
        for rare in range(2, n + 1):
            dist = brute_het_distribution(n, rare)
            ks = sorted(dist)
            for a, b in itertools.combinations(ks, 2):
                if dist[a] == dist[b]:
                    found += 1
                    hom = (rare - a) // 2
                    p = Q.spec_hwe_exact(n, a, hom)
                    assert p >= Fraction(dist[a] + dist[b], sum(dist.values()))
    assert found > 0
    assert Q.TIE == 1 + Fraction(1, 2 ** 24)


# ---- the surface ------------------------------------------------------------------------------------------------------------------
QC_SYMBOLS = ["pcoa_grm_set_variant_filters", "pcoa_grm_get_variant_filters", "pcoa_grm_hwe", "pcoa_grm_sample_counts",
              "pcoa_get_grm_qc_stats"]


def test_header_declares_the_entries_and_states_the_rule():
    lib = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "pcoa.h")).read()
    for sym in QC_SYMBOLS:
        assert sym in lib.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % sym, header), sym
    declared = set(re.findall(r"^(?:int|void|const char\*)\s+(pcoa_\w+)\(", header, flags=re.M))
    assert set(lib.EXPORTED_SYMBOLS) == declared
    for text in ("(double)(N - n_v) <= max_missing * (double)N", "p_v >= hwe_min_p", "P(k) <= P(h) * (1 + 2^-24)",
                 "p_v  = 1.0 when n = 0 or R = 0", "#define PCOA_GRM_ROWS_ALL  0", "#define PCOA_GRM_ROWS_USED 1",
                 "typedef struct pcoa_grm_qc_stats", "Not built: plink's inbreeding coefficient F, mid-p, per-population HWE"):
        assert text in header, text
    assert (lib.PCOA_GRM_ROWS_ALL, lib.PCOA_GRM_ROWS_USED) == (0, 1)
    fields = [f[0] for f in lib.PcoaGrmQcStats._fields_]
    body = re.search(r"typedef struct pcoa_grm_qc_stats \{(.*?)\} pcoa_grm_qc_stats;", header, flags=re.S).group(1)
    assert re.findall(r"(?:double|int64_t) (\w+);", body) == fields
    if os.path.exists(lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
        exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
        for sym in QC_SYMBOLS:
            assert sym in exported, sym


def test_qc_kernels_do_not_spill_to_scratch():
    import shutil
    import tempfile
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                              "-I", csrc, "-c", os.path.join(csrc, "grm_qc.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True)
    assert res.returncode == 0, res.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", res.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stdout)]
    assert len(names) == len(scratch)
    for family in ("grm_hwe_kernel", "grm_qc_fails_kernel", "grm_sample_counts_kernel", "grm_sample_counts_finish_kernel"):
        assert any(family in nm for nm in names), "no %s in grm_qc.hip" % family
    for nm, sc in zip(names, scratch):
        assert sc == 0, "%s spills %d bytes/lane" % (nm, sc)


# ---- the hosts ------------------------------------------------------------------------------------------------------------------
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
def bed(tmp_path_factory):
    d = tmp_path_factory.mktemp("grmqccli")
    write_golden_plink(load_golden("kat5"), str(d / "kat5"))
    return str(d / "kat5.bed"), str(d / "out.tsv")


NEED_GRM = [(["--grm-geno", "0.1"], "--grm-geno"), (["--grm-hwe", "1e-6"], "--grm-hwe"), (["--grm-mind", "0.1"], "--grm-mind"),
            (["--grm-variant-qc-output-path", "@out"], "--grm-variant-qc-output-path"),
            (["--grm-sample-qc-output-path", "@out"], "--grm-sample-qc-output-path")]


@pytest.mark.parametrize("extra,flag", NEED_GRM)
def test_both_hosts_refuse_the_flags_without_grm_before_an_engine_exists(bed, extra, flag):
    args = ["--input-path", bed[0]] + [bed[1] if a == "@out" else a for a in extra]
    for run in (_run_driver, _run_python):
        res = run(args)
        assert res.returncode != 0 and flag in res.stderr and "needs --grm" in res.stderr, res.stderr
        assert "Matrix size" not in res.stdout and "pcoa error" not in res.stderr and "pcoa_create" not in res.stderr
    assert not os.path.exists(bed[1])


@pytest.mark.parametrize("extra", [["--grm-geno", "1.5"], ["--grm-geno", "nan"], ["--grm-hwe", "1"], ["--grm-hwe", "-0.1"],
                                   ["--grm-mind", "-1"], ["--grm-mind", "x"]])
def test_both_hosts_refuse_values_out_of_range(bed, extra):
    for run in (_run_driver, _run_python):
        res = run(["--input-path", bed[0], "--grm"] + extra)
        assert res.returncode != 0 and extra[0] in res.stderr, res.stderr
        assert "Matrix size" not in res.stdout and "pcoa error" not in res.stderr and "pcoa_create" not in res.stderr


def test_the_flags_parse():
    vp = load_pkg("variants_pca")
    conf = vp.PcaConf(["--grm", "--grm-geno", "0.1", "--grm-hwe", "1e-6", "--grm-mind", "0.2"])
    assert (conf.grm_geno, conf.grm_hwe, conf.grm_mind) == (0.1, 1e-6, 0.2)
    conf = vp.PcaConf(["--grm"])
    assert conf.grm_geno is None and conf.grm_hwe is None and conf.grm_mind is None


# ---- the cohorts of the GPU tests tell the rules apart ----------------------------------------------------------------------------
def test_the_wrong_rules_differ_from_the_right_one_on_the_test_cohorts():
    n, v, maf, geno, hwe = 96, 120, 0.05, 0.125, 1e-3           # N_F, V_F, ... of tests/test_gpu_grm_qc.py
    codes = Q.filter_cohort(n, v, 21)
    counts = spec_grm_counts(codes, False)
    right = Q.spec_used(counts, n, maf, geno, hwe)
    # < in place of <= in the missing test loses the rows whose missing share equals max_missing
    wrong = Q.spec_used(counts, n, maf, geno, hwe, missing_lt=True)
    assert wrong.sum() < right.sum() and not np.any(wrong & ~right)
    assert all(n - counts[r, 0] == n // 8 for r in np.flatnonzero(right & ~wrong))
    # the one-sided tail keeps the rows with an excess of heterozygotes
    thr = Fraction(hwe)
    two = np.array([p < thr for p in Q.hwe_of_counts(counts)])
    one = np.array([Q.wrong_hwe_one_sided(int(a), int(b), int(c)) < thr for a, b, c in counts])
    assert two.sum() >= 6 and one.sum() < two.sum() and np.any(two & ~one)
    # and its p-values differ beyond the bound at most rows of a random cohort
    rc = spec_grm_counts(edge_rows(random_codes(np.random.default_rng(1000 + 65 + 70), 70, 65)), False)
    differ = sum(1 for a, b, c in rc
                 if abs(Q.wrong_hwe_one_sided(int(a), int(b), int(c)) - Q.spec_hwe_exact(int(a), int(b), int(c)))
                 > Q.hwe_bound(65) * Q.spec_hwe_exact(int(a), int(b), int(c)))
    assert differ > 35


def test_the_bound_and_the_statement_of_the_counts():
    assert Q.hwe_bound(4096) == Fraction(4 * 4096 + 32, 2 ** 53)
    assert Q.hwe_within(0.0, Fraction(1, 2 ** 950), 100) and not Q.hwe_within(1e-200, Fraction(1, 2 ** 950), 100)
    assert Q.hwe_within(0.5, Fraction(1, 2), 100) and not Q.hwe_within(0.5 + 1e-12, Fraction(1, 2), 100)
    codes = edge_rows(random_codes(np.random.default_rng(3), 40, 33))
    sc = Q.spec_sample_counts(codes, True)
    assert sc[1].tolist() == [0, 0, 0] and sc.shape == (33, 3)
    assert sc[:, 0].sum() == (codes != 1).sum() and sc[:, 2].sum() == (codes == 3).sum()
    rows = np.zeros(40, dtype=bool)
    rows[5:9] = True
    assert np.array_equal(Q.spec_sample_counts(codes, False, rows), Q.spec_sample_counts(codes[5:9], False))
    assert Q.spec_fails(spec_grm_counts(codes, False), 33)[1:] == (0, 0)

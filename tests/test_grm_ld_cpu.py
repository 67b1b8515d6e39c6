"""CPU tests of the LD prune of the GRM store (pcoa_grm_ld_*, --grm-ld-window): the popcount identities the band kernel rests on,
the condition under which the GPU shapes prove something (a rule that ignores missing calls and a pass that is not greedy give
another mask there, and enough in-window pairs exceed), the banded twin of the rule, the ABI surface, the kernels' resources and
the command-line surface of both hosts, which refuse a wrong combination before any device work."""
import os
import re
import subprocess

import numpy as np
import pytest

import grm_ld_cohort as C
from conftest import ROOT, load_pkg
from test_grm_cpu import _run_driver, _run_python, inputs  # noqa: F401  (inputs: the fixture with a PLINK fileset and a VCF)


# ---- the popcount identities ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, 47, 64, 130, 1025])
def test_popcount_identities_equal_the_direct_sums(n):
    """N % 16 != 0 leaves padding slots in the last word, and the pitch (a multiple of 4 words) whole padding words: all 01."""
    g = C.cohort(n, 40, 500 + n, miss=0.2)
    words = C.store_words(g)
    assert words.shape == (40, ((n + 15) // 16 + 3) // 4 * 4)
    assert np.all(words[:, (n + 15) // 16:] == C.K_LO)
    seen = 0
    for u in range(40):
        for v in range(u + 1, min(u + 8, 40)):
            want = C.direct_sums(g[u], g[v])
            assert C.popcount_sums(words[u], words[v]) == want, (n, u, v)
            assert C.popcount_sums(words[v], words[u]) == (want[0], want[2], want[1], want[4], want[3], want[5])
            seen += want[5] > 0
    assert seen > 0 or n == 1


# ---- the shapes of the GPU tests prove something ----------------------------------------------------------------------------
@pytest.mark.parametrize("n,v,w,t", C.SHAPES)
def test_wrong_rules_give_other_masks_on_the_gpu_shapes(n, v, w, t):
    g = C.cohort(n, v, 100 + n)
    cand = C.candidates(g)
    ex = C.exceeds_matrix(g, t)
    keep = C.greedy(ex, cand, w)
    no_missing = C.greedy(C.exceeds_matrix(g, t, ignore_missing=True), cand, w)
    non_greedy = C.greedy(ex, cand, w, non_greedy=True)
    pairs = int((ex & C.window_mask(v, w)).sum())
    print("N = %d: %d rows differ without the missing calls, %d without the greedy pass; %d in-window pairs exceed"
          % (n, (keep != no_missing).sum(), (keep != non_greedy).sum(), pairs))
    assert (keep != no_missing).any() and (keep != non_greedy).any()
    assert pairs >= 100
    # rows 3 (monomorphic) and 5 (never called) are no candidates; row 9 repeats row 8
    assert not cand[3] and not cand[5] and not keep[3] and not keep[5]
    assert ex[8, 9] or not cand[8]


@pytest.mark.parametrize("n,v,w,t", C.SHAPES[:4])
def test_banded_rule_equals_the_matrix_rule(n, v, w, t):
    g = C.cohort(n, v, 100 + n)
    ex, band = C.exceeds_matrix(g, t), C.exceeds_band(g, w, t)
    for d in (1, w):
        if d < v:
            assert np.array_equal(band[d:, d - 1], np.diagonal(ex, d))
    for breaks, maf in (((), 0.0), ((1, v // 2, v - 1), 0.0), ((w, w + 1), 0.1)):
        cand = C.candidates(g, maf)
        keep = C.greedy(ex, cand, w, breaks)
        assert np.array_equal(C.greedy_band(band, cand, w, breaks), keep)
        got = C.rule(g, w, t, breaks, maf)
        assert np.array_equal(got[0], keep) and got[1:] == (int(cand.sum()), int(keep.sum()), C.window_pairs(v, w, breaks))
    assert C.window_pairs(v, w) == int(C.window_mask(v, w).sum())
    assert C.window_pairs(v, w, (1, v // 2)) == int(C.window_mask(v, w, (1, v // 2)).sum())


# ---- the ABI surface ----------------------------------------------------------------------------------------------------------
GRM_LD_SYMBOLS = ["pcoa_grm_ld_prune", "pcoa_grm_ld_mask", "pcoa_grm_ld_clear", "pcoa_get_grm_ld_stats"]


def test_grm_ld_symbols_are_declared_bound_and_exported():
    lib = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "pcoa.h")).read()
    for sym in GRM_LD_SYMBOLS:
        assert sym in lib.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % sym, header), sym
    block = header[header.index("pcoa_create_grm: a ctx that holds"):header.index("int pcoa_create_grm(")]
    assert "LD pruning in front of the store" not in block and "pcoa_grm_ld_prune" in block
    assert [f[0] for f in lib.PcoaGrmLdStats._fields_] == re.findall(r"^\s+(?:int64_t|double) (grm_ld_\w+);", header, flags=re.M)
    if os.path.exists(lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
        exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
        for sym in GRM_LD_SYMBOLS:
            assert sym in exported, sym


def test_grm_ld_kernels_do_not_spill_to_scratch():
    """The band kernel holds 48 int32 accumulators per lane; an array that lands in scratch turns every popcount into a memory
    access.  hipcc reports it at compile time."""
    import shutil
    import tempfile
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                              "-I", csrc, "-c", os.path.join(csrc, "grm_ld.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True)
    assert res.returncode == 0, res.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", res.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stdout)]
    assert len(names) == len(scratch)
    for family in ("grm_ld_band_kernel", "grm_ld_reach_kernel"):
        assert any(family in nm for nm in names), "no %s in grm_ld.hip" % family
    for nm, sc in zip(names, scratch):
        assert sc == 0, "%s spills %d bytes/lane" % (nm, sc)


# ---- the hosts ----------------------------------------------------------------------------------------------------------------
# (arguments behind --input-path BED, with or without --grm; the two flags the message must name)
REFUSED = [
    (["--grm-ld-window", "50"], "--grm-ld-window", "--grm "),
    (["--grm-ld-r2", "0.3"], "--grm-ld-r2", "--grm "),
    (["--grm-ld-output-path", "@out"], "--grm-ld-output-path", "--grm "),
    (["--grm", "--grm-ld-r2", "0.3"], "--grm-ld-r2", "--grm-ld-window"),
    (["--grm", "--grm-ld-output-path", "@out"], "--grm-ld-output-path", "--grm-ld-window"),
    (["--grm", "--grm-ld-window", "1025"], "--grm-ld-window", "--grm"),
    (["--grm", "--grm-ld-window", "-1"], "--grm-ld-window", "--grm"),
    (["--grm", "--grm-ld-window", "50", "--grm-ld-r2", "1.5"], "--grm-ld-r2", "--grm-ld-window"),
    (["--grm", "--grm-ld-window", "50", "--grm-ld-r2", "-0.1"], "--grm-ld-r2", "--grm-ld-window"),
    (["--grm", "--ld-window", "50"], "ld-window", "--grm-ld-window"),
]


@pytest.mark.parametrize("run", [_run_driver, _run_python], ids=["cpp", "py"])
@pytest.mark.parametrize("extra,first,second", REFUSED)
def test_hosts_refuse_before_any_device_work(inputs, run, extra, first, second):  # noqa: F811
    out = os.path.join(inputs["dir"], "mask.tsv")
    res = run(["--input-path", inputs["bed"]] + [out if a == "@out" else a for a in extra])
    assert res.returncode != 0 and first in res.stderr and second in res.stderr, res.stderr
    assert "Matrix size" not in res.stdout and "pcoa_create" not in res.stderr and "pcoa error" not in res.stderr
    assert not os.path.exists(out)


def test_grm_ld_is_off_by_default():
    vp = load_pkg("variants_pca")
    conf = vp.PcaConf([])
    assert conf.grm_ld_window == 0 and conf.grm_ld_r2 is None and conf.grm_ld_output_path is None
    conf = vp.PcaConf(["--grm", "--grm-ld-window", "50"])
    assert conf.grm_ld_window == 50 and vp.LD_DEFAULT_R2 == 0.2

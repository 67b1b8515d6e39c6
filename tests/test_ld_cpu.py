"""CPU tests of the LD pruner: the numpy statement of the rule satisfies its two postconditions by direct evaluation and is not
what a non-greedy pass gives, the hosts refuse what --ld-window cannot serve before any device work, the --ld-output-path line
format, and the kernels' resources.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_pkg
from ld_cohort import exceeds_matrix, ld_cohort, ld_pairs, ld_rule, ld_rule_banded, ld_rule_nongreedy
from test_operator_cpu import _run_driver, _run_python

SHAPES = [(33, 300, 1, 0.5), (70, 700, 7, 0.2), (130, 1000, 64, 0.5), (260, 1000, 65, 0.8), (2504, 600, 50, 0.2),
          (4100, 300, 200, 0.5), (600, 131, 9, 0.3)]


@pytest.mark.parametrize("n,v,w,t", SHAPES)
def test_the_rule_satisfies_its_postconditions_and_is_greedy(n, v, w, t):
    x = ld_cohort(n, v, 1000 + n)
    a = x.sum(axis=1)
    assert a[3] == 0 and a[5] == n and np.array_equal(x[8], x[9])
    keep = ld_rule(x, w, t)
    ex = exceeds_matrix(x, t)
    in_window = np.zeros((v, v), dtype=bool)            # [v, u]: u is one of the w rows in front of v
    for d in range(1, w + 1):
        in_window[np.arange(d, v), np.arange(0, v - d)] = True
    assert np.array_equal(ex, ex.T)
    # no two kept variants within W exceed t
    assert not (ex & in_window & keep[:, None] & keep[None, :]).any()
    # every removed polymorphic variant has a kept in-window predecessor that exceeds t
    poly = (a > 0) & (a < n)
    blocked = (ex & in_window & keep[None, :]).any(axis=1)
    assert np.array_equal(~keep & poly, blocked & poly) and not keep[~poly].any()
    assert in_window.sum() == ld_pairs(v, w)
    # the cohort tells the greedy pass from a shortcut: exceeding pairs whose earlier member was itself removed
    stale = int((ex & in_window & ~keep[None, :] & poly[None, :]).sum())
    other = ld_rule_nongreedy(x, w, t)
    print("n=%d V=%d W=%d t=%g: kept %d, %d exceeding pairs with a removed earlier member, non-greedy differs in %d rows"
          % (n, v, w, t, keep.sum(), stale, (other != keep).sum()))
    assert stale > 0 and not np.array_equal(other, keep)
    assert 0.25 * v < keep.sum() < 0.75 * v


def test_a_break_starts_a_new_window():
    x = ld_cohort(70, 200, 5)
    whole = ld_rule(x, 7, 0.2)
    for cut in (1, 50, 199):
        assert np.array_equal(ld_rule(x, 7, 0.2, breaks=[cut]), np.concatenate([ld_rule(x[:cut], 7, 0.2), ld_rule(x[cut:], 7, 0.2)]))
    assert np.array_equal(ld_rule(x, 7, 0.2, breaks=[0]), whole)


@pytest.mark.parametrize("breaks", [(), (1, 50, 299, 300, 599)])
@pytest.mark.parametrize("t", [0.1, 0.5])
@pytest.mark.parametrize("w", [1, 5, 50])
def test_the_banded_rule_is_the_rule(w, t, breaks):
    """ld_rule_banded (the reference of the multi-chunk GPU tests, where a V x V matrix cannot be built) against ld_rule."""
    x = ld_cohort(70, 600, 77)
    keep = ld_rule(x, w, t, breaks=breaks)
    assert 0 < keep.sum() < 600
    assert np.array_equal(ld_rule_banded(x, w, t, breaks=breaks), keep)


# ---- host logic -------------------------------------------------------------------------------------------------------------
FLAG = "--ld-window"
# (extra arguments, what the message names, whether --gram implicit refuses the same thing first by its own rule)
REFUSED = [
    (["--gpus", "2"], "--gpus", True),
    (["--layout", "strips"], "--layout strips", True),
    (["--project-input-path", "other.vcf"], "--project-input-path", True),
    (["--ld-window", "0", "--ld-output-path", "mask.tsv"], "--ld-output-path", False),
    (["--ld-window", "0", "--ld-r2", "0.5"], "--ld-r2", False),
    (["--ld-window", "1025"], "1025", False),
    (["--ld-window", "-1"], "-1", False),
    (["--ld-r2", "1.5"], "--ld-r2", False),
    (["--ld-r2", "-0.1"], "--ld-r2", False),
    (["--ld-r2", "nan"], "--ld-r2", False),
]


@pytest.mark.parametrize("gram", ["stored", "implicit"])
@pytest.mark.parametrize("extra,what,implicit_first", REFUSED)
def test_both_hosts_refuse_before_any_device_work(extra, what, implicit_first, gram, tmp_path):
    """The input does not exist: a host that got as far as reading it, or as creating an engine, fails differently."""
    args = ["--input-path", str(tmp_path / "absent.bed"), "--gram", gram, FLAG, "5"] + extra     # (a later --ld-window wins)
    for run in (_run_driver, _run_python):
        res = run(args)
        assert res.returncode != 0, res.stdout
        assert "VariantsPcaDriver:" in res.stderr and "absent" not in res.stderr, res.stderr
        if gram == "implicit" and implicit_first:      # either refusal names its flag
            assert FLAG in res.stderr or "--gram implicit" in res.stderr, res.stderr
        else:
            assert "--ld-" in res.stderr and what in res.stderr, res.stderr


def test_both_hosts_refuse_more_than_one_input_set(tmp_path):
    args = ["--input-path", str(tmp_path / "a.vcf"), str(tmp_path / "b.vcf"), FLAG, "5"]
    for run in (_run_driver, _run_python):
        res = run(args)
        assert res.returncode != 0 and FLAG in res.stderr and "one input set" in res.stderr, res.stderr


def test_mask_file_format(tmp_path):
    vp = load_pkg("variants_pca")
    meta = [("17", 41196312, "rs1"), ("17", 41196319, "."), ("2", 7, "id;with,marks")]
    path = str(tmp_path / "mask.tsv")
    vp.write_ld_mask(path, meta, np.array([True, False, True]))
    assert open(path).read() == "0\t17\t41196312\trs1\t1\n1\t17\t41196319\t.\t0\n2\t2\t7\tid;with,marks\t1\n"
    vp.write_ld_mask(path, None, [0, 1])                 # an input without variant records
    assert open(path).read() == "0\t.\t.\t.\t0\n1\t.\t.\t.\t1\n"
    with pytest.raises(RuntimeError):
        vp.write_ld_mask(path, meta[:2], [1, 1, 1])


def test_the_binding_declares_every_call_of_the_header_block():
    L = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "pcoa.h")).read()
    for name in ("pcoa_ld_begin", "pcoa_ld_bits", "pcoa_ld_plink_bed", "pcoa_ld_break", "pcoa_ld_end", "pcoa_get_ld_stats"):
        assert ("int %s(" % name) in header and name in L.EXPORTED_SYMBOLS
    assert "#define PCOA_LD_MAX_WINDOW %d\n" % L.PCOA_LD_MAX_WINDOW in header and L.PCOA_LD_ACCUMULATE == 1
    assert load_pkg("variants_pca").LD_MAX_WINDOW == L.PCOA_LD_MAX_WINDOW


# ---- the kernels' resources ---------------------------------------------------------------------------------------------------
def test_no_ld_kernel_uses_scratch_and_the_record_is_current():
    """The five kernels of ld.hip compile for gfx950 without scratch, and profiles/r14a_ld_kernel_resources.txt lists each."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import tempfile
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                              "-c", os.path.join(csrc, "ld.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True)
    assert res.returncode == 0, res.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", res.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stdout)]
    assert len(names) == 5 and len(scratch) == 5
    for kernel in ("ld_count_kernel", "ld_band_kernel", "ld_resolve_kernel", "ld_scan_kernel", "ld_gather_kernel"):
        assert sum(kernel in nm for nm in names) == 1, kernel
    assert scratch == [0] * 5
    record = open(os.path.join(ROOT, "profiles", "r14a_ld_kernel_resources.txt")).read()
    for nm in names:
        assert nm in record, nm

"""CPU tests of --project-input-path (no GPU): the argument parsing and the refusals of both hosts, which must come before any
file is read or any engine exists, and the ABI surface of pcoa_project."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT, load_golden, load_pkg, write_golden_plink, write_golden_vcf


def _exe():
    exe = os.path.join(ROOT, "spark-examples_amd", "variants_pca_driver")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "spark-examples_amd", "host")])
    return exe


SCRIPT = os.path.join(ROOT, "spark-examples_amd", "variants_pca.py")


def _both(args):
    """(compiled host, Python host) results of the same command line."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")   # nothing here may need a device
    c = subprocess.run([_exe()] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120, env=env)
    p = subprocess.run([sys.executable, SCRIPT] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       timeout=120, env=env)
    return c, p


@pytest.fixture(scope="module")
def vcfs(tmp_path_factory):
    d = tmp_path_factory.mktemp("proj")
    g = load_golden("pops40")
    ref, new = str(d / "panel.vcf"), str(d / "study.vcf")
    write_golden_vcf(g, ref)
    write_golden_vcf(g, new)
    write_golden_plink(g, str(d / "panel_plink"))
    return {"ref": ref, "new": new, "same_stem": str(d / "sub" / "panel.vcf"), "plink": str(d / "panel_plink.bed"),
            "npz": os.path.join(ROOT, "tests", "golden", "pops40.npz")}


@pytest.mark.parametrize("extra, words", [
    (["--gpus", "2"], "--gpus 2"),
    (["--layout", "strips"], "--layout strips"),
])
def test_both_hosts_refuse_what_projection_cannot_serve(vcfs, extra, words):
    c, p = _both(["--input-path", vcfs["ref"], "--project-input-path", vcfs["new"]] + extra)
    for r in (c, p):
        assert r.returncode != 0 and "--project-input-path" in r.stderr and words in r.stderr, r.stderr[-2000:]
        assert "Matrix size" not in r.stdout   # refused before any input was read


def test_compiled_host_refuses_carrier_lists(vcfs):
    c, _ = _both(["--input-path", vcfs["ref"], "--project-input-path", vcfs["new"], "--carrier-format", "lists"])
    assert c.returncode == 2 and "--carrier-format lists" in c.stderr and "Matrix size" not in c.stdout


@pytest.mark.parametrize("side", ["reference", "projected"])
def test_both_hosts_refuse_non_vcf_inputs_on_either_side(vcfs, side):
    for other in ("plink", "npz"):
        if other == "npz" and side == "reference":
            args = ["--input-path", vcfs["npz"], "--project-input-path", vcfs["new"]]
        elif other == "npz":
            args = ["--input-path", vcfs["ref"], "--project-input-path", vcfs["npz"]]
        elif side == "reference":
            args = ["--input-path", vcfs["plink"], "--project-input-path", vcfs["new"]]
        else:
            args = ["--input-path", vcfs["ref"], "--project-input-path", vcfs["plink"]]
        c, p = _both(args)
        for host, r in (("compiled", c), ("python", p)):
            if host == "compiled" and other == "npz":
                continue   # the compiled host reads an .npz as what it claims to be; only PLINK is a different kind of input there
            assert r.returncode != 0 and "VCF inputs on both sides" in r.stderr, (host, other, r.stderr[-2000:])
            assert "Matrix size" not in r.stdout


def test_both_hosts_refuse_a_callset_id_collision(vcfs):
    os.makedirs(os.path.dirname(vcfs["same_stem"]), exist_ok=True)
    write_golden_vcf(load_golden("pops40"), vcfs["same_stem"])
    c, p = _both(["--input-path", vcfs["ref"], "--project-input-path", vcfs["same_stem"]])
    for r in (c, p):
        assert r.returncode != 0 and "callset-id collision" in r.stderr and "'panel'" in r.stderr, r.stderr[-2000:]
        assert "Matrix size" not in r.stdout


def test_project_input_path_needs_a_file():
    c, p = _both(["--input-path", "x.vcf", "--project-input-path"])
    assert c.returncode == 2 and "--project-input-path needs at least one file" in c.stderr
    assert p.returncode == 2 and "--project-input-path" in p.stderr   # argparse: nargs="+"


def test_help_names_the_flag_on_both_hosts():
    c, p = _both(["--help"])
    for r in (c, p):
        assert r.returncode == 0 and "--project-input-path" in r.stdout, r.stdout[-2000:]


def test_python_host_parses_the_flag_as_a_list():
    vp = load_pkg("variants_pca")
    conf = vp.PcaConf(["--input-path", "a.vcf", "--project-input-path", "b.vcf", "c.vcf.gz"])
    assert conf.project_input_path == ["b.vcf", "c.vcf.gz"] and conf.inputPath == ["a.vcf"]
    assert vp.PcaConf(["--input-path", "a.vcf"]).project_input_path is None


def test_pcoa_project_is_bound_and_refuses_null_engines():
    L = load_pkg("_lib")
    assert "pcoa_project" in L.EXPORTED_SYMBOLS
    lib = L.load()
    rc = lib.pcoa_project(None, None, 2, None, None, None)
    assert rc == L.PCOA_ERR_INVALID_ARG

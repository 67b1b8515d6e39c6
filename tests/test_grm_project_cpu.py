"""CPU tests of the SNP weights and the projection of new samples on a GRM engine (pcoa_grm_weights, pcoa_grm_project,
--grm-weights-output-path, --grm-project-path): the numpy statement of what they compute (imported by
tests/test_gpu_grm_project.py), the identities it rests on, the ABI surface, the command-line surface of both hosts, which must
refuse a study fileset that does not match the panel before any engine exists, and the compile-time resource check of the
kernels of grm_multi.hip.  The spec of K itself is test_grm_cpu.py's."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden, load_pkg, write_golden_plink, write_golden_vcf
from test_grm_cpu import _run_driver, _run_python, balding_nichols, dense_k, dosage, exact_cohort, pack_bed, random_codes, \
    spec_grm_counts, spec_grm_weights


# ---- the spec (include/pcoa.h, "SNP weights of the axes of K") --------------------------------------------------------------
# comps: [N][k] (what compute(k) returns), lam: [k].  The panel is (codes, ref_is_a1, min_maf); the study its own (codes, ref_is_a1)
# over the same variants.
def spec_grm_t(codes, ref_is_a1, comps, min_maf=0.0, block=4096):
    """t [V][k] = d (A u_c), in blocks of rows so that A is never held whole; 0 at an unused variant."""
    comps = np.asarray(comps, dtype=np.float64).reshape(codes.shape[1], -1)
    mu, d, used, m = spec_grm_weights(spec_grm_counts(codes, ref_is_a1), min_maf)
    t = np.zeros((codes.shape[0], comps.shape[1]), dtype=np.float64)
    for r0 in range(0, codes.shape[0], block):
        g, c = dosage(codes[r0:r0 + block], ref_is_a1)
        mb, db = mu[r0:r0 + block, None], d[r0:r0 + block, None]
        t[r0:r0 + block] = db * (g.astype(np.float64) @ comps - mb * (c.astype(np.float64) @ comps))
    return t


def scale_weights(t, d, used, m, lam):
    """w = used ? t / sqrt(d * ((double)M' * lambda_c)) : 0.0, in the header's expression."""
    lam = np.asarray(lam, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = t / np.sqrt(d[:, None] * (float(m) * lam[None, :]))
    return np.where(used[:, None], w, 0.0)


def spec_grm_weights_vectors(codes, ref_is_a1, comps, lam, min_maf=0.0, block=4096):
    """w [V][k]: the left singular vectors of Z = D^1/2 A / sqrt(M')."""
    mu, d, used, m = spec_grm_weights(spec_grm_counts(codes, ref_is_a1), min_maf)
    return scale_weights(spec_grm_t(codes, ref_is_a1, comps, min_maf, block), d, used, m, lam)


def spec_grm_project(panel, panel_ref_is_a1, study, study_ref_is_a1, comps, lam, min_maf=0.0, block=4096):
    """(coords [N_study][k], called [N_study] int32): coords = (sum_v g_vq t_vc + sum_v c_vq s_vc) / M' / lambda_c with
    s = -(mu t), mu / d / M' the panel's; called = the panel's used variants at which the study sample is called."""
    assert panel.shape[0] == study.shape[0]
    lam = np.asarray(lam, dtype=np.float64)
    mu, d, used, m = spec_grm_weights(spec_grm_counts(panel, panel_ref_is_a1), min_maf)
    t = spec_grm_t(panel, panel_ref_is_a1, comps, min_maf, block)
    y = np.zeros((study.shape[1], t.shape[1]), dtype=np.float64)
    called = np.zeros(study.shape[1], dtype=np.int64)
    for r0 in range(0, study.shape[0], block):
        g, c = dosage(study[r0:r0 + block], study_ref_is_a1)
        tb = t[r0:r0 + block]
        y += g.astype(np.float64).T @ tb + c.astype(np.float64).T @ (-(mu[r0:r0 + block, None] * tb))
        called += c[used[r0:r0 + block]].sum(axis=0, dtype=np.int64)
    return y / float(m) / lam[None, :], called.astype(np.int32)


def spec_grm_project_bound(panel, panel_ref_is_a1, study, study_ref_is_a1, comps, lam, min_maf=0.0):
    """(N_panel + V + 16) 2^-52 (W_study^T diag(d) (W_panel |u_c|))_q / (M' lambda_c) with W = g + mu c: the summation bound of
    test_grm_cpu.spec_grm_bound carried through both passes (mu, d, M' the panel's)."""
    comps = np.abs(np.asarray(comps, dtype=np.float64).reshape(panel.shape[1], -1))
    lam = np.asarray(lam, dtype=np.float64)
    mu, d, used, m = spec_grm_weights(spec_grm_counts(panel, panel_ref_is_a1), min_maf)
    gp, cp = dosage(panel, panel_ref_is_a1)
    gs, cs = dosage(study, study_ref_is_a1)
    wp = gp.astype(np.float64) + mu[:, None] * cp.astype(np.float64)
    ws = gs.astype(np.float64) + mu[:, None] * cs.astype(np.float64)
    y = ws.T @ (d[:, None] * (wp @ comps))
    return (panel.shape[1] + panel.shape[0] + 16) * 2.0 ** -52 * y / float(m) / lam[None, :]


# ---- cohorts ----------------------------------------------------------------------------------------------------------------
POPS = (1, 2, 3)


def pop_labels(n, proportions=POPS):
    parts = np.asarray(proportions, dtype=np.float64)
    edges = np.floor(np.cumsum(parts) / parts.sum() * n + 0.5).astype(int)
    return np.searchsorted(edges, np.arange(n), side="right")


def panel_and_held_out(seed=260, n_panel=260, v=1000, per_pop=(7, 13, 20), missing=0.03):
    """One Balding-Nichols draw of n_panel + sum(per_pop) samples of which the last of every population are held out: (panel
    codes, study codes, panel populations, study populations)."""
    rng = np.random.default_rng(seed)
    n = n_panel + sum(per_pop)
    codes = balding_nichols(rng, n, v, missing=missing)
    pop = pop_labels(n)
    held = np.zeros(n, dtype=bool)
    for p, k in enumerate(per_pop):
        held[np.nonzero(pop == p)[0][-k:]] = True
    return (np.ascontiguousarray(codes[:, ~held]), np.ascontiguousarray(codes[:, held]), pop[~held], pop[held])


def top_eigenpairs(codes, ref_is_a1, k, min_maf=0.0):
    lam, vec = np.linalg.eigh(dense_k(codes, ref_is_a1, min_maf))
    return vec[:, ::-1][:, :k], lam[::-1][:k], lam[::-1]


# ---- the identities ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bn():
    panel, study, pop_p, pop_s = panel_and_held_out()
    comps, lam, lam_all = top_eigenpairs(panel, False, 3)
    return {"panel": panel, "study": study, "pop_p": pop_p, "pop_s": pop_s, "comps": comps, "lam": lam, "lam_all": lam_all}


def test_the_weights_are_the_left_singular_vectors(bn):
    panel, comps, lam = bn["panel"], bn["comps"], bn["lam"]
    assert panel.shape == (1000, 260)
    mu, d, used, m = spec_grm_weights(spec_grm_counts(panel, False))
    w = spec_grm_weights_vectors(panel, False, comps, lam, block=37)
    assert np.abs(w.T @ w - np.eye(3)).max() <= 1e-12
    g, c = dosage(panel, False)
    z = np.sqrt(d)[:, None] * (g.astype(np.float64) - mu[:, None] * c.astype(np.float64)) / np.sqrt(m)
    assert np.abs(z.T @ w / np.sqrt(lam)[None, :] - comps).max() <= 1e-12
    assert not w[~used].any()
    # the unscaled vector and the scaled one differ by the stated factor only
    t = spec_grm_t(panel, False, comps)
    assert np.array_equal(scale_weights(t, d, used, m, lam), spec_grm_weights_vectors(panel, False, comps, lam))


def test_the_panel_projected_on_itself_returns_its_components(bn):
    panel, comps, lam = bn["panel"], bn["comps"], bn["lam"]
    coords, called = spec_grm_project(panel, False, panel, False, comps, lam, block=53)
    assert np.abs(coords - comps).max() <= 1e-12
    used = spec_grm_weights(spec_grm_counts(panel, False))[2]
    assert np.array_equal(called, (panel[used] != 1).sum(axis=0))
    # inside the summation bound of the two passes as well
    assert np.all(np.abs(coords - comps) <= spec_grm_project_bound(panel, False, panel, False, comps, lam) + 1e-15)


def test_held_out_samples_land_nearest_their_own_population(bn):
    panel, study, comps, lam = bn["panel"], bn["study"], bn["comps"][:, :2], bn["lam"][:2]
    la = bn["lam_all"]
    assert (la[0] - la[1]) / la[0] >= 0.01 and (la[1] - la[2]) / la[0] >= 0.01
    coords, called = spec_grm_project(panel, False, study, False, comps, lam)
    assert coords.shape == (40, 2) and called.shape == (40,) and called.min() > 0
    centroids = np.stack([comps[bn["pop_p"] == p].mean(axis=0) for p in range(3)])
    nearest = np.argmin(((coords[:, None, :] - centroids[None, :, :]) ** 2).sum(axis=2), axis=1)
    assert np.array_equal(nearest, bn["pop_s"])


def test_the_spec_is_order_free_on_an_exact_cohort_and_blind_to_the_study_coding():
    rng = np.random.default_rng(3)
    panel = exact_cohort(rng, 65, 32, 5, ref_is_a1=True)
    study = random_codes(rng, 37, 17, missing=0.1)
    comps = rng.integers(-8, 9, size=(65, 3)).astype(np.float64)
    lam = np.array([4.0, 2.0, 0.5])
    a = spec_grm_project(panel, True, study, False, comps, lam, block=7)
    b = spec_grm_project(panel, True, study, False, comps, lam)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].any()
    swapped = np.array([3, 1, 2, 0], dtype=np.uint8)[study]                 # 00 <-> 11 in the rows, the other flag: the same cohort
    c = spec_grm_project(panel, True, swapped, True, comps, lam)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    assert np.array_equal(spec_grm_t(panel, True, comps, block=5), spec_grm_t(panel, True, comps))
    assert not spec_grm_t(panel, True, comps)[~spec_grm_weights(spec_grm_counts(panel, True))[2]].any()


# ---- the ABI surface --------------------------------------------------------------------------------------------------------
PROJECT_SYMBOLS = ["pcoa_create_grm_study", "pcoa_grm_weights", "pcoa_grm_project"]


def test_project_symbols_are_declared_bound_and_exported():
    lib = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "pcoa.h")).read()
    for sym in PROJECT_SYMBOLS:
        assert sym in lib.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % sym, header), sym
    assert int(re.search(r"#define PCOA_VERSION_MINOR (\d+)", header).group(1)) >= 11
    eng = load_pkg("engine").PcoaEngine
    assert "grm_study" in eng.__init__.__code__.co_varnames and callable(eng.grm_weights) and callable(eng.grm_project)
    if os.path.exists(lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
        exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
        for sym in PROJECT_SYMBOLS:
            assert sym in exported, sym


# ---- the kernels: no scratch ------------------------------------------------------------------------------------------------
def test_grm_multi_kernels_do_not_spill_to_scratch():
    """grm_multi.hip keeps 16 K fp64 values per lane in registers in both passes and 16 K row partials in the first: every
    instantiation must fit the register file (hipcc reports it at compile time)."""
    import shutil
    import tempfile
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                              "-I", csrc, "-c", os.path.join(csrc, "grm_multi.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True)
    assert res.returncode == 0, res.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", res.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stdout)]
    assert len(names) == len(scratch)
    for family, count in (("grm_ax_multi_kernel", 2), ("grm_at_multi_kernel", 2), ("grm_project_finish_kernel", 1),
                          ("grm_called_sum_kernel", 1), ("grm_weights_out_kernel", 1)):
        assert sum(family in nm for nm in names) == count, "%s: %d instantiation(s) expected" % (family, count)
    for nm, sc in zip(names, scratch):
        assert sc == 0, "%s spills %d bytes/lane" % (nm, sc)


# ---- the hosts --------------------------------------------------------------------------------------------------------------
def read_fileset(prefix):
    """(codes [V][N], .bim lines, .fam lines) of a PLINK 1 fileset."""
    fam = [ln for ln in open(prefix + ".fam").read().splitlines() if ln.strip()]
    bim = [ln for ln in open(prefix + ".bim").read().splitlines() if ln.strip()]
    n = len(fam)
    raw = np.fromfile(prefix + ".bed", dtype=np.uint8)[3:].reshape(len(bim), (n + 3) // 4)
    codes = ((raw[:, :, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(raw.shape[0], -1)[:, :n]
    return np.ascontiguousarray(codes), bim, fam


def write_fileset(prefix, codes, bim, fam):
    with open(prefix + ".fam", "w") as f:
        f.write("".join(ln + "\n" for ln in fam))
    with open(prefix + ".bim", "w") as f:
        f.write("".join(ln + "\n" for ln in bim))
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6c, 0x1b, 0x01]))
        f.write(pack_bed(codes).tobytes())


def split_fileset(src, panel, study, study_cols):
    """The samples `study_cols` of the fileset `src` become the fileset `study`, the others `panel`; returns (panel codes, study
    codes)."""
    codes, bim, fam = read_fileset(src)
    mask = np.zeros(codes.shape[1], dtype=bool)
    mask[np.asarray(study_cols)] = True
    write_fileset(panel, codes[:, ~mask], bim, [ln for ln, m in zip(fam, mask) if not m])
    write_fileset(study, codes[:, mask], bim, [ln for ln, m in zip(fam, mask) if m])
    return np.ascontiguousarray(codes[:, ~mask]), np.ascontiguousarray(codes[:, mask])


@pytest.fixture(scope="module")
def filesets(tmp_path_factory):
    d = tmp_path_factory.mktemp("grmproject")
    g = load_golden("kat5")
    write_golden_plink(g, str(d / "kat5"))
    write_golden_vcf(g, str(d / "kat5.vcf"))
    codes, bim, fam = read_fileset(str(d / "kat5"))
    study_fam = ["FAM%d Q%04d 0 0 0 -9" % (i, i) for i in range(2)]
    write_fileset(str(d / "study"), codes[:, :2], bim, study_fam)
    paths = {"bed": str(d / "kat5.bed"), "vcf": str(d / "kat5.vcf"), "study": str(d / "study.bed"), "dir": str(d)}

    def variant(name, bim_lines=bim, fam_lines=study_fam):
        write_fileset(str(d / name), codes[:, :2], bim_lines, fam_lines)
        paths[name] = str(d / name) + ".bed"

    line3 = bim[2].split("\t")
    variant("pos", bim[:2] + ["\t".join(line3[:3] + [str(int(line3[3]) + 1)] + line3[4:])] + bim[3:])
    variant("swapped", bim[:2] + ["\t".join(line3[:4] + [line3[5], line3[4]])] + bim[3:])
    variant("cm", ["\t".join(ln.split("\t")[:2] + ["0.5"] + ln.split("\t")[3:]) for ln in bim])   # the cM column may differ
    variant("short", bim[:-1])
    variant("samename", fam_lines=[study_fam[0], fam[1]])
    paths["n_bim"] = len(bim)
    return paths


def no_engine(res):
    return "Matrix size" not in res.stdout and "pcoa_create" not in res.stderr and "pcoa error" not in res.stderr


@pytest.mark.parametrize("run", [_run_driver, _run_python], ids=["driver", "python"])
def test_the_new_flags_need_grm(filesets, run):
    out = os.path.join(filesets["dir"], "w.tsv")
    for extra, flag in ((["--grm-weights-output-path", out], "--grm-weights-output-path"),
                        (["--grm-project-path", filesets["study"]], "--grm-project-path")):
        res = run(["--input-path", filesets["bed"]] + extra)
        assert res.returncode != 0 and "--grm " in res.stderr and flag in res.stderr, res.stderr
        assert no_engine(res) and not os.path.exists(out)


@pytest.mark.parametrize("run", [_run_driver, _run_python], ids=["driver", "python"])
def test_the_old_refusals_name_the_new_flags(filesets, run):
    out = os.path.join(filesets["dir"], "l.tsv")
    for extra, old, new in ((["--loadings-output-path", out], "loadings-output-path", "--grm-weights-output-path"),
                            (["--project-input-path", filesets["vcf"]], "project-input-path", "--grm-project-path")):
        res = run(["--input-path", filesets["bed"], "--grm"] + extra)
        assert res.returncode != 0 and "--grm" in res.stderr and old in res.stderr and new in res.stderr, res.stderr
        assert no_engine(res)


@pytest.mark.parametrize("run", [_run_driver, _run_python], ids=["driver", "python"])
def test_a_study_that_does_not_match_the_panel_is_refused_before_any_engine_exists(filesets, run):
    base = ["--input-path", filesets["bed"], "--grm", "--grm-project-path"]
    cases = [("pos", ["line 3", "pos.bim", "kat5.bim"]),
             ("swapped", ["line 3", "exchanged", "not flipped"]),
             ("short", ["line %d" % filesets["n_bim"], "short.bim ends"]),
             ("samename", ["S0001", "repeats"]),
             ("vcf", [".bed"])]
    for name, words in cases:
        res = run(base + [filesets[name]])
        assert res.returncode != 0 and "--grm-project-path" in res.stderr, (name, res.stderr)
        for word in words:
            assert word in res.stderr, (name, word, res.stderr)
        assert no_engine(res), (name, res.stderr)
    # the first differing line is the one that is named
    res = run(base + [filesets["pos"]])
    assert "line 3:" in res.stderr and "line 4" not in res.stderr


def test_grm_project_flags_are_off_by_default():
    vp = load_pkg("variants_pca")
    conf = vp.PcaConf(["--grm"])
    assert conf.grm_weights_output_path is None and conf.grm_project_path is None
    conf = vp.PcaConf(["--grm", "--grm-weights-output-path", "w", "--grm-project-path", "s.bed"])
    assert conf.grm_weights_output_path == "w" and conf.grm_project_path == "s.bed"


def test_a_matching_study_passes_the_check_and_the_cm_column_is_not_compared(filesets):
    vp = load_pkg("variants_pca")
    vp.check_grm_study(filesets["bed"], filesets["study"])
    vp.check_grm_study(filesets["bed"], filesets["cm"])
    with pytest.raises(SystemExit) as ei:
        vp.check_grm_study(filesets["bed"], filesets["swapped"])
    assert "line 3" in str(ei.value)

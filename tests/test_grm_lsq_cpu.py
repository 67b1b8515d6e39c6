"""CPU tests of the least-squares projection of sparsely called samples on a GRM engine (pcoa_grm_project_lsq,
--grm-project-lsq): the numpy twin of the rule in include/pcoa.h (imported by tests/test_gpu_grm_lsq.py), whose solve is a scalar
fp64 restatement of the header's operation sequence, the identities the rule rests on, the claim it is built for -- a sample
called at a share f of the variants lands where its full data would put it, not at f times that --, the undetermined rule, the
ABI surface, the refusals of both hosts, and the compile-time resource check of the kernels of grm_lsq.hip."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, load_pkg
from test_grm_cpu import _run_driver, _run_python, dosage, exact_cohort, spec_grm_counts, spec_grm_weights
from test_grm_project_cpu import filesets, no_engine, panel_and_held_out, spec_grm_project, spec_grm_t, top_eigenpairs  # noqa: F401


# ---- the twin (include/pcoa.h, "least-squares projection of sparsely called samples") ---------------------------------------
def pair_index(c, c2):
    return c * (c + 1) // 2 + c2


def lsq_solve_one(hq, pq):
    """(x [K], determined): the header's sequence on one sample's packed H_q and P_q, in Python floats -- every product and
    difference an fp64 operation of its own."""
    k = len(pq)
    h = [float(x) for x in hq]
    for c in range(k):
        rc = c * (c + 1) // 2
        hcc = h[rc + c]
        if hcc == 0.0:
            return [float("nan")] * k, False
        for j in range(c):
            rj = j * (j + 1) // 2
            s = h[rc + j]
            for i in range(j):
                s = s - h[rc + i] * h[rj + i]
            h[rc + j] = s
        s = hcc
        for i in range(c):
            w = h[rc + i]
            el = w / h[i * (i + 1) // 2 + i]
            s = s - w * el
            h[rc + i] = el
        if s <= 2.0 ** -40 * hcc:
            return [float("nan")] * k, False
        h[rc + c] = s
    b = [float(x) for x in pq]
    for c in range(k):
        rc = c * (c + 1) // 2
        s = b[c]
        for i in range(c):
            s = s - h[rc + i] * b[i]
        b[c] = s
    for c in range(k):
        b[c] = b[c] / h[c * (c + 1) // 2 + c]
    for c in range(k - 1, -1, -1):
        s = b[c]
        for i in range(c + 1, k):
            s = s - h[i * (i + 1) // 2 + c] * b[i]
        b[c] = s
    return b, True


def lsq_solve(h, p):
    """h [Nq][K (K + 1) / 2], p [Nq][K] -> (x [Nq][K], determined [Nq] bool)."""
    x = np.empty(p.shape, dtype=np.float64)
    det = np.empty(p.shape[0], dtype=bool)
    for q in range(p.shape[0]):
        x[q], det[q] = lsq_solve_one(h[q], p[q])
    return x, det


def lsq_products(t, d, used):
    """p [V][K (K + 1) / 2] = used ? (t_c * t_c') / d : 0.0, in the header's expression."""
    k = t.shape[1]
    out = np.zeros((t.shape[0], k * (k + 1) // 2), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(k):
            for c2 in range(c + 1):
                out[:, pair_index(c, c2)] = np.where(used, (t[:, c] * t[:, c2]) / d, 0.0)
    return out


def spec_grm_lsq(panel, panel_ref_is_a1, study, study_ref_is_a1, comps, min_maf=0.0, block=4096, t=None, solve=True):
    """(H [Nq][K (K + 1) / 2], P [Nq][K], x [Nq][K], determined [Nq] bool).  t: [V][K] to use in place of the twin's own
    t = d (A u_c) (the device's, where a test separates the two passes).  solve=False: x and determined are None."""
    assert panel.shape[0] == study.shape[0]
    mu, d, used, m = spec_grm_weights(spec_grm_counts(panel, panel_ref_is_a1), min_maf)
    if t is None:
        t = spec_grm_t(panel, panel_ref_is_a1, comps, min_maf, block)
    prod = lsq_products(t, d, used)
    h = np.zeros((study.shape[1], prod.shape[1]), dtype=np.float64)
    p = np.zeros((study.shape[1], t.shape[1]), dtype=np.float64)
    for r0 in range(0, study.shape[0], block):
        g, c = dosage(study[r0:r0 + block], study_ref_is_a1)
        tb = t[r0:r0 + block]
        p += g.astype(np.float64).T @ tb + c.astype(np.float64).T @ (-(mu[r0:r0 + block, None] * tb))
        h += c.astype(np.float64).T @ prod[r0:r0 + block]
    x, det = lsq_solve(h, p) if solve else (None, None)
    return h, p, x, det


def mask_calls(study, share, seed):
    """A copy of `study` with every call set to 01 independently with probability `share`."""
    out = study.copy()
    out[np.random.default_rng(seed).random(out.shape) < share] = 1
    return out


def slopes(est, full):
    """Per axis, the regression slope (with intercept) of the estimated coordinates on the full-data ones."""
    return np.array([np.polyfit(full[:, c], est[:, c], 1)[0] for c in range(full.shape[1])])


def nearest_centroid(coords, comps, pop_p):
    centroids = np.stack([comps[pop_p == p].mean(axis=0) for p in range(3)])
    return np.argmin(((coords[:, None, :] - centroids[None, :, :]) ** 2).sum(axis=2), axis=1)


# ---- the identities ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bn():
    panel, study, pop_p, pop_s = panel_and_held_out()
    comps, lam, _ = top_eigenpairs(panel, False, 3)
    return {"panel": panel, "study": study, "pop_p": pop_p, "pop_s": pop_s, "comps": comps, "lam": lam}


@pytest.fixture(scope="module")
def bn_full():
    """The same draw with no missing call in it: every sample is fully called."""
    panel, study, pop_p, pop_s = panel_and_held_out(missing=0.0)
    comps, lam, _ = top_eigenpairs(panel, False, 3)
    return {"panel": panel, "study": study, "comps": comps, "lam": lam}


def test_the_twin_equals_lstsq_on_the_standardised_called_rows(bn):
    panel, comps, lam = bn["panel"], bn["comps"], bn["lam"]
    study = mask_calls(bn["study"], 0.7, 0)
    mu, d, used, m = spec_grm_weights(spec_grm_counts(panel, False))
    t = spec_grm_t(panel, False, comps)
    h, p, x, det = spec_grm_lsq(panel, False, study, False, comps, block=97)
    assert det.all()
    g, c = dosage(study, False)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(used[:, None], t / np.sqrt(d * float(m))[:, None], 0.0)          # w_vc sqrt(lambda_c)
    for q in range(study.shape[1]):
        rows = used & (c[:, q] == 1)
        z = np.sqrt(d[rows]) * (g[rows, q].astype(np.float64) - mu[rows]) / np.sqrt(float(m))
        ref = np.linalg.lstsq(w[rows], z, rcond=None)[0]
        assert np.abs(x[q] - ref).max() <= 1e-10, q


def test_a_fully_called_panel_projected_on_itself_returns_its_components(bn_full):
    """With calls missing in the panel, K is the mean-imputed matrix and a panel sample's fit over ITS called rows is not u: the
    identity is the fully called one, so the fixture is drawn with missing = 0 (at its usual 3 % of missing calls the largest
    |x - u| is 6.9e-3)."""
    panel, comps, lam = bn_full["panel"], bn_full["comps"], bn_full["lam"]
    m = spec_grm_weights(spec_grm_counts(panel, False))[3]
    h, p, x, det = spec_grm_lsq(panel, False, panel, False, comps, block=53)
    assert det.all() and np.abs(x - comps).max() <= 1e-10
    # H of a fully called sample is diag(M' lambda), the same for every sample
    k = comps.shape[1]
    for c in range(k):
        for c2 in range(c + 1):
            col = h[:, c * (c + 1) // 2 + c2]
            want = float(m) * lam[c] if c == c2 else 0.0
            assert np.abs(col - want).max() <= 1e-12 * float(m) * lam[0], (c, c2)
    # and P / M' / lambda is the mean-imputed coordinate, so the two rules agree
    coords, _ = spec_grm_project(panel, False, panel, False, comps, lam, block=53)
    assert np.abs(x - coords).max() <= 1e-10


@pytest.mark.parametrize("seed", range(5))
def test_sparsely_called_samples_land_where_their_full_data_puts_them(bn, seed):
    """The claim: held-out calls masked to 01 with probability 0.7.  The least-squares placement regresses on the unmasked
    mean-imputed one with slope in [0.9, 1.15] per axis and every sample falls nearest its own population's centroid; the
    mean-imputed placement of the same masked samples has slope below 0.4."""
    panel, comps, lam = bn["panel"], bn["comps"][:, :2], bn["lam"][:2]
    full, _ = spec_grm_project(panel, False, bn["study"], False, comps, lam)
    masked = mask_calls(bn["study"], 0.7, seed)
    h, p, x, det = spec_grm_lsq(panel, False, masked, False, comps)
    assert det.all()
    s = slopes(x, full)
    assert np.all(s >= 0.9) and np.all(s <= 1.15), s
    assert np.array_equal(nearest_centroid(x, comps, bn["pop_p"]), bn["pop_s"])
    shrunk, _ = spec_grm_project(panel, False, masked, False, comps, lam)
    assert np.all(slopes(shrunk, full) < 0.4), slopes(shrunk, full)


def test_h_and_p_are_the_same_integers_under_any_row_order_and_block_size():
    rng = np.random.default_rng(11)
    panel = exact_cohort(rng, 65, 32, 5, ref_is_a1=True)
    study = mask_calls(exact_cohort(rng, 37, 32, 5), 0.5, 1)
    comps = rng.integers(-8, 9, size=(65, 3)).astype(np.float64)
    a = spec_grm_lsq(panel, True, study, False, comps, block=7)
    b = spec_grm_lsq(panel, True, study, False, comps)
    perm = rng.permutation(panel.shape[0])
    c = spec_grm_lsq(panel[perm], True, study[perm], False, comps, block=5)
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1])
    assert a[0].any() and a[1].any() and np.array_equal(a[0], np.round(a[0])) and np.array_equal(a[1], np.round(a[1]))
    swapped = np.array([3, 1, 2, 0], dtype=np.uint8)[study]      # 00 <-> 11 in the rows, the other flag: the same cohort
    e = spec_grm_lsq(panel, True, swapped, True, comps)
    assert np.array_equal(a[0], e[0]) and np.array_equal(a[1], e[1])


# ---- undetermined samples ---------------------------------------------------------------------------------------------------
def undetermined_cohort(seed=5, n_panel=65, v_used=64, v_unused=3, nq=8, k=2):
    """(panel, study, comps, expect): an exact panel whose used rows r0 and r1 are equal (so t is equal there); study sample 1
    is called at K - 1 used variants, sample 3 at none, sample 5 only at r0 and r1 -- K rows at which its t columns are
    proportional; every other sample is called almost everywhere.  expect: determined [nq]."""
    rng = np.random.default_rng(seed)
    panel = exact_cohort(rng, n_panel, v_used, v_unused)
    used = np.nonzero(spec_grm_weights(spec_grm_counts(panel, False))[2])[0]
    r0, r1 = int(used[3]), int(used[17])
    panel[r1] = panel[r0]
    study = exact_cohort(rng, nq, v_used + v_unused)
    study[:, 1] = 1
    study[used[:k - 1], 1] = 2
    study[:, 3] = 1
    study[:, 5] = 1
    study[[r0, r1], 5] = (0, 2)
    comps = rng.integers(-8, 9, size=(n_panel, k)).astype(np.float64)
    expect = np.ones(nq, dtype=bool)
    expect[[1, 3, 5]] = False
    return panel, study, comps, expect


def test_the_three_kinds_of_undetermined_samples_and_their_neighbours():
    panel, study, comps, expect = undetermined_cohort()
    h, p, x, det = spec_grm_lsq(panel, False, study, False, comps)
    assert np.array_equal(det, expect)
    assert np.isnan(x[~expect]).all() and np.isfinite(x[expect]).all()
    assert h[3].max() == 0.0 and h[1, 0] > 0.0 and h[5].min() > 0.0      # none called; K - 1 rows; two proportional rows
    k = comps.shape[1]
    called = (study[spec_grm_weights(spec_grm_counts(panel, False))[2]] != 1).sum(axis=0)
    assert called[1] == k - 1 and called[3] == 0 and called[5] == k and called[expect].min() > k


# ---- the ABI surface --------------------------------------------------------------------------------------------------------
LSQ_SYMBOLS = ["pcoa_grm_project_lsq", "pcoa_get_grm_lsq_stats"]


def test_lsq_symbols_are_declared_bound_and_exported():
    lib = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "pcoa.h")).read()
    for sym in LSQ_SYMBOLS:
        assert sym in lib.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % sym, header), sym
    assert int(re.search(r"#define PCOA_VERSION_MINOR (\d+)", header).group(1)) >= 17
    eng = load_pkg("engine").PcoaEngine
    assert callable(eng.grm_project_lsq) and callable(eng.grm_lsq_stats)
    if os.path.exists(lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
        exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
        for sym in LSQ_SYMBOLS:
            assert sym in exported, sym


# ---- the kernels: no scratch ------------------------------------------------------------------------------------------------
def test_grm_lsq_kernels_do_not_spill_to_scratch():
    """grm_lsq_pairs_kernel<4> keeps 64 fp64 accumulators per lane beside the rows and products in flight; the solve works in
    global memory with no local array: every instantiation must report 0 scratch (hipcc reports it at compile time)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                              "-I", csrc, "-c", os.path.join(csrc, "grm_lsq.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True)
    assert res.returncode == 0, res.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", res.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stdout)]
    assert len(names) == len(scratch)
    for family, count in (("grm_lsq_products_kernel", 1), ("grm_lsq_pairs_kernel", 3), ("grm_lsq_finish_kernel", 1),
                          ("grm_lsq_solve_kernel", 1)):
        assert sum(family in nm for nm in names) == count, "%s: %d instantiation(s) expected" % (family, count)
    for nm, sc in zip(names, scratch):
        assert sc == 0, "%s spills %d bytes/lane" % (nm, sc)


# ---- the hosts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [_run_driver, _run_python], ids=["driver", "python"])
def test_project_lsq_needs_grm(filesets, run):
    res = run(["--input-path", filesets["bed"], "--grm-project-lsq"])
    assert res.returncode != 0 and "--grm " in res.stderr and "--grm-project-lsq" in res.stderr, res.stderr
    assert no_engine(res)


@pytest.mark.parametrize("run", [_run_driver, _run_python], ids=["driver", "python"])
def test_project_lsq_alone_is_refused_and_the_message_names_the_two_projections(filesets, run):
    res = run(["--input-path", filesets["bed"], "--grm", "--grm-project-lsq"])
    assert res.returncode != 0, res.stderr
    for word in ("--grm-project-lsq", "--grm-project-path", "--grm-project-removed"):
        assert word in res.stderr, (word, res.stderr)
    assert no_engine(res)


@pytest.mark.parametrize("run", [_run_driver, _run_python], ids=["driver", "python"])
def test_project_lsq_refuses_more_than_16_components(filesets, run):
    res = run(["--input-path", filesets["bed"], "--grm", "--grm-project-removed", "--grm-project-lsq", "--num-pc", "17"])
    assert res.returncode != 0 and "--grm-project-lsq" in res.stderr and "16" in res.stderr, res.stderr
    assert no_engine(res)


def test_project_lsq_is_off_by_default():
    vp = load_pkg("variants_pca")
    assert vp.PcaConf(["--grm"]).grm_project_lsq is False
    assert vp.PcaConf(["--grm", "--grm-project-removed", "--grm-project-lsq"]).grm_project_lsq is True

"""GPU tests of pcoa_project (out-of-sample projection onto a reference cohort's principal coordinates) and of
--project-input-path in both hosts.  The main check needs no oracle: a strip over the reference cohort itself projects every
sample onto its own component entries, up to the residual the eigensolver verified (pcoa.h)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_cases, int_gram, load_golden, load_pkg, write_golden_vcf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    return load_pkg("engine")


@pytest.fixture(scope="module")
def L():
    return load_pkg("_lib")


def _tile(rng, n, v, pops=5):
    """v x n uint8 genotypes with population structure (0 / 1)."""
    lab = np.sort(rng.integers(0, pops, size=n))
    f = rng.uniform(0.02, 0.5, size=(v, pops))
    return (rng.random((v, n)) < f[:, lab]).astype(np.uint8)


def _engine(E, n, x, strip=None, **kw):
    e = E.PcoaEngine(n, strip=strip, **kw)
    e.accumulate_dense_u8(np.ascontiguousarray(x))
    e.finalize()
    return e


def _identity_bound(lam):
    """pcoa_compute accepts a pair when ||r_c|| <= 1e-11 |lambda_1|: the identity error |r_c[i]| / |lambda_c| is below
    1e-11 |lambda_1| / |lambda_c|; a factor of ten covers the order of the sum."""
    return 1e-10 * abs(lam[0]) / np.abs(lam)


@pytest.mark.parametrize("n, k", [(2504, 4), (20000, 2)])
def test_projecting_the_reference_cohort_returns_its_components(E, n, k):
    rng = np.random.default_rng(n)
    x = _tile(rng, n, 1500)
    ref = _engine(E, n, x)
    comps, lam, _ = ref.compute(k)
    bound = _identity_bound(lam)
    for c0, w in [(0, 1), (1000, 777), (n - 257, 257)]:
        cross = _engine(E, n, x, strip=(c0, w))
        got = ref.project(cross, comps, lam)
        cross.close()
        assert got.shape == (w, k)
        err = np.abs(got - comps[c0:c0 + w]).max(axis=0)
        assert np.all(err <= bound), (c0, w, err, bound)
    ref.close()


def _numpy_projection(s_ref, x_cross, comps, lam):
    """The spec of pcoa.h in fp64 numpy: b(q, j) = ((x(j, q) - m_q) - mean_j) + mm, coord = (sum_j b u_c[j]) / lambda_c.
    Returns (coords, sum_j |b u_c[j]| / |lambda_c|)."""
    n_ref = s_ref.shape[0]
    rs = s_ref.sum(axis=1)
    mean = rs.astype(np.float64) / n_ref
    mm = float(rs.sum()) / n_ref / n_ref
    m_q = x_cross.sum(axis=0).astype(np.float64) / n_ref
    b = ((x_cross.astype(np.float64) - m_q[None, :]) - mean[:, None]) + mm     # [n_ref][cols]
    return (b.T @ comps) / lam, (np.abs(b).T @ np.abs(comps)) / np.abs(lam)


@pytest.fixture(scope="module")
def small(E):
    """N_ref = 500 reference samples and 123 new ones; new sample 0 copies reference sample 7's genotypes."""
    rng = np.random.default_rng(5)
    n_ref, n_new = 500, 123
    x = _tile(rng, n_ref + n_new, 2000)
    x[:, n_ref] = x[:, 7]
    s = int_gram(x)
    ref = _engine(E, n_ref, x[:, :n_ref])
    assert np.array_equal(ref.gram(), s[:n_ref, :n_ref])
    cross = _engine(E, n_ref + n_new, x, strip=(n_ref, n_new))
    yield dict(x=x, s=s, ref=ref, cross=cross, n_ref=n_ref, n_new=n_new)
    cross.close()
    ref.close()


def test_projection_agrees_with_numpy_and_places_a_copy_on_its_original(small):
    ref, cross, s, n_ref = small["ref"], small["cross"], small["s"], small["n_ref"]
    comps, lam, _ = ref.compute(3)
    got = ref.project(cross, comps, lam)
    want, scale = _numpy_projection(s[:n_ref, :n_ref], s[:n_ref, n_ref:], comps, lam)
    assert np.all(np.abs(got - want) <= 1e-12 * scale)
    assert np.all(np.abs(got[0] - comps[7]) <= _identity_bound(lam))


def test_columns_are_independent_and_calls_deterministic(E, small):
    ref, x, n_ref, n_new = small["ref"], small["x"], small["n_ref"], small["n_new"]
    comps, lam, _ = ref.compute(2)
    one = ref.project(small["cross"], comps, lam)
    assert np.array_equal(one, ref.project(small["cross"], comps, lam))     # two calls: bit for bit
    a = _engine(E, n_ref + n_new, x, strip=(n_ref, 60))
    b = _engine(E, n_ref + n_new, x, strip=(n_ref + 60, n_new - 60))
    two = np.concatenate([ref.project(a, comps, lam), ref.project(b, comps, lam)])
    a.close()
    b.close()
    assert np.array_equal(one, two)


def test_nine_components_run_in_two_chunks_equal_to_one_at_a_time(small):
    ref, cross = small["ref"], small["cross"]
    comps, lam, _ = ref.compute(9)
    got = ref.project(cross, comps, lam)
    for c in range(9):
        assert np.array_equal(got[:, c:c + 1], ref.project(cross, comps[:, c:c + 1], lam[c:c + 1])), c


def test_int64_part(E, small):
    s, n_ref, n_new = small["s"], small["n_ref"], small["n_new"]
    big = s + 3 * 2 ** 31                          # every entry beyond int32; centring cancels the constant exactly
    ref = E.PcoaEngine(n_ref)
    ref.load_gram(big[:n_ref, :n_ref])
    cross = E.PcoaEngine(n_ref + n_new, strip=(n_ref, n_new))
    cross.load_gram(big[:, n_ref:])
    assert ref.timings()["gram_i64_live"] == 1 and cross.timings()["gram_i64_live"] == 1
    comps, lam, _ = ref.compute(2)
    got = ref.project(cross, comps, lam)
    want, scale = _numpy_projection(big[:n_ref, :n_ref], big[:n_ref, n_ref:], comps, lam)
    assert np.all(np.abs(got - want) <= 1e-12 * scale)
    c_small, l_small, _ = small["ref"].compute(2)
    small_coords = small["ref"].project(small["cross"], c_small, l_small)
    _, scale_small = _numpy_projection(s[:n_ref, :n_ref], s[:n_ref, n_ref:], c_small, l_small)
    assert np.all(np.abs(got - small_coords) <= 1e-6 * scale_small)
    cross.close()
    ref.close()


def test_refusals(E, L, small):
    ref, cross, n_ref = small["ref"], small["cross"], small["n_ref"]
    lib = L.load()
    comps, lam, _ = ref.compute(2)
    u = np.ascontiguousarray(comps.T)
    out = np.zeros((2, small["n_new"]))
    p = lambda a: ctypes.c_void_p(a.ctypes.data)

    def call(r, c, k, uu=u, ll=lam, oo=out):
        rc = lib.pcoa_project(r._ctx if r is not None else None, c._ctx if c is not None else None, k,
                              p(uu) if uu is not None else None, p(ll) if ll is not None else None, p(oo) if oo is not None else None)
        return rc, lib.pcoa_last_error(r._ctx if r is not None else None).decode()

    assert call(ref, None, 2)[0] == L.PCOA_ERR_INVALID_ARG
    for kw in ({"uu": None}, {"ll": None}, {"oo": None}):
        rc, msg = call(ref, cross, 2, **kw)
        assert rc == L.PCOA_ERR_INVALID_ARG and "NULL" in msg
    for k in (0, -1, n_ref + 1):
        rc, msg = call(ref, cross, k)
        assert rc == L.PCOA_ERR_INVALID_ARG and "num_pc" in msg, k
    rc, msg = call(ref, cross, 2, ll=np.array([lam[0], 0.0]))
    assert rc == L.PCOA_ERR_INVALID_ARG and "eigenvalue 1" in msg
    short = E.PcoaEngine(n_ref - 1, strip=(0, 4))
    rc, msg = call(ref, short, 2)
    assert rc == L.PCOA_ERR_INVALID_ARG and "fewer than ref's" in msg
    short.close()
    rc, msg = call(cross, ref, 2)
    assert rc == L.PCOA_ERR_INVALID_ARG and "ref is a strip owner" in msg
    rc, msg = call(ref, ref, 2)
    assert rc == L.PCOA_ERR_INVALID_ARG and "cross is not a strip owner" in msg
    # an engine whose input check failed cannot serve: forced MX-FP4 fed a multiplicity of 2
    bad = E.PcoaEngine(n_ref + 4, strip=(n_ref, 4), gram_kernel="fp4")
    t = np.zeros((3, n_ref + 4), dtype=np.uint8)
    t[1, 2] = 2
    try:
        bad.accumulate_dense_u8(t)
    except E.PcoaError:
        pass   # (reported here or at the next synchronising call: the engine's S stays invalid either way)
    rc, msg = call(ref, bad, 2, oo=np.zeros((2, 4)))
    assert rc == L.PCOA_ERR_STATE and msg.startswith("project: cross:"), (rc, msg)
    bad.close()
    with pytest.raises(E.PcoaError):
        ref.project(cross, comps, np.array([lam[0], 0.0]))


# ---------------------------------------------------------------------------------------------------------- both hosts
def _exe():
    exe = os.path.join(ROOT, "spark-examples_amd", "variants_pca_driver")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "spark-examples_amd", "host")])
    return exe


def _hosts(args):
    c = subprocess.run([_exe()] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "spark-examples_amd", "variants_pca.py")] + args,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    return c, p


def _rows(stdout):
    return dict((l.split("\t")[0], l) for l in stdout.splitlines() if "\t" in l)


@pytest.mark.parametrize("name", golden_cases())
def test_both_hosts_project_a_renamed_copy_of_every_golden_onto_itself(E, name, tmp_path):
    g = load_golden(name)
    n = int(g["n_samples"])
    panel, study = str(tmp_path / "panel.vcf"), str(tmp_path / "study.vcf")
    write_golden_vcf(g, panel)
    with open(panel) as f:
        text = f.read()
    with open(study, "w") as f:   # the same genotypes under other sample names
        f.write(re.sub(r"\tS(\d{4})", r"\tP\1", text))
    base = ["--all-references"]
    plain_c, plain_p = _hosts(["--input-path", panel] + base)
    assert plain_c.returncode == 0 and plain_p.returncode == 0, (plain_c.stderr[-2000:], plain_p.stderr[-2000:])
    ref = E.PcoaEngine(n)                          # lambda of the run: the engine on the golden's S
    ref.load_gram(g["similarity"])
    _, lam, _ = ref.compute(2)
    ref.close()
    c, p = _hosts(["--input-path", panel, "--project-input-path", study] + base)
    if np.any(lam == 0.0):
        for r in (c, p):
            assert r.returncode != 0 and "zero or not finite" in r.stderr
        return
    assert c.returncode == 0 and p.returncode == 0, (c.stderr[-2000:], p.stderr[-2000:])
    assert c.stdout == p.stdout
    assert "Projected %d samples onto 2 principal components of %d reference samples." % (n, n) in c.stdout
    assert "Matrix size: %d." % n in c.stdout
    want, got = _rows(plain_c.stdout), _rows(c.stdout)
    assert _rows(plain_p.stdout) == want
    assert len(got) == 2 * n
    bound = _identity_bound(lam)
    for i in range(n):
        s_name, p_name = "S%04d" % i, "P%04d" % i
        assert got[s_name] == want[s_name]                      # the reference rows: byte for byte
        a = np.array([float(v) for v in got[s_name].split("\t")[2:4]])
        b = np.array([float(v) for v in got[p_name].split("\t")[2:4]])
        assert got[p_name].split("\t")[1] == "study"
        assert np.all(np.abs(a - b) <= bound), (i, a, b, bound)

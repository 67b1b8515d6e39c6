"""The Lanczos path of computePca (csrc/eig_lanczos.hip) held to exact spectra, with the branch taken asserted by name.

Every case loads an integer S with a known spectrum (tests/eig_spectra.py) through pcoa_gram_load_i64 and checks: the
counters of pcoa_timings against the branch the case is built for (eig_method, matvec_form, lanczos_steps,
lanczos_block_steps), the pairs against the reference (eig_spectra.check_pairs: eigenvalues, host residuals, orthogonality,
vectors or cluster subspaces, the sign rule), and a second compute on the same engine bit-identical to the first.  One
`LANCZOS_EIG {json}` line per case reports the observed maxima and the counters (profiles/*_lanczos_bands.txt).

The bars are eig_spectra.lanczos_bars: derived from the acceptance rule of the path (true residual x 0.125 <= 1e-11 scale),
not from the dense solver's accuracy and not measured.  Pairs that the dense solver returned (`auto` after a Lanczos run
that did not verify) are held to the dense bars.

The single-vector iteration examines its Ritz pairs at m = 12, 16, 20, 24, every 8 steps to 64, then every m / 2 (96, 144,
216, 324, 486), at k + 2 first where that is more than 12, and at mmax = min(N, 512) at the latest; lanczos_steps is the m of
the last check.

The knobs are read once per process, so every environment runs in one child process, which takes its cases in turn, checks
them and reports one JSON line per case (pairs in an .npz beside it for the comparisons between environments).  Walls of the
children on an idle MI355X, process start-up and the building of the references included: upper_triangle 3.0 s, default
3.2 s, band_restarts 2.4 s, explicit_b 2.5 s; the limits in ENVS are about 10x.  Every in-process case takes under a second
but the first (1.8 s: the library and the device are opened).
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import eig_spectra as E  # noqa: E402
from conftest import load_oracle, load_pkg  # noqa: E402

pytestmark = pytest.mark.gpu

PCOA_ERR_NOT_CONVERGED = -7
MMAX = 512
BAND_MMAX = 40                # the smallest budget the band iteration accepts for k = 2 is 4 * 2 (k + 2) + 2 = 34


def schedule(n, k):
    """The m at which lanczos_single examines its Ritz pairs."""
    mmax = min(n, MMAX)
    out, m = set(), min(max(12, k + 2), mmax)
    while True:
        out.add(m)
        if m >= mmax:
            return out
        m = min(m + 4 if m < 24 else m + 8 if m < 64 else m + m // 2, mmax)


# case -> (builder of the Spectrum, eig)
CASES = {}
for _n in (32, 33, 40, 255, 256, 257, 1025):
    CASES["planted-%d" % _n] = ((lambda n: lambda: E.planted(n, 2))(_n), "lanczos")
CASES["low-rank-600-k11"] = (lambda: E.shifted_low_rank(600, 11, v=24), "lanczos")
CASES["low-rank-600-k15"] = (lambda: E.shifted_low_rank(600, 11, v=24).top(15), "lanczos")
CASES["full-but-one-32"] = (lambda: E.planted(32, 31), "auto")
for _n in (64, 1028):
    CASES["rank3-%d" % _n] = ((lambda n: lambda: E.shifted_low_rank(n, 2, v=3, c=0))(_n), "auto")
    CASES["rank3-lanczos-%d" % _n] = (CASES["rank3-%d" % _n][0], "lanczos")
for _n in (260, 1025):
    CASES["negative-dominant-%d" % _n] = ((lambda n: lambda: E.negative_dominant(n, 2))(_n), "lanczos")
CASES["int64-1028"] = (lambda: E.shifted_low_rank(1028, 2, scale=2 ** 24), "lanczos")
CASES["multiplicity2-1028"] = (lambda: E.multiplicity(1028, 4, 2), "auto")
CASES["multiplicity2-band-1028"] = (CASES["multiplicity2-1028"][0], "band")
CASES["near-tie-1028"] = (lambda: E.near_tie(1028, 2), "auto")
# children
CASES["planted-1028"] = (lambda: E.planted(1028, 2), "auto")
CASES["planted-2052"] = (lambda: E.planted(2052, 2), "auto")
CASES["near-tie-1044"] = (lambda: E.near_tie(1044, 2), "auto")
CASES["noisy-1028"] = (lambda: E.shifted_low_rank(1028, 2, v=8, noise=True), "lanczos")
CASES["multiplicity2-1028-k2"] = (lambda: E.multiplicity(1028, 4, 2).top(2), "lanczos")

SYM_CASES = ("planted-1028", "planted-2052", "near-tie-1044")
# environment -> (cases, knobs, child time limit in seconds: about 10x the wall on an idle MI355X)
ENVS = {
    "upper_triangle": (SYM_CASES, {"PCOA_SYMV_SYM_MIN_N": "4"}, 30),
    "default": (SYM_CASES + ("planted-257",), {}, 30),
    "band_restarts": (("noisy-1028", "multiplicity2-1028-k2"), {"PCOA_LANCZOS_BAND": "2", "PCOA_LANCZOS_BAND_MMAX": str(BAND_MMAX)}, 30),
    "explicit_b": (("planted-257",), {"PCOA_EXPLICIT_CENTER": "1"}, 30),
}


_SPECTRA = {}


def spectrum(case):
    """The case's Spectrum, built once per builder (cases that differ in `eig` only share it) and never modified."""
    build = CASES[case][0]
    if build not in _SPECTRA:
        _SPECTRA[build] = build()
    return _SPECTRA[build]


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def O():
    return load_oracle()


def _bmul(O, sp):
    b = getattr(sp, "b", None)
    if b is None:
        b = O.center_matrix(sp.s)[0]
    return lambda u: b @ u


COUNTERS = ("eig_method", "matvec_form", "lanczos_steps", "lanczos_block_steps", "gram_i64_live", "eig_dense_form")


def _report(case, sp, t, obs, wall):
    rec = {"case": case, "n": sp.n, "k": sp.k, "family": sp.family}
    rec.update(dict((key, int(t[key])) for key in COUNTERS))
    rec.update({"gpu_ms": round(1e3 * t["compute_total_seconds"], 2), "host_s": round(wall, 2)})
    rec.update(dict((key, float("%.3g" % v)) for key, v in obs.items()))
    print("LANCZOS_EIG " + json.dumps(rec))
    return rec


def solve(P, sp, eig):
    """Two computes on one engine: the pairs (bit-identical the second time) and the timings of the first."""
    with P.PcoaEngine(sp.n, eig=eig) as eng:
        eng.load_gram(sp.s)
        comps, lam, _ = eng.compute(sp.k)
        t = eng.timings()
        comps2, lam2, _ = eng.compute(sp.k)
    assert np.array_equal(comps, comps2) and np.array_equal(lam, lam2), "second compute differs"
    return comps, lam, t


def check(O, case, sp, comps, lam, t, wall=0.0):
    """Lanczos pairs to the Lanczos bars, the dense solver's to the dense bars."""
    assert t["eig_method"] in (1, 2), t
    bars = E.lanczos_bars(sp) if t["eig_method"] == 1 else None
    obs = E.check_pairs(sp, comps, lam, _bmul(O, sp), case, bars=bars)
    return _report(case, sp, t, obs, wall)


def run(P, O, case):
    t0 = time.time()
    sp = spectrum(case)
    comps, lam, t = solve(P, sp, CASES[case][1])
    check(O, case, sp, comps, lam, t, time.time() - t0)
    return sp, comps, lam, t


# ------------------------------------------------------------------------------------------- in-process: no knob needed
@pytest.mark.parametrize("n", [32, 33, 40, 255, 256, 257, 1025])
def test_single_vector_iteration_on_ordinary_spectra(P, O, n):
    """mmax = n < 512, the ceil(n / 256) slices of the CGS kernels, the 4-byte mat-vec (n % 4 != 0) and the 16-byte one."""
    sp, _, _, t = run(P, O, "planted-%d" % n)
    assert t["eig_method"] == 1 and t["matvec_form"] == 0 and t["lanczos_block_steps"] == 0, t
    assert t["lanczos_steps"] in schedule(n, sp.k), (t["lanczos_steps"], sorted(schedule(n, sp.k)))


@pytest.mark.parametrize("k", [11, 15])
def test_first_check_waits_for_k_plus_2_steps(P, O, k):
    """next_check = k + 2 where that is more than 12: T_m needs the k wanted Ritz values and one more on each side."""
    sp, _, _, t = run(P, O, "low-rank-600-k%d" % k)
    assert sp.k == k and t["eig_method"] == 1 and t["matvec_form"] == 0, t
    assert t["lanczos_steps"] >= k + 2 and t["lanczos_steps"] in schedule(600, k), (t, sorted(schedule(600, k)))


def test_more_pairs_than_the_krylov_basis_can_hold(P, O):
    """n = 32, k = 31: mmax = 32 < k + 2.  Neither iteration starts: `lanczos` reports it, `auto` returns the dense solver's
    pairs."""
    sp = spectrum("full-but-one-32")
    with P.PcoaEngine(sp.n, eig="lanczos") as eng:
        eng.load_gram(sp.s)
        with pytest.raises(P.PcoaError) as err:
            eng.compute(sp.k)
        assert err.value.code == PCOA_ERR_NOT_CONVERGED, err.value
        t = eng.timings()
        assert t["lanczos_steps"] == 0 and t["lanczos_block_steps"] == 0, t
    _, _, _, t = run(P, O, "full-but-one-32")
    assert t["eig_method"] == 2 and t["lanczos_steps"] == 0 and t["lanczos_block_steps"] == 0, t


@pytest.mark.parametrize("n", [64, 1028])
def test_breakdown_on_a_rank_3_matrix(P, O, n):
    """rank(B) = 3 < 12 steps: the Krylov space is exhausted before the first check.  `auto` returns verified pairs,
    whichever method answers; `lanczos` returns pairs that pass or PCOA_ERR_NOT_CONVERGED, never pairs that fail."""
    run(P, O, "rank3-%d" % n)
    sp = spectrum("rank3-lanczos-%d" % n)
    try:
        comps, lam, t = solve(P, sp, "lanczos")
    except P.PcoaError as exc:
        assert exc.code == PCOA_ERR_NOT_CONVERGED, exc
        print("LANCZOS_EIG " + json.dumps({"case": "rank3-lanczos-%d" % n, "n": n, "k": sp.k, "not_converged": True}))
        return
    assert t["eig_method"] == 1, t
    check(O, "rank3-lanczos-%d" % n, sp, comps, lam, t)


@pytest.mark.parametrize("n", [260, 1025])
def test_negative_dominant_spectrum_is_ranked_by_magnitude(P, O, n):
    _, _, lam, t = run(P, O, "negative-dominant-%d" % n)
    assert t["eig_method"] == 1 and t["matvec_form"] == 0, t
    assert np.all(lam < 0) and np.all(np.diff(np.abs(lam)) <= 0), lam


def test_int64_part_live(P, O):
    sp, _, _, t = run(P, O, "int64-1028")
    assert np.abs(sp.s).max() >= 2 ** 31
    assert t["eig_method"] == 1 and t["gram_i64_live"] == 1 and t["matvec_form"] == 0, t


def test_exact_multiplicity_2(P, O):
    """The leading eigenvalue has multiplicity 2 exactly: the cluster's subspace is checked (check_pairs), under `auto` and
    with the band iteration from the start.  In exact arithmetic a single start vector holds one direction of that eigenspace
    and the iteration breaks down after four steps (B has four distinct eigenvalues).  In fp64 lanczos_finish_kernel
    normalises whatever CGS2 left of w (`rn = (nrm > 0.0) ? 1.0 / nrm : 0.0; vn[i] = w[i] * rn`, eig_lanczos.hip:632-634): the
    rounding residue restarts the iteration in the complement, which holds the second direction, and the check at m = 12
    accepts both copies on their true residual at the fp64 floor (`r <= 1e-13 * scale`, :936).  So `auto` is not asserted to
    reach the band iteration here: whichever iteration answers, its pairs must pass, and the line reports it."""
    sp, _, _, t = run(P, O, "multiplicity2-1028")
    assert ([0, 1], True) in sp.groups and t["eig_method"] == 1, t
    _, _, _, t = run(P, O, "multiplicity2-band-1028")
    assert t["eig_method"] == 1 and t["lanczos_steps"] == 0 and t["lanczos_block_steps"] > 0, t


def test_near_tie(P, O):
    """Two leading eigenvalues within a relative 1e-9: verified pairs, the cluster's subspace checked; the line reports
    which iteration returned them."""
    sp, _, _, t = run(P, O, "near-tie-1028")
    assert sp.groups == [([0, 1], True)] and t["eig_method"] in (1, 2), t


def test_caller_supplied_product(P, O):
    """pcoa_lanczos_with_matvec over the host product: the same bars, eigenvalues within 1e-12 ||B|| of the built-in one's."""
    import torch
    sp, eig = spectrum("planted-257"), CASES["planted-257"][1]
    _, lam_builtin, _ = solve(P, sp, eig)
    host = E.centred_matmul_host(sp.s.astype(np.float64))

    def matvec(v):
        return torch.from_numpy(host(v.cpu().numpy()[:, None])[:, 0]).to(v.device)

    with P.PcoaEngine(sp.n, eig=eig) as eng:
        comps, lam = eng.lanczos(matvec, sp.k)
        t = eng.timings()
    assert t["eig_method"] == 1 and t["lanczos_block_steps"] == 0 and t["lanczos_steps"] in schedule(sp.n, sp.k), t
    check(O, "planted-257-caller-product", sp, comps, lam, t)
    assert np.all(np.abs(lam - lam_builtin) <= 1e-12 * sp.norm), (lam, lam_builtin)


# ----------------------------------------------------------------------------------------------------- child processes
def child_main(argv):
    out_dir, names = argv[0], argv[1].split(",")
    P, O = load_pkg(), load_oracle()
    for case in names:
        eig = CASES[case][1]
        t0 = time.time()
        sp = spectrum(case)
        rec = {"case": case}
        try:
            comps, lam, t = solve(P, sp, eig)
            np.savez(os.path.join(out_dir, case + ".npz"), comps=comps, lam=lam)
            rec.update(dict((key, int(t[key])) for key in COUNTERS))
            rec.update(check(O, case, sp, comps, lam, t, time.time() - t0))
        except P.PcoaError as exc:
            rec["error"] = "PcoaError %d: %s" % (exc.code, exc)
        except AssertionError as exc:
            rec["error"] = "AssertionError: %s" % exc
        print(json.dumps(rec))
        sys.stdout.flush()


_RUNS = {}
_FAULTED = []


@pytest.fixture(scope="module")
def out_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("lanczos_bands"))


def _run_env(name, out_dir):
    """One child per environment, once per session, never retried; after a child that died of a signal or ran out of time
    nothing more is started on the GPU from this module."""
    if name in _RUNS:
        return _RUNS[name]
    cases, knobs, limit = ENVS[name]
    if _FAULTED:
        pytest.fail("not started: an earlier child of this module ended abnormally (%s)" % _FAULTED[0])
    where = os.path.join(out_dir, name)
    os.makedirs(where)
    cmd = [sys.executable, os.path.abspath(__file__), where, ",".join(cases)]
    t0 = time.time()
    try:
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                             env=dict(os.environ, **knobs), timeout=limit)
    except subprocess.TimeoutExpired as e:
        _FAULTED.append("%s: time limit %d s" % (name, limit))
        _RUNS[name] = {"error": "child exceeded its time limit of %d s; stdout so far:\n%s" % (limit, e.stdout)}
        return _RUNS[name]
    print("child '%s': %.1f s" % (name, time.time() - t0))
    for line in res.stdout.splitlines():
        if line.startswith("LANCZOS_EIG "):
            print("LANCZOS_EIG " + json.dumps(dict(json.loads(line[12:]), env=name)))
    run = {"cases": dict((d["case"], d) for d in (json.loads(s) for s in res.stdout.splitlines() if s.startswith("{"))),
           "dir": where}
    if res.returncode != 0:
        if res.returncode < 0 or res.returncode in (134, 139):
            _FAULTED.append("%s: exit status %d" % (name, res.returncode))
        run["error"] = "child exited with status %d\n%s" % (res.returncode, res.stderr[-4000:])
    _RUNS[name] = run
    return run


def _case(env_name, case, out_dir):
    run = _run_env(env_name, out_dir)
    assert "error" not in run, run["error"]
    assert case in run["cases"], "no result for %s" % case
    r = run["cases"][case]
    assert "error" not in r, "%s in '%s': %s" % (case, env_name, r["error"])
    pairs = np.load(os.path.join(run["dir"], case + ".npz"))
    return r, pairs["comps"], pairs["lam"]


def _same_pairs(sp, a, b, tol):
    """Eigenvalues within tol ||B||; isolated vectors within tol, a cluster returned whole as its subspace."""
    (ca, la), (cb, lb) = a, b
    assert np.all(np.abs(la - lb) <= tol * sp.norm), (la, lb)
    for members, whole in sp.groups:
        if len(members) == 1:
            t = members[0]
            u = ca[:, t] if ca[:, t] @ cb[:, t] >= 0 else -ca[:, t]
            d = float(np.linalg.norm(u - cb[:, t]))
        else:
            assert whole
            u, v = ca[:, members], cb[:, members]
            d = float(np.linalg.norm(u - v @ (v.T @ u), 2))
        assert d <= tol, "PC%s differ by %.3g" % ([t + 1 for t in members], d)


@pytest.mark.parametrize("case", ENVS["default"][0])
def test_default_environment_takes_the_row_form(out_dir, case):
    """The cases of the other environments in a child without a knob: what they are compared with."""
    d, _, _ = _case("default", case, out_dir)
    assert d["matvec_form"] == 0 and d["eig_method"] == 1 and d["gram_i64_live"] == 0, d


@pytest.mark.parametrize("case", SYM_CASES)
def test_upper_triangle_form_forced_at_small_n(out_dir, case):
    """PCOA_SYMV_SYM_MIN_N=4: row sums and mat-vec from the upper-triangular tiles; the pairs pass the bars (in the child) and
    equal those of the default forms to 1e-12."""
    r, comps, lam = _case("upper_triangle", case, out_dir)
    assert r["matvec_form"] == 1 and r["eig_method"] == 1 and r["gram_i64_live"] == 0, r
    d, dcomps, dlam = _case("default", case, out_dir)
    assert d["matvec_form"] == 0 and d["eig_method"] == 1, d
    _same_pairs(spectrum(case), (comps, lam), (dcomps, dlam), 1e-12)


def test_band_iteration_with_thick_restarts(out_dir):
    """PCOA_LANCZOS_BAND=2, PCOA_LANCZOS_BAND_MMAX=40: only the band iteration, with a basis of 40 vectors of which 8 stay
    free for a restart.  A full-rank spectrum needs more columns than the basis holds: thick restarts."""
    r, _, _ = _case("band_restarts", "noisy-1028", out_dir)
    assert r["eig_method"] == 1 and r["lanczos_steps"] == 0, r
    assert r["lanczos_block_steps"] > BAND_MMAX, "no thick restart: %s" % r


def test_band_iteration_exhausts_an_invariant_subspace(out_dir):
    """The same environment on the exact multiplicity: B = c J + Z^T C Z has the eigenvalues lambda_1 (twice), lambda_3, c
    (N - 4 times) and 0, so the k + 2 = 4 start vectors span an invariant subspace of 3 (range of Z^T) + 1 (the constant
    vector) + 4 (one vector of the c-eigenspace each) = 8 dimensions.  Every later candidate vanishes against the basis
    and is deflated (`nrm > 1e-9 * anorm`, eig_lanczos.hip:1074), and after 8 columns `exhausted = (J == cnt)` (:1078)
    ends the iteration on exact pairs: no restart can happen, and lanczos_block_steps is 8, not more than 40."""
    r, _, _ = _case("band_restarts", "multiplicity2-1028-k2", out_dir)
    assert r["eig_method"] == 1 and r["lanczos_steps"] == 0, r
    assert r["lanczos_block_steps"] == 3 + 1 + (r["k"] + 2), r


def test_explicit_b_is_bit_identical_to_the_implicit_form(out_dir):
    r, comps, lam = _case("explicit_b", "planted-257", out_dir)
    assert r["matvec_form"] == 2 and r["eig_method"] == 1, r
    d, dcomps, dlam = _case("default", "planted-257", out_dir)
    assert d["matvec_form"] == 0 and d["eig_method"] == 1 and d["lanczos_steps"] == r["lanczos_steps"], (d, r)
    assert np.array_equal(comps, dcomps) and np.array_equal(lam, dlam)


if __name__ == "__main__":
    child_main(sys.argv[1:])

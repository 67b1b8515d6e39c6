"""The similarity measures on the GPU (pcoa_set_similarity; csrc/measure.hip): every kernel of the new family held to the
numpy rules of variants_pca.similarity_measure / centred_measure, at the sample counts where its loops change path.

EXACT cases: measure_cohort.exact_groups, whose K is in {0, 1} and whose B is in {0.75, -0.25} under both measures.  For an
integer x every partial sum of B x is a multiple of 0.25 far below 2^53, so every form, in every order of addition, must
return the numpy product bit for bit (np.array_equal).  Sample counts, by what they reach:
  form 1 (measure_symv_sym_tiles_kernel; the row sums from its uncentred twin): 4, 64, 1020 the corner tile alone; 1024, 2048
    no ragged tile; 1028, 1044 ragged tiles of 4 and 20 rows; 1540, 2044 the quad-group mask edges; 2052 interior + ragged +
    corner; 3076 the interior index loop with bi > 0
  forms 0 and 2 (measure_symv_rows_kernel over S, symv_kernel over the B of measure_center_kernel): 16-byte loads around the
    ends of row_dot's main loop (j + 768 < n)

ROUNDED cases: measure_cohort.populations (d_i varies about 3x, two samples empty), against the rule evaluated in
np.longdouble from the integer S read back from the engine.
  entries    |B - ref| <= (4 N + 32) 2^-53 per entry: |K| <= 1 with at most 4 roundings (a division that need not be correctly
             rounded, or two products and q's own rounding); a row sum of N terms <= 1 in any order errs by at most
             N^2 2^-53, hence N 2^-53 on a mean; the matrix mean errs by the same order again; three add / subtracts on
             magnitudes <= 2.  A wrong d_j, a dropped term or a misplaced column is 10^6 or more times larger.
             Row sums within N^2 2^-53; nonzero_rows equal.
  mat-vec    |y_i - ref_i| <= N 2^-52 (|B| |x|)_i + (4 N + 32) 2^-53 ||x||_1: the summation bound of
             test_gpu_centred_matvec_forms.py plus the entry bound above.
  eigenpairs against numpy.linalg.eigh of the reference B: eigenvalues within 1e-6 relative, vectors within 1e-6 up to sign
             (the project's bar against the oracle); measure_cohort asserts the relative gaps that condition them.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import measure_cohort as M  # noqa: E402
from conftest import int_gram, load_golden, load_pkg  # noqa: E402

pytestmark = pytest.mark.gpu

PCOA_ERR_INVALID_ARG, PCOA_ERR_STATE = -1, -8
PCOA_FLAG_EIG_HOUSEHOLDER = 0x20
CHILD_LIMIT = 30              # seconds: about 10x what a child takes on an idle MI355X, start-up included


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def I():
    return load_pkg("ingest")


def feed_bits(I, eng, x):
    eng.accumulate_bits(I.pack_bits(x))


def _mismatch(n, kind, form, what, got, want):
    bad = np.nonzero(got != want)[0]
    i = int(bad[0])
    return "N = %d, %s, form %d, %s: %d of %d entries differ; first y[%d] = %r, want %r (rows %s ..)" % (
        n, kind, form, what, bad.size, n, i, float(got[i]), float(want[i]), bad[:8].tolist())


# ------------------------------------------------------------------------------------------------------- 1. exact, every form
def _check_exact(P, I, n, forms):
    with P.PcoaEngine(n) as eng:
        feed_bits(I, eng, M.exact_groups(n))
        for kind in M.MEASURES:
            s, b, xs, ref = M.exact_case(n, kind)
            eng.set_similarity(kind)
            assert eng.get_similarity() == kind
            for form in forms:
                for v in range(xs.shape[0]):
                    y = eng.debug_centred_matvec(xs[v], form)
                    assert np.array_equal(y, ref[:, v]), _mismatch(n, kind, form, "integer x %d" % v, y, ref[:, v])
                y = eng.debug_centred_matvec(np.ones(n), form)
                assert not y.any(), _mismatch(n, kind, form, "B 1", y, np.zeros(n))
            got_b, rs, nz, mm = eng.center()
            assert np.array_equal(got_b, b), "N = %d, %s: center() differs from {0.75, -0.25} in %d entries" % (n, kind, int((got_b != b).sum()))
            assert np.all(rs == n / 4) and mm == 0.25 and nz == n
        assert np.array_equal(eng.gram(), s)


@pytest.mark.parametrize("n", M.EXACT_TILE_N)
def test_exact_cohort_upper_triangle_and_row_forms(P, I, n):
    _check_exact(P, I, n, (1, 0, 2))


@pytest.mark.parametrize("n", [n for n in M.EXACT_ROW_N if n not in M.EXACT_TILE_N])
def test_exact_cohort_row_forms(P, I, n):
    _check_exact(P, I, n, (0, 2))


# ------------------------------------------------------------------------------------------------------- 2. / 3. rounded
def rounded_engine(P, n):
    x8 = M.populations(n, M.ROUNDED_V, empty=M.EMPTY).astype(np.uint8)
    eng = P.PcoaEngine(n)
    eng.accumulate_dense_u8(x8)
    return eng


def _check_entries(eng, n, kind, s_ref):
    """center() of the engine (measure already set) against the long-double reference from s_ref."""
    ref_b, ref_r, ref_mm, ref_nz = M.reference(s_ref, kind)
    got_b, rs, nz, mm = eng.center()
    err = np.abs((got_b.astype(np.longdouble) - ref_b).astype(np.float64))
    worst = np.unravel_index(int(np.argmax(err)), err.shape)
    rerr = float(np.abs((rs.astype(np.longdouble) - ref_r).astype(np.float64)).max())
    print("N = %d, %s: max |B - ref| = %.3g (bound %.3g) at %s; max |r - ref| = %.3g (bound %.3g); |mm - ref| = %.3g" % (
        n, kind, err[worst], M.entry_bound(n), worst, rerr, M.row_sum_bound(n), abs(float(np.longdouble(mm) - ref_mm))))
    assert err[worst] <= M.entry_bound(n), "N = %d, %s: |B - ref| = %.3g > %.3g at %s" % (n, kind, err[worst], M.entry_bound(n), worst)
    assert rerr <= M.row_sum_bound(n)
    assert abs(float(np.longdouble(mm) - ref_mm)) <= M.entry_bound(n)
    assert nz == ref_nz
    return ref_b


@pytest.mark.parametrize("n", M.ROUNDED_N)
def test_rounded_entries_against_the_long_double_rule(P, n):
    """Scalar-load (N % 4 != 0) and quad-load row paths of the row-sum pass, and the dense centring."""
    with rounded_engine(P, n) as eng:
        s = eng.gram()
        assert np.array_equal(s, int_gram(M.populations(n, M.ROUNDED_V, empty=M.EMPTY)))
        for kind in M.MEASURES:
            eng.set_similarity(kind)
            _check_entries(eng, n, kind, s)
            assert eng.center()[2] == n - 2                                       # two samples carry nothing


def _check_matvec(eng, n, kind, forms, ref_b, what=""):
    bl = ref_b
    ab = np.abs(ref_b.astype(np.float64))
    vectors = []
    for k in M.edge_columns(n):
        e = np.zeros(n)
        e[k] = 1.0
        vectors.append(("column %d" % k, e))
    vectors.append(("gaussian", np.random.default_rng(n).standard_normal(n)))
    for name, xv in vectors:
        ref = bl @ xv.astype(np.longdouble)
        bound = M.matvec_bound(n, ab, xv)
        for form in forms:
            y = eng.debug_centred_matvec(xv, form)
            err = np.abs((y.astype(np.longdouble) - ref).astype(np.float64))
            worst = int(np.argmax(err / bound))
            if name == "gaussian":
                print("N = %d, %s%s, form %d: max |y - ref| / bound = %.3g (row %d)" % (n, kind, what, form, err[worst] / bound[worst], worst))
            assert np.all(err <= bound), "N = %d, %s%s, form %d, %s: |y - ref| = %.3g > %.3g at row %d" % (
                n, kind, what, form, name, err[worst], bound[worst], worst)


@pytest.mark.parametrize("n", M.ROUNDED_N)
def test_rounded_matvec_every_form(P, n):
    forms = (0, 1, 2) if n % 4 == 0 else (0, 2)
    with rounded_engine(P, n) as eng:
        s = eng.gram()
        for kind in M.MEASURES:
            eng.set_similarity(kind)
            _check_matvec(eng, n, kind, forms, M.reference(s, kind)[0])
        if n % 4:
            with pytest.raises(P.PcoaError) as err:
                eng.debug_centred_matvec(np.ones(n), 1)
            assert err.value.code == PCOA_ERR_STATE


# ------------------------------------------------------------------------------------------------------- 4. int64 part live
@pytest.mark.parametrize("n", M.I64_N)
def test_int64_part_live(P, n):
    """2^22 S leaves int32: the HAS64 row kernels and the s64 branches of the diagonal and the dense centring.  Both measures
    are scale-invariant, so the reference is the UNSCALED S's."""
    s = int_gram(M.populations(n, M.I64_V, empty=M.EMPTY))
    assert (s * M.I64_SCALE).max() >= 2 ** 31
    with P.PcoaEngine(n) as eng:
        eng.load_gram(s * M.I64_SCALE)
        assert eng.timings()["gram_i64_live"] == 1
        for kind in M.MEASURES:
            eng.set_similarity(kind)
            ref_b = _check_entries(eng, n, kind, s)
            _check_matvec(eng, n, kind, (0,), ref_b, " (int64)")
            with pytest.raises(P.PcoaError) as err:
                eng.debug_centred_matvec(np.ones(n), 1)
            assert err.value.code == PCOA_ERR_STATE


# ------------------------------------------------------------------------------------------------------- 5. eigenpairs
def eig_check(comps, lam, nz, s, kind):
    """'' or what differs from numpy.linalg.eigh of the reference B."""
    n = s.shape[0]
    w, z, b, gaps = M.eig_reference(s, kind)
    bad = []
    if nz != n:
        bad.append("nonzero_rows = %d, want %d" % (nz, n))
    rel = np.abs(lam - w) / np.abs(w)
    if not np.all(rel <= 1e-6):
        bad.append("eigenvalues %s, want %s" % (lam.tolist(), w.tolist()))
    for c in range(M.NUM_PC):
        a = comps[:, c] if np.dot(comps[:, c], z[:, c]) >= 0 else -comps[:, c]
        d = float(np.linalg.norm(a - z[:, c]))
        if not d < 1e-6:
            bad.append("PC%d differs by %.3g" % (c + 1, d))
    return "; ".join(bad)


def eig_run(P, n, kind, flags=0):
    x8 = M.eig_cohort(n).astype(np.uint8)
    with P.PcoaEngine(n, flags=flags) as eng:
        eng.accumulate_dense_u8(x8)
        eng.set_similarity(kind)
        comps, lam, nz = eng.compute(M.NUM_PC)
        t = eng.timings()
        s = eng.gram()
    return eig_check(comps, lam, nz, s, kind), int(t["eig_method"]), int(t["matvec_form"]), int(t["lanczos_steps"])


@pytest.mark.parametrize("kind", M.MEASURES)
@pytest.mark.parametrize("n,flags,method,form", [(6, 0, 2, None), (20, 0, 2, None), (260, 0, 1, 0), (1025, 0, 1, 0),
                                                 (1025, PCOA_FLAG_EIG_HOUSEHOLDER, 2, None)])
def test_eigenpairs_in_process(P, n, flags, method, form, kind):
    bad, eig_method, matvec_form, steps = eig_run(P, n, kind, flags)
    print("N = %d, %s: eig_method %d, matvec_form %d, %d Lanczos steps" % (n, kind, eig_method, matvec_form, steps))
    assert eig_method == method and (form is None or matvec_form == form)
    assert not bad, bad


def child_main(argv):
    """One (n, kind) per argument with the knobs of the parent's environment: one JSON line each."""
    P = load_pkg()
    for arg in argv:
        n, kind = arg.split(":")
        bad, eig_method, matvec_form, steps = eig_run(P, int(n), kind)
        print(json.dumps({"n": int(n), "kind": kind, "bad": bad, "eig_method": eig_method, "matvec_form": matvec_form}))
        sys.stdout.flush()


_CHILD = {}


def _child(env_name, n):
    """The child for one knob, once per session, never retried."""
    if env_name in _CHILD:
        return _CHILD[env_name]
    out = _CHILD[env_name] = {}
    env = dict(os.environ, **{env_name: "1024" if env_name == "PCOA_SYMV_SYM_MIN_N" else "1"})
    cmd = [sys.executable, os.path.abspath(__file__)] + ["%d:%s" % (n, kind) for kind in M.MEASURES]
    try:
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env, timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired as e:
        out["error"] = "child exceeded its time limit of %d s; stdout so far:\n%s" % (CHILD_LIMIT, e.stdout)
        return out
    out["cases"] = dict((d["kind"], d) for d in (json.loads(t) for t in res.stdout.splitlines() if t.startswith("{")))
    if res.returncode != 0:
        out["error"] = "child exited with status %d\n%s" % (res.returncode, res.stderr[-4000:])
    return out


@pytest.mark.parametrize("kind", M.MEASURES)
@pytest.mark.parametrize("env_name,n,form", [("PCOA_SYMV_SYM_MIN_N", 2052, 1), ("PCOA_EXPLICIT_CENTER", 260, 2)])
def test_eigenpairs_in_a_child(env_name, n, form, kind):
    """PCOA_SYMV_SYM_MIN_N=1024 at N = 2052: the upper-triangle mat-vec with the fp64 row sums of the tile pass;
    PCOA_EXPLICIT_CENTER=1 at N = 260: Lanczos over the materialised B.  (The knobs are read once: a child each.)"""
    run = _child(env_name, n)
    assert "error" not in run, run["error"]
    assert kind in run["cases"], "no result for %s" % kind
    r = run["cases"][kind]
    assert r["eig_method"] == 1 and r["matvec_form"] == form, r
    assert not r["bad"], r["bad"]


# ------------------------------------------------------------------------------------------------------- 6. the setting
def test_get_returns_what_set_stored_and_it_survives_reset(P):
    n = 67
    x8 = M.populations(n, 300).astype(np.uint8)
    with P.PcoaEngine(n) as eng:
        assert eng.get_similarity() == "shared"
        for kind in ("jaccard", "cosine", "shared", "cosine"):
            eng.set_similarity(kind)
            assert eng.get_similarity() == kind
        eng.set_similarity(1)
        assert eng.get_similarity() == "jaccard"
        eng.accumulate_dense_u8(x8)
        before = eng.compute(2)
        eng.reset()
        assert eng.get_similarity() == "jaccard" and not eng.gram().any()
        eng.accumulate_dense_u8(x8)
        after = eng.compute(2)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        for bad_kind in (3, -1, 99):
            with pytest.raises(P.PcoaError) as err:
                eng.set_similarity(bad_kind)
            assert err.value.code == PCOA_ERR_INVALID_ARG and "pcoa_set_similarity" in str(err.value)
            assert eng.get_similarity() == "jaccard"
        with pytest.raises(ValueError):
            eng.set_similarity("dice")


@pytest.mark.parametrize("kind", M.MEASURES)
def test_a_subset_inherits_the_measure(P, kind):
    n = 260
    x8 = M.eig_cohort(n).astype(np.uint8)
    keep = np.setdiff1d(np.arange(n), np.arange(5, n, 9))
    with P.PcoaEngine(n) as eng, P.PcoaEngine(keep.size) as fresh:
        eng.accumulate_dense_u8(x8)
        eng.set_similarity(kind)
        sub = eng.subset(keep)
        try:
            assert sub.get_similarity() == kind
            c1, l1, nz1 = sub.compute(2)
        finally:
            sub.close()
        fresh.accumulate_dense_u8(np.ascontiguousarray(x8[:, keep]))
        fresh.set_similarity(kind)
        c2, l2, nz2 = fresh.compute(2)
        assert nz1 == nz2 == keep.size
        assert np.all(np.abs(l1 - l2) <= 1e-6 * np.abs(l2))
        for c in range(2):
            a = c1[:, c] if np.dot(c1[:, c], c2[:, c]) >= 0 else -c1[:, c]
            assert np.linalg.norm(a - c2[:, c]) < 1e-6
        assert not eig_check(c2, l2, nz2, int_gram(x8[:, keep]), kind)


def _shared_results(eng):
    comps, lam, nz = eng.compute(2)
    b, rs, nzc, mm = eng.center()
    return comps, lam, nz, b, rs, nzc, mm


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_switching_back_to_shared_returns_the_same_bits(P):
    n = 1044
    x8 = M.populations(n, 400).astype(np.uint8)
    with P.PcoaEngine(n) as never, P.PcoaEngine(n) as eng:
        never.accumulate_dense_u8(x8)
        eng.accumulate_dense_u8(x8)
        want = _shared_results(never)
        eng.set_similarity("jaccard")
        measured = eng.compute(2)
        assert not np.array_equal(measured[1], want[1])                           # it did decompose something else
        eng.debug_centred_matvec(np.ones(n), 1)
        eng.set_similarity("shared")
        assert _same_bits(_shared_results(eng), want)


def test_strip_owner_and_operator_refuse_a_measure_and_stay_usable(P, I):
    n = 64
    x = M.populations(n, 200)
    with P.PcoaEngine(n, strip=(0, n)) as strip, P.PcoaEngine(n, operator=True) as op, P.PcoaEngine(n) as full:
        for eng, word in ((strip, "strip owner"), (op, "operator ctx")):
            for kind in M.MEASURES:
                with pytest.raises(P.PcoaError) as err:
                    eng.set_similarity(kind)
                assert err.value.code == PCOA_ERR_STATE and word in str(err.value), str(err.value)
            eng.set_similarity("shared")                                          # the default is theirs to set
            assert eng.get_similarity() == "shared"
        bits = I.pack_bits(x)
        for eng in (strip, op, full):
            eng.accumulate_bits(bits)
        want = full.compute(2)
        got_op = op.compute(2)
        assert np.all(np.abs(got_op[1] - want[1]) <= 1e-6 * np.abs(want[1])) and got_op[2] == want[2]
        got_strip = load_pkg("engine").compute_strips([strip], 2)
        assert np.all(np.abs(got_strip[1] - want[1]) <= 1e-6 * np.abs(want[1]))


def test_project_against_a_measured_ref_is_refused(P):
    n_ref, n = 40, 52
    x8 = M.populations(n, 300).astype(np.uint8)
    with P.PcoaEngine(n_ref) as ref, P.PcoaEngine(n, strip=(n_ref, n - n_ref)) as cross:
        ref.accumulate_dense_u8(np.ascontiguousarray(x8[:, :n_ref]))
        cross.accumulate_dense_u8(x8)
        ref.set_similarity("jaccard")
        comps, lam, _ = ref.compute(2)
        with pytest.raises(P.PcoaError) as err:
            ref.project(cross, comps, lam)
        assert err.value.code == PCOA_ERR_STATE and "not built" in str(err.value)
        ref.set_similarity("shared")
        comps, lam, _ = ref.compute(2)
        assert ref.project(cross, comps, lam).shape == (n - n_ref, 2)             # both engines still serve


def test_the_screen_does_not_look_at_the_measure(P):
    import related_cohort as R
    n = 260
    x8 = R.related_cohort(n, 2000).astype(np.uint8)
    with P.PcoaEngine(n) as eng:
        eng.accumulate_dense_u8(x8)
        plain = eng.similar_pairs(R.THRESHOLD)
        for kind in M.MEASURES:
            eng.set_similarity(kind)
            eng.compute(2)
            got = eng.similar_pairs(R.THRESHOLD)
            assert np.array_equal(got[0], plain[0]) and got[1] == plain[1] and np.array_equal(got[2], plain[2])
        assert [(int(p["i"]), int(p["j"])) for p in plain[0]] == R.planted_pairs(n)


# ------------------------------------------------------------------------------------------------------- 7. default untouched
@pytest.mark.parametrize("case", ["pops40", "n1044"])
def test_explicit_shared_is_the_default_bit_for_bit(P, case):
    """Passes before and after the measures exist (where the call is missing, the explicit engine is the default engine)."""
    with_call = hasattr(P.PcoaEngine, "set_similarity")
    if case == "pops40":
        g = load_golden("pops40")
        n = int(g["n_samples"])
        feed = lambda eng: eng.accumulate_calls(g["sample_idx"], g["row_offsets"])
    else:
        n = 1044
        x8 = M.populations(n, 400).astype(np.uint8)
        feed = lambda eng: eng.accumulate_dense_u8(x8)
    with P.PcoaEngine(n) as never, P.PcoaEngine(n) as explicit:
        feed(never)
        feed(explicit)
        if with_call:
            explicit.set_similarity("shared")
        assert _same_bits(_shared_results(explicit), _shared_results(never))
        if case == "pops40":
            assert np.array_equal(never.center()[0], g["centered"])


# ------------------------------------------------------------------------------------------------------- 8. both hosts
@pytest.fixture(scope="module")
def host_cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("measurehosts")
    x = M.eig_cohort(M.HOST_N)
    names = [M.name_of(i) for i in range(M.HOST_N)]
    M.write_vcf(x, str(d / "cohort.vcf"), names)
    return {"vcf": str(d / "cohort.vcf"), "s": int_gram(x), "names": names}


_runs = {}


def run_once(host, path, extra=()):
    key = (host, path, tuple(extra))
    if key not in _runs:
        _runs[key] = (M.run_driver if host == "driver" else M.run_python)(["--input-path", path] + list(extra))
    return _runs[key]


@pytest.mark.parametrize("kind", M.MEASURES)
def test_both_hosts_end_to_end(host_cohort, kind):
    extra = ("--similarity-measure", kind)
    a = run_once("driver", host_cohort["vcf"], extra)
    b = run_once("python", host_cohort["vcf"], extra)
    assert a.returncode == 0, a.stderr
    assert b.returncode == 0, b.stderr
    assert a.stdout.encode() == b.stdout.encode()
    assert "Non zero rows in matrix: %d / %d." % (M.HOST_N, M.HOST_N) in a.stdout
    rows = [ln.split("\t") for ln in a.stdout.splitlines() if ln.count("\t") == 3]
    assert [r[0] for r in rows] == host_cohort["names"]
    got = np.array([[float(r[2]), float(r[3])] for r in rows])
    w, z, _, _ = M.eig_reference(host_cohort["s"], kind)
    for c in range(2):
        col = got[:, c] if np.dot(got[:, c], z[:, c]) >= 0 else -got[:, c]
        assert np.linalg.norm(col - z[:, c]) < 1e-6
    plain = run_once("driver", host_cohort["vcf"])
    assert plain.returncode == 0 and plain.stdout != a.stdout                     # the measure changed the coordinates


@pytest.mark.parametrize("host", ["driver", "python"])
def test_shared_is_a_run_without_the_flag(host_cohort, host):
    a = run_once(host, host_cohort["vcf"], ("--similarity-measure", "shared"))
    b = run_once(host, host_cohort["vcf"])
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    assert a.stdout.encode() == b.stdout.encode()


if __name__ == "__main__":
    child_main(sys.argv[1:])

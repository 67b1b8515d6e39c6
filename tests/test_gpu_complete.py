"""The pairwise-complete similarity on the GPU (pcoa_set_call_companion, pcoa_accumulate_plink_bed_calls; csrc/complete.hip):
every kernel of the new family held to the numpy rule variants_pca.call_complete_measure / centred_measure, at the sample
counts where its loops change path (the shapes are measure_cohort's, for the twins of its kernels).

DECODE: random 2-bit codes, the padding pairs of the last byte set to 01: S must be bit-identical to an engine fed by
pcoa_accumulate_plink_bed alone and Q to the numpy Gram of code == 01, for host rows, device rows with a wider pitch, pinned
queued rows, and calls of 37 rows.

EXACT cases: complete_cohort.exact_calls, K in {0, kappa}, B in {0.75 kappa, -0.25 kappa}, kappa = 1 / (1 + extra) in
{1, 1/2, 1/4}: every form, in every order of addition, must return the numpy product bit for bit.  extra = 0 puts the M > 0
guard on 3/4 of the entries.

ROUNDED cases: complete_cohort.populations_with_missing, against the rule evaluated in np.longdouble.  s <= M, so |K| <= 1
with one division and exact integer conversions: measure_cohort's entry_bound, row_sum_bound and matvec_bound apply unchanged.
With the carrier engine's int64 part live S is loaded as 2^22 S: a power of two scales K, the row sums, the means and B
exactly (no operation rounds differently), so the device's results divided by 2^22 are held to the same bounds against the
reference of the unscaled S.

EIGENPAIRS against numpy.linalg.eigh of the reference B: 1e-6 relative on the eigenvalues, 1e-6 on the vectors up to sign."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import complete_cohort as C  # noqa: E402
from conftest import int_gram, load_pkg  # noqa: E402

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


def feed_pair(I, eng, q, carriers, missing):
    eng.accumulate_bits(I.pack_bits(carriers))
    q.accumulate_bits(I.pack_bits(missing))


# ------------------------------------------------------------------------------------------------------- 1. decode + accumulate
@pytest.mark.parametrize("ref_is_a1", [False, True])
@pytest.mark.parametrize("v", C.DECODE_V)
@pytest.mark.parametrize("n", C.DECODE_N)
def test_pair_decode_and_accumulate(P, n, v, ref_is_a1):
    import torch
    rows = C.random_codes(n, v, seed=1000 * n + v)
    carriers, missing = C.decode_pair(rows, n, ref_is_a1)
    want_s, want_q = int_gram(carriers), int_gram(missing)
    nb = rows.shape[1]
    with P.PcoaEngine(n) as alone, P.PcoaEngine(n) as eng, P.PcoaEngine(n) as q:
        alone.accumulate_plink_bed(rows, ref_is_a1=ref_is_a1)
        s_alone = alone.gram()
        assert np.array_equal(s_alone, want_s)

        def check(what):
            s, qq = eng.gram(), q.gram()
            assert np.array_equal(s, s_alone), "N = %d, V = %d, %s: S differs from pcoa_accumulate_plink_bed's in %d entries" % (
                n, v, what, int((s != s_alone).sum()))
            assert np.array_equal(qq, want_q), "N = %d, V = %d, %s: Q differs from the Gram of code == 01 in %d entries" % (
                n, v, what, int((qq != want_q).sum()))
            eng.reset()
            q.reset()

        eng.accumulate_plink_bed_calls(rows, q, ref_is_a1=ref_is_a1)
        check("host rows")
        wide = np.random.default_rng(n + v).integers(0, 256, size=(v, nb + 5), dtype=np.uint8)   # what lies behind a row is not its own
        wide[:, :nb] = rows
        dev = torch.from_numpy(wide).cuda()
        eng.accumulate_plink_bed_calls(dev[:, :nb], q, ref_is_a1=ref_is_a1)
        check("device rows, row_bytes = %d" % (nb + 5))
        pinned = torch.from_numpy(rows).pin_memory()
        eng.accumulate_plink_bed_calls(pinned, q, ref_is_a1=ref_is_a1, asynchronous=True)
        check("pinned queued rows")
        for v0 in range(0, v, C.DECODE_CALL_ROWS):
            eng.accumulate_plink_bed_calls(rows[v0:v0 + C.DECODE_CALL_ROWS], q, ref_is_a1=ref_is_a1)
        check("calls of %d rows" % C.DECODE_CALL_ROWS)
        del pinned, dev


def test_pair_accumulate_refuses_a_wrong_companion(P):
    n = 20
    rows = C.random_codes(n, 8, seed=1)
    with P.PcoaEngine(n) as eng, P.PcoaEngine(n + 1) as other_n, P.PcoaEngine(n, operator=True) as op, \
            P.PcoaEngine(n, gram_kernel="f32") as f32:
        for bad in (eng, other_n, op, f32):
            with pytest.raises(P.PcoaError) as err:
                eng.accumulate_plink_bed_calls(rows, bad)
            assert err.value.code == PCOA_ERR_INVALID_ARG and "pcoa_accumulate_plink_bed_calls" in str(err.value)
        assert not eng.gram().any()


# ------------------------------------------------------------------------------------------------------- 2. exact, every form
def _mismatch(n, extra, form, what, got, want):
    bad = np.nonzero(got != want)[0]
    i = int(bad[0])
    return "N = %d, extra = %d, form %d, %s: %d of %d entries differ; first y[%d] = %r, want %r (rows %s ..)" % (
        n, extra, form, what, bad.size, n, i, float(got[i]), float(want[i]), bad[:8].tolist())


def _check_exact(P, I, n, forms):
    with P.PcoaEngine(n) as eng, P.PcoaEngine(n) as q:
        for extra in C.EXTRAS:
            s, qq, v, b, xs, ref = C.exact_case(n, extra)
            carriers, missing, _ = C.exact_calls(n, extra)
            eng.reset()
            q.reset()
            feed_pair(I, eng, q, carriers, missing)
            eng.set_call_companion(q, v)
            kappa = 1.0 / (1 + extra)
            for form in forms:
                for k in range(xs.shape[0]):
                    y = eng.debug_centred_matvec(xs[k], form)
                    assert np.array_equal(y, ref[:, k]), _mismatch(n, extra, form, "integer x %d" % k, y, ref[:, k])
                y = eng.debug_centred_matvec(np.ones(n), form)
                assert not y.any(), _mismatch(n, extra, form, "B 1", y, np.zeros(n))
            got_b, rs, nz, mm = eng.center()
            assert np.array_equal(got_b, b), "N = %d, extra = %d: center() differs in %d entries" % (n, extra, int((got_b != b).sum()))
            assert np.all(rs == n * kappa / 4) and mm == kappa / 4 and nz == n
            assert np.array_equal(eng.gram(), s) and np.array_equal(q.gram(), qq)


@pytest.mark.parametrize("n", C.EXACT_TILE_N)
def test_exact_cohort_upper_triangle_and_row_forms(P, I, n):
    _check_exact(P, I, n, (1, 0, 2))


@pytest.mark.parametrize("n", [n for n in C.EXACT_ROW_N if n not in C.EXACT_TILE_N])
def test_exact_cohort_row_forms(P, I, n):
    _check_exact(P, I, n, (0, 2))


# ------------------------------------------------------------------------------------------------------- 3. rounded
ALL_MISSING, CALLED_EMPTY = (1,), (3,)      # both below the smallest N


def _check_entries(eng, n, s_ref, q_ref, v, scale=1.0, what=""):
    """center() of the bound engine against the long-double reference; scale: the power of two S was loaded with."""
    ref_b, ref_r, ref_mm, ref_nz = C.reference(s_ref, q_ref, v)
    got_b, rs, nz, mm = eng.center()
    got_b, rs, mm = got_b / scale, rs / scale, mm / scale
    err = np.abs((got_b.astype(np.longdouble) - ref_b).astype(np.float64))
    worst = np.unravel_index(int(np.argmax(err)), err.shape)
    rerr = float(np.abs((rs.astype(np.longdouble) - ref_r).astype(np.float64)).max())
    print("N = %d%s: max |B - ref| = %.3g (bound %.3g) at %s; max |r - ref| = %.3g (bound %.3g); |mm - ref| = %.3g" % (
        n, what, err[worst], C.entry_bound(n), worst, rerr, C.row_sum_bound(n), abs(float(np.longdouble(mm) - ref_mm))))
    assert err[worst] <= C.entry_bound(n), "N = %d%s: |B - ref| = %.3g > %.3g at %s" % (n, what, err[worst], C.entry_bound(n), worst)
    assert rerr <= C.row_sum_bound(n)
    assert abs(float(np.longdouble(mm) - ref_mm)) <= C.entry_bound(n)
    assert nz == ref_nz
    return ref_b, ref_nz


def _check_matvec(eng, n, forms, ref_b, scale=1.0, what=""):
    ab = np.abs(ref_b.astype(np.float64))
    vectors = []
    for k in C.edge_columns(n):
        e = np.zeros(n)
        e[k] = 1.0
        vectors.append(("column %d" % k, e))
    vectors.append(("gaussian", np.random.default_rng(n).standard_normal(n)))
    for name, xv in vectors:
        ref = ref_b @ xv.astype(np.longdouble)
        bound = C.matvec_bound(n, ab, xv)
        for form in forms:
            y = eng.debug_centred_matvec(xv, form) / scale
            err = np.abs((y.astype(np.longdouble) - ref).astype(np.float64))
            worst = int(np.argmax(err / bound))
            if name == "gaussian":
                print("N = %d%s, form %d: max |y - ref| / bound = %.3g (row %d)" % (n, what, form, err[worst] / bound[worst], worst))
            assert np.all(err <= bound), "N = %d%s, form %d, %s: |y - ref| = %.3g > %.3g at row %d" % (
                n, what, form, name, err[worst], bound[worst], worst)


@pytest.mark.parametrize("n", C.ROUNDED_N)
def test_rounded_entries_and_matvec_every_form(P, I, n):
    """Scalar-load (N % 4 != 0) and quad-load row paths, the tile form where N % 4 == 0, the dense centring; one sample without
    a single call (a zero row of K: M = 0 against everybody) and one called everywhere that carries nothing."""
    x, m, _ = C.populations_with_missing(n, C.ROUNDED_V, all_missing=ALL_MISSING, called_empty=CALLED_EMPTY)
    forms = (0, 1, 2) if n % 4 == 0 else (0, 2)
    with P.PcoaEngine(n) as eng, P.PcoaEngine(n) as q:
        feed_pair(I, eng, q, x, m)
        s, qq = eng.gram(), q.gram()
        assert np.array_equal(s, int_gram(x)) and np.array_equal(qq, int_gram(m))
        eng.set_call_companion(q, C.ROUNDED_V)
        ref_b, ref_nz = _check_entries(eng, n, s, qq, C.ROUNDED_V)
        assert ref_nz == n - 2 and eng.center()[2] == n - 2
        _check_matvec(eng, n, forms, ref_b)
        if n % 4:
            with pytest.raises(P.PcoaError) as err:
                eng.debug_centred_matvec(np.ones(n), 1)
            assert err.value.code == PCOA_ERR_STATE


@pytest.mark.parametrize("n", C.I64_N)
def test_int64_part_of_the_carrier_engine_live(P, I, n):
    """2^22 S leaves int32: the HAS64 row kernels and the s64 branch of the dense centring."""
    x, m, s, qq, v = C.i64_cohort(n)
    with P.PcoaEngine(n) as eng, P.PcoaEngine(n) as q:
        eng.load_gram(s * C.I64_SCALE)
        assert eng.timings()["gram_i64_live"] == 1
        q.accumulate_bits(I.pack_bits(m))
        assert np.array_equal(q.gram(), qq)
        eng.set_call_companion(q, v)
        ref_b, _ = _check_entries(eng, n, s, qq, v, scale=float(C.I64_SCALE), what=" (int64)")
        _check_matvec(eng, n, (0, 2), ref_b, scale=float(C.I64_SCALE), what=" (int64)")
        with pytest.raises(P.PcoaError) as err:
            eng.debug_centred_matvec(np.ones(n), 1)
        assert err.value.code == PCOA_ERR_STATE


# ------------------------------------------------------------------------------------------------------- 4. eigenpairs
def eig_check(comps, lam, nz, s, q, v):
    """'' or what differs from numpy.linalg.eigh of the reference B."""
    n = s.shape[0]
    w, z, b, gaps = C.eig_reference(s, q, v)
    bad = []
    if nz != n:
        bad.append("nonzero_rows = %d, want %d" % (nz, n))
    rel = np.abs(lam - w) / np.abs(w)
    if not np.all(rel <= 1e-6):
        bad.append("eigenvalues %s, want %s" % (lam.tolist(), w.tolist()))
    for c in range(C.NUM_PC):
        a = comps[:, c] if np.dot(comps[:, c], z[:, c]) >= 0 else -comps[:, c]
        d = float(np.linalg.norm(a - z[:, c]))
        if not d < 1e-6:
            bad.append("PC%d differs by %.3g" % (c + 1, d))
    return "; ".join(bad)


def eig_run(P, n, flags=0, eig=None):
    I = load_pkg("ingest")
    x, m = C.eig_cohort(n)
    v = x.shape[0]
    with P.PcoaEngine(n, flags=flags, eig=eig) as eng, P.PcoaEngine(n) as q:
        feed_pair(I, eng, q, x, m)
        eng.set_call_companion(q, v)
        comps, lam, nz = eng.compute(C.NUM_PC)
        t = eng.timings()
        s, qq = eng.gram(), q.gram()
    return (eig_check(comps, lam, nz, s, qq, v), int(t["eig_method"]), int(t["matvec_form"]), int(t["lanczos_steps"]),
            int(t.get("lanczos_block_steps", 0)))


@pytest.mark.parametrize("n,flags,eig,method,form", [(6, 0, None, 2, None), (20, 0, None, 2, None), (260, 0, None, 1, 0),
                                                     (1025, 0, None, 1, 0), (2052, 0, None, 1, 0),
                                                     (260, 0, "band", 1, 0), (1025, 0, "band", 1, 0),
                                                     (260, PCOA_FLAG_EIG_HOUSEHOLDER, None, 2, None),
                                                     (1025, PCOA_FLAG_EIG_HOUSEHOLDER, None, 2, None)])
def test_eigenpairs_in_process(P, n, flags, eig, method, form):
    bad, eig_method, matvec_form, steps, band = eig_run(P, n, flags, eig)
    print("N = %d, eig = %s: eig_method %d, matvec_form %d, %d Lanczos steps, %d band vectors" % (n, eig, eig_method, matvec_form, steps, band))
    assert eig_method == method and (form is None or matvec_form == form)
    if eig == "band":
        assert band > 0
    assert not bad, bad


def child_main(argv):
    """One n per argument with the knobs of the parent's environment: one JSON line each."""
    P = load_pkg()
    for arg in argv:
        bad, eig_method, matvec_form, steps, band = eig_run(P, int(arg))
        print(json.dumps({"n": int(arg), "bad": bad, "eig_method": eig_method, "matvec_form": matvec_form}))
        sys.stdout.flush()


@pytest.mark.parametrize("env_name,n,form", [("PCOA_SYMV_SYM_MIN_N", 2052, 1), ("PCOA_EXPLICIT_CENTER", 260, 2)])
def test_eigenpairs_in_a_child(env_name, n, form):
    """PCOA_SYMV_SYM_MIN_N=1024 at N = 2052: the upper-triangle mat-vec with the fp64 row sums of the tile pass;
    PCOA_EXPLICIT_CENTER=1 at N = 260: Lanczos over the materialised B.  (The knobs are read once: a child each, never retried.)"""
    env = dict(os.environ, **{env_name: "1024" if env_name == "PCOA_SYMV_SYM_MIN_N" else "1"})
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(n)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, env=env, timeout=CHILD_LIMIT)
    assert res.returncode == 0, "child exited with status %d\n%s" % (res.returncode, res.stderr[-4000:])
    cases = [json.loads(t) for t in res.stdout.splitlines() if t.startswith("{")]
    assert len(cases) == 1, res.stdout
    r = cases[0]
    assert r["eig_method"] == 1 and r["matvec_form"] == form, r
    assert not r["bad"], r["bad"]


# ------------------------------------------------------------------------------------------------------- 5. life cycle
def _results(eng):
    comps, lam, nz = eng.compute(2)
    b, rs, nzc, mm = eng.center()
    return comps, lam, nz, b, rs, nzc, mm


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_bind_unbind_returns_the_shared_bits_and_the_binding_survives_reset(P, I):
    n = 1044
    x, m, _ = C.populations_with_missing(n, 400)
    with P.PcoaEngine(n) as never, P.PcoaEngine(n) as eng, P.PcoaEngine(n) as q:
        never.accumulate_bits(I.pack_bits(x))
        feed_pair(I, eng, q, x, m)
        want = _results(never)
        assert eng.get_call_companion() == (None, 0)
        eng.set_call_companion(q, 400)
        got_q, got_v = eng.get_call_companion()
        assert got_q is q and got_v == 400
        bound = _results(eng)
        assert not np.array_equal(bound[1], want[1])                              # it did decompose something else
        eng.debug_centred_matvec(np.ones(n), 1)
        eng.reset()
        assert eng.get_call_companion()[0] is q and not eng.gram().any()          # the binding survives, S does not
        eng.accumulate_bits(I.pack_bits(x))
        assert _same_bits(_results(eng), bound)
        eng.set_call_companion(None)
        assert eng.get_call_companion() == (None, 0)
        assert _same_bits(_results(eng), want)


def test_refusals_leave_the_ctx_usable(P, I):
    n = 64
    x, m, _ = C.populations_with_missing(n, 200)
    L = load_pkg("_lib")
    lib = L.load()
    assert lib.pcoa_set_call_companion(None, None, 0) == PCOA_ERR_INVALID_ARG
    assert b"pcoa_set_call_companion" in lib.pcoa_last_error(None)
    with P.PcoaEngine(n) as eng, P.PcoaEngine(n) as q, P.PcoaEngine(n) as q2, P.PcoaEngine(n + 4) as other_n, \
            P.PcoaEngine(n, strip=(0, n)) as strip, P.PcoaEngine(n, operator=True) as op:
        feed_pair(I, eng, q, x, m)

        def refused(call, code, *words):
            with pytest.raises(P.PcoaError) as err:
                call()
            assert err.value.code == code, str(err.value)
            for w in words:
                assert w in str(err.value), str(err.value)
            assert eng.get_call_companion() == (None, 0)

        refused(lambda: eng.set_call_companion(eng, 200), PCOA_ERR_INVALID_ARG, "ctx itself")
        refused(lambda: eng.set_call_companion(other_n, 200), PCOA_ERR_INVALID_ARG, "samples")
        refused(lambda: eng.set_call_companion(q, -1), PCOA_ERR_INVALID_ARG, "n_variants")
        refused(lambda: eng.set_call_companion(strip, 200), PCOA_ERR_STATE, "strip owner")
        refused(lambda: eng.set_call_companion(op, 200), PCOA_ERR_STATE, "operator ctx")
        for bad, word in ((strip, "strip owner"), (op, "operator ctx")):
            with pytest.raises(P.PcoaError) as err:
                bad.set_call_companion(q, 200)
            assert err.value.code == PCOA_ERR_STATE and word in str(err.value)
        q.set_call_companion(q2, 200)
        refused(lambda: eng.set_call_companion(q, 200), PCOA_ERR_STATE, "itself has a companion")
        q.set_call_companion(None)
        eng.set_similarity("jaccard")
        refused(lambda: eng.set_call_companion(q, 200), PCOA_ERR_STATE, "Jaccard / cosine")
        eng.set_similarity("shared")
        eng.set_call_companion(q, 200)
        for kind in ("jaccard", "cosine"):
            with pytest.raises(P.PcoaError) as err:
                eng.set_similarity(kind)
            assert err.value.code == PCOA_ERR_STATE and "call companion" in str(err.value)
            assert eng.get_similarity() == "shared"
        eng.set_similarity("shared")
        comps, lam, nz = eng.compute(2)                                           # still bound, still serves
        assert nz == n and np.all(np.isfinite(lam))


def test_companion_on_another_device_is_refused(P):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("the different-devices refusal needs a second GPU")
    with P.PcoaEngine(8, device=0) as eng, P.PcoaEngine(8, device=1) as q:
        with pytest.raises(P.PcoaError) as err:
            eng.set_call_companion(q, 10)
        assert err.value.code == PCOA_ERR_STATE and "different devices" in str(err.value)


def test_n_variants_below_a_missing_count_is_invalid(P, I):
    n = 65
    x, m, _ = C.populations_with_missing(n, 200)
    worst = int(m.sum(axis=0).max())
    with P.PcoaEngine(n) as eng, P.PcoaEngine(n) as q:
        feed_pair(I, eng, q, x, m)
        eng.set_call_companion(q, worst - 1)
        for call in (lambda: eng.compute(2), lambda: eng.center(), lambda: eng.debug_centred_matvec(np.ones(n), 0)):
            with pytest.raises(P.PcoaError) as err:
                call()
            assert err.value.code == PCOA_ERR_INVALID_ARG and "n_variants" in str(err.value) and "missing count" in str(err.value)
        eng.set_call_companion(q, 200)                                            # binding again with the right V: it serves
        assert eng.compute(2)[2] == n


def test_companion_with_an_int64_part_is_not_built(P, I):
    n = 65
    x, m, _ = C.populations_with_missing(n, 200)
    with P.PcoaEngine(n) as eng, P.PcoaEngine(n) as q:
        eng.accumulate_bits(I.pack_bits(x))
        q.load_gram(int_gram(m) * 2 ** 26)
        assert q.timings()["gram_i64_live"] == 1
        eng.set_call_companion(q, 200 * 2 ** 26)
        with pytest.raises(P.PcoaError) as err:
            eng.compute(2)
        assert err.value.code == PCOA_ERR_STATE and "not built" in str(err.value) and "companion" in str(err.value)
        eng.set_call_companion(None)
        assert eng.compute(2)[2] == n


def test_an_error_of_the_companion_is_reported_on_ctx(P, I):
    n = 40
    x, m, _ = C.populations_with_missing(n, 100)
    with P.PcoaEngine(n) as eng, P.PcoaEngine(n, gram_kernel="fp4") as q:
        eng.accumulate_bits(I.pack_bits(x))
        t = m.astype(np.uint8)
        t[1, 2] = 2                                                               # forced FP4 refuses anything but 0 / 1
        try:
            q.accumulate_dense_u8(t)
        except P.PcoaError:
            pass   # (reported here or at the next synchronising call: the engine's S stays invalid either way)
        eng.set_call_companion(q, 100)
        with pytest.raises(P.PcoaError) as err:
            eng.compute(2)
        assert err.value.code == PCOA_ERR_INVALID_ARG and "the call companion:" in str(err.value) and "other than 0 or 1" in str(err.value)
        eng.set_call_companion(None)
        assert eng.compute(2)[2] == n


def test_project_against_a_bound_ref_is_refused(P, I):
    n_ref, n = 40, 52
    x, m, _ = C.populations_with_missing(n, 300)
    with P.PcoaEngine(n_ref) as ref, P.PcoaEngine(n_ref) as q, P.PcoaEngine(n, strip=(n_ref, n - n_ref)) as cross:
        feed_pair(I, ref, q, x[:, :n_ref], m[:, :n_ref])
        cross.accumulate_bits(I.pack_bits(x))
        ref.set_call_companion(q, 300)
        comps, lam, _ = ref.compute(2)
        with pytest.raises(P.PcoaError) as err:
            ref.project(cross, comps, lam)
        assert err.value.code == PCOA_ERR_STATE and "not built" in str(err.value)
        ref.set_call_companion(None)
        comps, lam, _ = ref.compute(2)
        assert ref.project(cross, comps, lam).shape == (n - n_ref, 2)             # both engines still serve


def test_the_screen_and_the_reads_do_not_look_at_the_binding(P, I):
    n = 260
    x, m, _ = C.populations_with_missing(n, 400)
    with P.PcoaEngine(n) as eng, P.PcoaEngine(n) as q:
        feed_pair(I, eng, q, x, m)
        plain = eng.similar_pairs(0.2)
        s = eng.gram()
        eng.set_call_companion(q, 400)
        eng.compute(2)
        got = eng.similar_pairs(0.2)
        assert np.array_equal(got[0], plain[0]) and got[1] == plain[1] and np.array_equal(got[2], plain[2])
        assert np.array_equal(eng.gram(), s)


def test_a_subset_of_a_bound_ctx_equals_a_fresh_pair(P, I):
    n = 260
    x, m = C.eig_cohort(n)
    v = x.shape[0]
    keep = np.setdiff1d(np.arange(n), np.arange(5, n, 9))
    with P.PcoaEngine(n) as eng, P.PcoaEngine(n) as q, P.PcoaEngine(keep.size) as fresh, P.PcoaEngine(keep.size) as fresh_q:
        feed_pair(I, eng, q, x, m)
        eng.set_call_companion(q, v)
        before = _results(eng)
        sub = eng.subset(keep)
        try:
            sub_q, sub_v = sub.get_call_companion()
            assert sub_q is not None and sub_q is not q and sub_v == v
            assert np.array_equal(sub_q.gram(), int_gram(m[:, keep]))
            b1, rs1, nz1, mm1 = sub.center()
            c1, l1, _ = sub.compute(2)
        finally:
            sub.close()
        feed_pair(I, fresh, fresh_q, x[:, keep], m[:, keep])
        fresh.set_call_companion(fresh_q, v)
        b2, rs2, nz2, mm2 = fresh.center()
        c2, l2, _ = fresh.compute(2)
        assert np.array_equal(b1, b2) and np.array_equal(rs1, rs2) and nz1 == nz2 == keep.size and mm1 == mm2
        assert np.all(np.abs(l1 - l2) <= 1e-6 * np.abs(l2))
        for c in range(2):
            a = c1[:, c] if np.dot(c1[:, c], c2[:, c]) >= 0 else -c1[:, c]
            assert np.linalg.norm(a - c2[:, c]) < 1e-6
        assert _same_bits(_results(eng), before)                                  # destroying the subset left the source pair alone
        assert eng.get_call_companion()[0] is q


# ------------------------------------------------------------------------------------------------------- 6. both hosts
@pytest.fixture(scope="module")
def host_cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("completehosts")
    x, m = C.eig_cohort(C.HOST_N)
    names = [C.name_of(i) for i in range(C.HOST_N)]
    prefix = str(d / "set" / "cohort")
    C.write_plink(prefix, x, m, names)
    return {"bed": prefix + ".bed", "x": x, "m": m, "names": names, "dir": str(d)}


_runs = {}


def run_once(host, path, extra=()):
    key = (host, path, tuple(extra))
    if key not in _runs:
        _runs[key] = (C.run_driver if host == "driver" else C.run_python)(["--input-path", path] + list(extra))
    return _runs[key]


def test_both_hosts_end_to_end(host_cohort):
    h = host_cohort
    rates = {"driver": os.path.join(h["dir"], "rates_driver.tsv"), "python": os.path.join(h["dir"], "rates_python.tsv")}
    a = run_once("driver", h["bed"], ("--missing-calls", "pairwise", "--call-rate-output-path", rates["driver"]))
    b = run_once("python", h["bed"], ("--missing-calls", "pairwise", "--call-rate-output-path", rates["python"]))
    assert a.returncode == 0, a.stderr
    assert b.returncode == 0, b.stderr
    assert a.stdout.encode() == b.stdout.encode()
    v = h["x"].shape[0]
    assert "Missing calls: %d of %d genotypes (pairwise-complete similarity)" % (int(h["m"].sum()), v * C.HOST_N) in a.stdout
    assert "Non zero rows in matrix: %d / %d." % (C.HOST_N, C.HOST_N) in a.stdout
    rows = [ln.split("\t") for ln in a.stdout.splitlines() if ln.count("\t") == 3]
    assert [r[0] for r in rows] == h["names"]
    got = np.array([[float(r[2]), float(r[3])] for r in rows])
    w, z, _, _ = C.eig_reference(int_gram(h["x"]), int_gram(h["m"]), v)
    for c in range(2):
        col = got[:, c] if np.dot(got[:, c], z[:, c]) >= 0 else -got[:, c]
        assert np.linalg.norm(col - z[:, c]) < 1e-6
    want = C.call_rate_lines(h["names"], h["m"])
    for host in ("driver", "python"):
        assert open(rates[host]).read().splitlines() == want, host
    plain = run_once("driver", h["bed"])
    assert plain.returncode == 0 and plain.stdout != a.stdout                     # the rule changed the coordinates


@pytest.mark.parametrize("host", ["driver", "python"])
def test_outlier_rounds_compose(host_cohort, host):
    r = run_once(host, host_cohort["bed"], ("--missing-calls", "pairwise", "--outlier-iterations", "2", "--outlier-sigma", "1.5"))
    assert r.returncode == 0, r.stderr
    assert "Outlier round 1: removed" in r.stderr and "Missing calls:" in r.stdout
    assert "Non zero rows in matrix:" in r.stdout


@pytest.mark.parametrize("host", ["driver", "python"])
def test_ignore_is_a_run_without_the_flag(host_cohort, host):
    a = run_once(host, host_cohort["bed"], ("--missing-calls", "ignore"))
    b = run_once(host, host_cohort["bed"])
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    assert a.stdout.encode() == b.stdout.encode()


if __name__ == "__main__":
    child_main(sys.argv[1:])

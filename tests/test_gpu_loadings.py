"""GPU tests of the per-variant loadings (pcoa_loadings_*, csrc/loadings.hip): the sums are exact integers wherever the inputs
are, with the bits of samples >= N and every pad word set; .bed rows, the operator store and every split of a call give the
same bits as one call over bitsets; real vectors stay inside the derived summation bound; the loadings of a computed
decomposition are the left singular vectors of X J; nothing modifies S; every error leaves the ctx usable.  The spec is the
numpy statement in loadings_cohort.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_pkg
from loadings_cohort import decode_bed, encode_bed, identity_defects, loadings_rule, pack_rows, planted_cohort, \
    summation_bound

pytestmark = pytest.mark.gpu

SEGMENT_KNOB = "PCOA_OPERATOR_SEGMENT_ROWS"
DENSITY = 0.14
ALL_PC = [1, 2, 3, 8, 9]
# N: below one word; the word boundary; a ragged last word; 79 words (five passes of a 16-lane group); past 8,192 samples; and
# the two sizes at which a row is shared by 32 and by 64 lanes (32 and 64 words: loadings_lanes in csrc/loadings.hip), which the
# other sizes (8 and 16 lanes) do not reach
CROSSED_N = [33, 2504, 8200]
OTHER_N = [6, 31, 32, 70, 1000, 2048]


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def L():
    return load_pkg("_lib")


def cohort(rng, n, nv):
    """0/1 rows of density 0.14 with one all-zero and one all-ones row (rows 0 and 1 where there are that many)."""
    x = (rng.random((nv, n)) < DENSITY).astype(np.uint8)
    x[0] = 0
    if nv > 1:
        x[1] = 1
    return x


def to_dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dtype) if dtype is not None else a).cuda()


def run_bits(ld, bits, in_dev, out_dev):
    """One pcoa_loadings_bits call in one of the four pointer forms; always returns numpy [rows, k]."""
    arg = to_dev(bits, np.int32) if in_dev else bits
    out = ld.bits(arg, device_out=out_dev)
    return out.cpu().numpy() if out_dev else out


def exact_case(P, rng, n, shapes):
    """shapes: (nv, pad_words, num_pc, in_dev, out_dev).  Integer vectors in [-8, 8], flags 0: every partial sum is an integer
    below 2^53 in any order, so the result is numpy's product bit for bit."""
    nv_max = max(s[0] for s in shapes)
    x = cohort(rng, n, nv_max)
    xf = x.astype(np.float64)
    with P.PcoaEngine(n) as eng:
        for nv, pad, k, in_dev, out_dev in shapes:
            rows = slice(1, 2) if nv == 1 and nv_max > 1 else slice(0, nv)   # a single row: the all-ones one
            u = rng.integers(-8, 9, size=(n, k)).astype(np.float64)
            want = xf[rows] @ u
            assert np.abs(want).max() < 2.0 ** 53
            bits = pack_rows(x[rows], n, pad_words=pad, garbage=rng)
            with eng.loadings(u, None, centre=False, unit=False) as ld:
                got = run_bits(ld, bits, in_dev, out_dev)
            assert got.shape == want.shape and np.array_equal(got, want), (n, nv, pad, k, in_dev, out_dev)


# ---- 1. exact integer rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", CROSSED_N)
def test_integer_sums_are_exact_for_every_num_pc(P, n):
    """Every num_pc over 2,049 rows (several workgroups for every chunk size), then one row and 33 rows; the four pointer forms
    and both pitches rotate through the calls; tail bits and pad words are all ones."""
    rng = np.random.default_rng(4000 + n)
    shapes = []
    for i, k in enumerate(ALL_PC):
        shapes.append((2049, 3 * (i & 1), k, bool(i & 1), bool(i & 2)))
        shapes.append(([1, 33][i & 1], 3 * ((i + 1) & 1), k, not (i & 1), not (i & 2)))
    exact_case(P, rng, n, shapes)


@pytest.mark.parametrize("n", OTHER_N)
def test_integer_sums_are_exact_at_the_word_boundaries(P, n):
    rng = np.random.default_rng(4100 + n)
    ks = [k for k in ALL_PC if k <= n]
    shapes = [(nv, 3 * ((i + j) & 1), ks[(i + j) % len(ks)], bool((i + j) & 1), bool((i + j) & 2))
              for i, nv in enumerate([1, 33, 2049]) for j in range(2)]
    exact_case(P, rng, n, shapes)


# ---- 2. PLINK rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nv", [(31, 33), (33, 33), (2504, 2049)])   # N % 4 = 3, 1, 0
def test_bed_rows_equal_their_decoded_bitsets_bit_for_bit(P, n, nv):
    rng = np.random.default_rng(4200 + n)
    x = cohort(rng, n, nv)
    u = rng.standard_normal((n, 3))
    lam = np.array([9.0, 5.0, 2.5])
    with P.PcoaEngine(n) as eng, eng.loadings(u, lam) as ld:
        for a1 in (False, True):
            missing = rng.random((nv, n)) < 0.02
            bed = encode_bed(x, n, missing=missing, ref_is_a1=a1, rng=rng)
            carriers = decode_bed(bed, n, ref_is_a1=a1)
            assert np.array_equal(carriers, x & ~missing)
            want = ld.bits(pack_rows(carriers, n))
            got_host = ld.plink_bed(bed, ref_is_a1=a1)
            got_dev = ld.plink_bed(to_dev(bed), ref_is_a1=a1, device_out=True).cpu().numpy()
            assert np.array_equal(got_host, want) and np.array_equal(got_dev, want), (n, a1)
            assert not want[0].any()   # the all-zero row


# ---- 3. operator store ----------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
sys.path.insert(0, %(tests)r)
import numpy as np
from conftest import load_pkg
from loadings_cohort import pack_rows
P = load_pkg()
L = load_pkg("_lib")
rng = np.random.default_rng(4300)
n, v = 130, 134
x = (rng.random((v, n)) < 0.14).astype(np.uint8)
bits = pack_rows(x, n)
u = rng.standard_normal((n, 3))
lam = np.array([7.0, 3.0, 1.5])
with P.PcoaEngine(n, operator=True) as eng:
    for a, b in ((0, 1), (1, 34), (34, 134)):        # calls of 1, 33 and 100 rows into segments of 64
        eng.accumulate_bits(bits[a:b])
    assert eng.operator_info()[0] == v
    with eng.loadings(u, lam) as ld:
        want = ld.bits(bits)
        for first, cnt in ((0, v), (0, 1), (60, 10), (63, 2), (v - 1, 1), (5, 0)):
            got = ld.operator(first, cnt)
            assert got.shape == (cnt, 3) and np.array_equal(got, want[first:first + cnt]), (first, cnt)
        got = ld.operator(0, None, device_out=True).cpu().numpy()
        assert np.array_equal(got, want)
        for first, cnt in ((0, v + 1), (v, 1), (-1, 2), (3, -1)):
            try:
                ld.operator(first, cnt)
                raise AssertionError("no error for %%r" %% ((first, cnt),))
            except P.PcoaError as e:
                assert e.code == L.PCOA_ERR_INVALID_ARG, e
        assert np.array_equal(ld.operator(0, v), want)   # the ctx is usable after the errors
with P.PcoaEngine(n) as full:
    with full.loadings(u, lam) as ld:
        try:
            ld.operator(0, 0)
            raise AssertionError("a full engine served pcoa_loadings_operator")
        except P.PcoaError as e:
            assert e.code == L.PCOA_ERR_STATE, e
print("LOADINGS-STORE-OK")
"""


def test_store_rows_across_segment_boundaries_equal_bitsets_bit_for_bit():
    """Segments of 64 rows (the knob is read once per process: a fresh child)."""
    env = dict(os.environ)
    env[SEGMENT_KNOB] = "64"
    res = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests")}], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0 and "LOADINGS-STORE-OK" in res.stdout, res.stdout[-3000:]


# ---- 4. independence ------------------------------------------------------------------------------------------------------
def test_an_entry_does_not_depend_on_its_companions_or_on_the_split_of_the_call(P):
    n, nv = 2504, 2049
    rng = np.random.default_rng(4400)
    x = cohort(rng, n, nv)
    bits = pack_rows(x, n)
    u = rng.standard_normal((n, 9))
    lam = rng.uniform(1.0, 50.0, size=9)
    with P.PcoaEngine(n) as eng:
        with eng.loadings(u, lam) as ld:
            all9 = ld.bits(bits)
            again = ld.bits(to_dev(bits, np.int32), device_out=True).cpu().numpy()
            split = np.concatenate([ld.bits(bits[0:1]), ld.bits(bits[1:34]), ld.bits(bits[34:])])
        assert np.array_equal(all9, again) and np.array_equal(all9, split)
        for c in range(9):
            with eng.loadings(u[:, c:c + 1], lam[c:c + 1]) as ld:
                assert np.array_equal(ld.bits(bits)[:, 0], all9[:, c]), c
        with eng.loadings(u[:, 4:6], lam[4:6]) as ld:   # two of them as a pair
            assert np.array_equal(ld.bits(bits), all9[:, 4:6])


# ---- 5. summation bound, real vectors -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 2504, 4100])
def test_real_vectors_stay_inside_the_summation_bound(P, n):
    """CENTRE | UNIT against the longdouble rule; the bound is loadings_cohort.summation_bound (derived, not measured)."""
    rng = np.random.default_rng(4500 + n)
    nv = 257
    x = cohort(rng, n, nv)
    u = rng.standard_normal((n, 3)) + 0.3      # a mean that is not small
    lam = np.array([812.5, 77.0, 3.25])
    with P.PcoaEngine(n) as eng, eng.loadings(u, lam) as ld:
        got = ld.bits(pack_rows(x, n, pad_words=1, garbage=rng))
    want = loadings_rule(x, u, lam)
    bound = summation_bound(x, u, lam, want)
    err = np.abs(got.astype(np.longdouble) - want)
    print("n = %d: max error %.3e, max error / bound %.3f" % (n, float(err.max()), float((err[1:] / bound[1:]).max())))
    assert (err <= bound).all()
    assert not got[0].any() and np.array_equal(got[0], np.zeros(3))   # c_v = 0: exactly 0


# ---- 6. end to end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operator", [False, True])
def test_loadings_of_a_computed_decomposition_are_the_left_singular_vectors(P, operator):
    """The solver accepts pairs at a 1e-11 relative residual and both defects are U^T R / lambda: 1e-8 covers the three decades
    of scale / lambda_3 on this cohort; the rule alone gives 3e-15 (test_loadings_cpu.py)."""
    x = planted_cohort()
    n = x.shape[1]
    bits = pack_rows(x, n)
    with P.PcoaEngine(n, operator=operator) as eng:
        eng.accumulate_bits(bits)
        comps, lam, _ = eng.compute(3)
        with eng.loadings(comps, lam) as ld:
            w = ld.operator() if operator else ld.bits(bits)
    ortho, back = identity_defects(x, comps, lam, w)
    print("operator = %s: lambda = %s, |W^T W - I| = %.3e, |(XJ)^T W / sqrt(lambda) - U| = %.3e" % (operator, lam, ortho, back))
    assert ortho <= 1e-8 and back <= 1e-8


# ---- 7. state -------------------------------------------------------------------------------------------------------------
def test_loadings_leave_s_alone_and_run_behind_queued_accumulation(P):
    n, nv = 333, 700
    rng = np.random.default_rng(4700)
    x = cohort(rng, n, nv)
    bits = pack_rows(x, n)
    u = rng.standard_normal((n, 2))
    lam = np.array([4.0, 2.0])
    with P.PcoaEngine(n) as eng:
        eng.accumulate_bits(bits[:400])
        s_before = eng.gram().astype(np.int64)
        eng.accumulate_bits(to_dev(bits[400:], np.int32))     # a device tile: queued, not waited for
        with eng.loadings(u, lam) as ld:
            queued = ld.bits(bits)                            # behind the queued accumulation
            eng.sync()
            settled = ld.bits(bits)
            bed = encode_bed(x, n, rng=rng)
            ld.plink_bed(bed)
            ld.bits(to_dev(bits, np.int32), device_out=True)
        assert np.array_equal(queued, settled)
        s_after = eng.gram().astype(np.int64)
        xf = x.astype(np.float64)
        assert np.array_equal(s_after, (xf.T @ xf).astype(np.int64))
        assert np.array_equal(s_before, (xf[:400].T @ xf[:400]).astype(np.int64))
        with eng.loadings(u, lam) as ld:                      # S read as int64 around a sequence of loadings calls
            ld.bits(bits)
            ld.plink_bed(bed)
            st = ld.stats()
        assert np.array_equal(eng.gram().astype(np.int64), s_after)
        assert st["loadings_variants"] >= 2 * nv and st["loadings_bytes"] > 0 and st["loadings_seconds"] > 0


def test_every_error_leaves_the_ctx_usable(P, L):
    n = 70
    rng = np.random.default_rng(4800)
    lib = L.load()
    x = cohort(rng, n, 33)
    bits = pack_rows(x, n)
    bed = encode_bed(x, n, rng=rng)
    ui = rng.integers(-8, 9, size=(n, 2)).astype(np.float64)
    want = x.astype(np.float64) @ ui
    u_t = np.ascontiguousarray(ui.T)
    out = np.zeros((33, 2))
    vp = ctypes.c_void_p

    def ptr(a):
        return vp(a.ctypes.data)

    with P.PcoaEngine(n) as eng:
        ctx = eng._ctx
        # before begin: PCOA_ERR_STATE from every rows call
        assert lib.pcoa_loadings_bits(ctx, ptr(bits), 33, bits.shape[1], 0, ptr(out), 0) == L.PCOA_ERR_STATE
        assert lib.pcoa_loadings_plink_bed(ctx, ptr(bed), 33, bed.shape[1], 0, 0, ptr(out), 0) == L.PCOA_ERR_STATE
        assert b"pcoa_loadings_begin" in lib.pcoa_last_error(ctx)
        assert lib.pcoa_loadings_end(ctx) == L.PCOA_OK
        # begin's argument errors
        lam_bad = [np.array([1.0, 0.0]), np.array([1.0, -2.0]), np.array([np.inf, 1.0]), np.array([1.0, np.nan])]
        bad = [lib.pcoa_loadings_begin(ctx, 2, None, None, 0),
               lib.pcoa_loadings_begin(ctx, 0, ptr(u_t), None, 0),
               lib.pcoa_loadings_begin(ctx, n + 1, ptr(u_t), None, 0),
               lib.pcoa_loadings_begin(ctx, 2, ptr(u_t), None, L.PCOA_LOADINGS_UNIT),
               lib.pcoa_loadings_begin(ctx, 2, ptr(u_t), None, 8)]
        bad += [lib.pcoa_loadings_begin(ctx, 2, ptr(u_t), ptr(lb), L.PCOA_LOADINGS_UNIT) for lb in lam_bad]
        assert bad == [L.PCOA_ERR_INVALID_ARG] * len(bad)
        assert lib.pcoa_loadings_bits(ctx, ptr(bits), 33, bits.shape[1], 0, ptr(out), 0) == L.PCOA_ERR_STATE   # still not begun
        assert lib.pcoa_loadings_begin(ctx, 2, ptr(u_t), None, 0) == L.PCOA_OK
        # the rows calls' argument errors
        bad = [lib.pcoa_loadings_bits(ctx, None, 33, bits.shape[1], 0, ptr(out), 0),
               lib.pcoa_loadings_bits(ctx, ptr(bits), 33, bits.shape[1], 0, None, 0),
               lib.pcoa_loadings_bits(ctx, ptr(bits), -1, bits.shape[1], 0, ptr(out), 0),
               lib.pcoa_loadings_bits(ctx, ptr(bits), 33, bits.shape[1] - 1, 0, ptr(out), 0),
               lib.pcoa_loadings_plink_bed(ctx, None, 33, bed.shape[1], 0, 0, ptr(out), 0),
               lib.pcoa_loadings_plink_bed(ctx, ptr(bed), 33, bed.shape[1], 0, 0, None, 0),
               lib.pcoa_loadings_plink_bed(ctx, ptr(bed), 33, bed.shape[1] - 1, 0, 0, ptr(out), 0)]
        assert bad == [L.PCOA_ERR_INVALID_ARG] * len(bad)
        assert lib.pcoa_loadings_operator(ctx, 0, 1, ptr(out), 0) == L.PCOA_ERR_STATE      # not an operator ctx
        assert lib.pcoa_loadings_begin(ctx, 2, None, None, 0) == L.PCOA_ERR_INVALID_ARG    # the resident vectors stay
        # ... and case 1 again on the same ctx
        assert lib.pcoa_loadings_bits(ctx, ptr(bits), 33, bits.shape[1], 0, ptr(out), 0) == L.PCOA_OK
        assert np.array_equal(out, want)
        assert lib.pcoa_loadings_bits(ctx, ptr(bits), 0, bits.shape[1], 0, None, 0) == L.PCOA_OK       # an empty call
        assert lib.pcoa_loadings_end(ctx) == L.PCOA_OK
        assert lib.pcoa_loadings_bits(ctx, ptr(bits), 33, bits.shape[1], 0, ptr(out), 0) == L.PCOA_ERR_STATE
        # the accumulation path is what it was
        eng.accumulate_bits(bits)
        xf = x.astype(np.float64)
        assert np.array_equal(eng.gram().astype(np.int64), (xf.T @ xf).astype(np.int64))


def test_strip_and_subset_engines_serve(P):
    """Only n, the device, the stream and the staging slots are used: every kind of ctx gives the full engine's bits."""
    n = 130
    rng = np.random.default_rng(4900)
    x = cohort(rng, n, 65)
    bits = pack_rows(x, n)
    u = rng.standard_normal((n, 2))
    lam = np.array([3.0, 2.0])
    with P.PcoaEngine(n) as eng:
        eng.accumulate_bits(bits)
        with eng.loadings(u, lam) as ld:
            want = ld.bits(bits)
        keep = np.arange(0, n, 2)
        sub_bits = pack_rows(x[:, keep], len(keep))
        with eng.subset(keep) as sub, sub.loadings(u[keep], lam) as ld:
            got_sub = ld.bits(sub_bits)
    with P.PcoaEngine(len(keep)) as small, small.loadings(u[keep], lam) as ld:
        assert np.array_equal(got_sub, ld.bits(sub_bits))
    with P.PcoaEngine(n, strip=(32, 64)) as strip, strip.loadings(u, lam) as ld:
        assert np.array_equal(ld.bits(bits), want)


# ---- 8. hosts -------------------------------------------------------------------------------------------------------------
GOLDEN = "tile130"


@pytest.fixture(scope="module")
def host_runs(tmp_path_factory):
    """--loadings-output-path runs of both hosts over one golden fixture as VCF and as PLINK, each (host, kind, gram) once."""
    from conftest import load_golden, write_golden_plink, write_golden_vcf
    from test_operator_cpu import _run_driver, _run_python
    d = tmp_path_factory.mktemp("loadings_hosts")
    g = load_golden(GOLDEN)
    write_golden_vcf(g, str(d / (GOLDEN + ".vcf")))
    write_golden_plink(g, str(d / GOLDEN))
    paths = {"vcf": str(d / (GOLDEN + ".vcf")), "plink": str(d / GOLDEN) + ".bed"}
    ingest = load_pkg("ingest")
    n = int(g["n_samples"])
    _, _, data = ingest.load_vcf(paths["vcf"], None)
    idx, offs = data[0][1], data[0][2]
    x_vcf = np.zeros((len(offs) - 1, n), dtype=np.uint8)
    for r in range(len(offs) - 1):
        x_vcf[r, idx[offs[r]:offs[r + 1]]] = 1
    _, _, data = ingest.load_plink(paths["plink"], None, as_bits=True)
    x_bed = np.unpackbits(data[0][1].view(np.uint8), axis=1, bitorder="little")[:, :n]
    cache = {}

    def run(host, kind, gram):
        key = (host, kind, gram)
        if key not in cache:
            out = str(d / ("%s_%s_%s.tsv" % key))
            res = (_run_driver if host == "driver" else _run_python)(
                ["--input-path", paths[kind], "--all-references", "--gram", gram, "--loadings-output-path", out])
            assert res.returncode == 0, res.stderr[-3000:]
            lines = [ln.split("\t") for ln in open(out).read().splitlines()]
            cache[key] = ([ln[:4] for ln in lines], np.array([[float(t) for t in ln[4:]] for ln in lines]))
        return cache[key]

    return run, {"vcf": x_vcf, "plink": x_bed}


def host_bound(x, w):
    """Case 5's bound for the rows of a host's file, from numpy's eigenpairs of the same cohort (the bound is a function of
    |u|, lambda and the rows: the solver's 1e-11 does not move it)."""
    u, lam = centred_eig_of(x)
    return np.asarray(summation_bound(x, u, lam, w), dtype=np.float64)


def centred_eig_of(x):
    from loadings_cohort import centred_eig
    return centred_eig(x, 2)


@pytest.mark.parametrize("kind", ["vcf", "plink"])
def test_both_hosts_write_the_same_loadings_file(host_runs, kind):
    run, xs = host_runs
    x = xs[kind]
    head_d, w_d = run("driver", kind, "implicit")
    head_p, w_p = run("python", kind, "implicit")
    assert len(head_d) == x.shape[0] and head_d == head_p            # index, contig, position, id: line for line
    assert [h[0] for h in head_d] == [str(v) for v in range(x.shape[0])]
    assert all(h[1] == "17" and int(h[2]) >= 41196312 for h in head_d)
    assert all(h[3].startswith("rs") for h in head_d) if kind == "plink" else all(h[3] == "." for h in head_d)
    assert w_d.shape == (x.shape[0], 2) and w_p.shape == w_d.shape
    assert (np.abs(w_d - w_p) <= host_bound(x, w_d)).all()
    assert np.abs(w_d.T @ w_d - np.eye(2)).max() <= 1e-8            # the rows ARE the left singular vectors of this cohort
    assert not w_d[x.sum(axis=1) == 0].any()


@pytest.mark.parametrize("host,kind", [("driver", "plink"), ("python", "plink"), ("python", "vcf")])
def test_a_hosts_second_pass_over_a_stored_s_equals_its_implicit_file(host_runs, host, kind):
    """The same rows through pcoa_loadings_plink_bed / _bits in a second pass and through pcoa_loadings_operator.  The two
    files come from two decompositions -- the stored S and the operator take different mat-vecs, and the solver accepts either's
    pairs at a 1e-11 relative residual -- so they are held to case 5's summation bound PLUS that residual's share, 1e-9 max|w|
    (two decades over 1e-11 for scale / gap, as case 6 takes three).  Observed on an MI355X: 1.4e-15 on the PLINK fixture
    (1.46x the summation bound alone), 5.3e-16 on the VCF fixture (0.68x)."""
    run, xs = host_runs
    x = xs[kind]
    head_i, w_i = run(host, kind, "implicit")
    head_s, w_s = run(host, kind, "stored")
    assert head_s == head_i and w_s.shape == w_i.shape
    for c in range(2):
        if np.dot(w_s[:, c], w_i[:, c]) < 0:
            w_s[:, c] = -w_s[:, c]
    bound = host_bound(x, w_i)
    diff = np.abs(w_s - w_i)
    live = bound > 0
    print("%s %s: max |stored - implicit| = %.3e, max over the bound = %.3f" % (host, kind, float(diff.max()),
                                                                               float((diff[live] / bound[live]).max())))
    slack = bound + 1e-9 * np.abs(w_i).max()
    assert (diff <= slack).all(), float(diff.max())

"""GPU tests of reading K out (pcoa_grm_block, --grm-output-path): the rectangle the fp64 matrix-core kernel of grm_dense.hip
returns equals the numpy statement variants_pca.grm_dense_rule bit for bit on cohorts where every partial sum is an integer
(which also pins the operand and result layout of the instruction), is exactly symmetric and independent of how it was cut on
rounded cohorts, stays inside the summation bound there, ties in with the product and computePca of the same ctx, refuses what
it must and leaves the ctx as it was, and both hosts write the same GCTA-layout files."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, align_sign, load_golden, load_pkg, write_golden_plink
from grm_walk import entry_bound
from test_grm_cpu import balding_nichols, edge_rows, exact_cohort, pack_bed, random_codes, spec_grm_bound, spec_grm_counts, \
    spec_grm_weights

pytestmark = pytest.mark.gpu

DIVISORS = ("used", "pairwise")


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def rule():
    return load_pkg("variants_pca").grm_dense_rule


def fill(eng, codes, ref_is_a1=False, cuts=None):
    rows = pack_bed(codes)
    edges = [0] + sorted(cuts or []) + [rows.shape[0]]
    for a, b in zip(edges[:-1], edges[1:]):
        eng.accumulate_plink_bed(np.ascontiguousarray(rows[a:b]), ref_is_a1=ref_is_a1)
    eng.sync()


def block(eng, rect, divisor, device=False):
    """(K, n) of a rectangle as numpy, through host or device pointers."""
    k, n = eng.grm_block(rect[0], rect[1], rect[2], rect[3], divisor, pairs=True, device=device)
    return (k.cpu().numpy(), n.cpu().numpy()) if device else (k, n)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. exact cohorts -------------------------------------------------------------------------------------------------------
# (used, unused) rows: V = 1, 3, 4, 5, 7, 9, 66, 515 around the k-step of 4; M' a power of two
EXACT_V = [(1, 0), (2, 1), (4, 0), (4, 1), (4, 3), (8, 1), (64, 2), (512, 3)]


def rectangles(n):
    """the full square, 1 x 1 on and off the diagonal, one crossing the diagonal with no word boundary aligned (where N holds
    it), one strictly below the diagonal, the last row alone"""
    out = [(0, n, 0, n), (n // 2, 1, n // 2, 1), (n - 3, 1, 5, 1), (5, 1, n - 3, 1), (n - 10, 10, 0, 10), (n - 1, 1, 0, n)]
    if n >= 48:
        out.append((17, 30, 3, 45))
    return out


@pytest.mark.parametrize("n", [32, 33, 47, 48, 49, 63, 64, 65, 130, 1025])
def test_blocks_equal_the_rule_bit_for_bit_on_exact_cohorts(P, rule, n):
    """mu_v = 1 and d_v = 2: a in {-1, 0, 1}, every partial sum an integer, M' a power of two, and num / n one correctly rounded
    division: the device must return numpy's bits whatever the order, and a wrong lane map of the instruction cannot."""
    rng = np.random.default_rng(4000 + n)
    with P.PcoaEngine(n, grm=True) as eng:
        for k, (vu, vx) in enumerate(EXACT_V):
            for ref_is_a1 in ((False, True) if (vu, vx) == (64, 2) else (bool((k + n) & 1),)):
                codes = exact_cohort(rng, n, vu, vx, ref_is_a1)
                eng.reset()
                fill(eng, codes, ref_is_a1)
                assert eng.grm_info()[:2] == (vu + vx, vu)
                for divisor in DIVISORS:
                    want_k, want_n = rule(codes, ref_is_a1, 0.0, divisor)
                    num = want_k * vu if divisor == "used" else None
                    assert num is None or np.array_equal(num, np.rint(num))
                    for q, (r0, r, c0, c) in enumerate(rectangles(n)):
                        got_k, got_n = block(eng, (r0, r, c0, c), divisor, device=bool((q + k) & 1))
                        where = (n, vu, vx, ref_is_a1, divisor, (r0, r, c0, c))
                        assert same_bits(got_n, want_n[r0:r0 + r, c0:c0 + c].astype(np.int32)), where
                        assert same_bits(got_k, np.ascontiguousarray(want_k[r0:r0 + r, c0:c0 + c])), where
                assert same_bits(eng.grm_pairs_block(0, n, 0, n), want_n.astype(np.int32))


# ---- 2. segments ------------------------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(tests)r)
from conftest import load_pkg
from test_grm_cpu import exact_cohort, pack_bed
P = load_pkg()
rule = load_pkg("variants_pca").grm_dense_rule
rng = np.random.default_rng(65)
n = 65
with P.PcoaEngine(n, grm=True) as eng:
    for vu, vx in ((64, 31), (64, 32), (64, 33), (128, 72)):
        codes = exact_cohort(rng, n, vu, vx)
        rows = pack_bed(codes)
        eng.reset()
        cuts = [0] + sorted(set(int(c) for c in rng.integers(1, vu + vx, size=4))) + [vu + vx]
        for a, b in zip(cuts[:-1], cuts[1:]):
            eng.accumulate_plink_bed(np.ascontiguousarray(rows[a:b]))
        info = eng.grm_info()
        assert info[:2] == (vu + vx, vu) and info[2] == -(-(vu + vx) // 96) * 96 * 32, info   # segments of 96 rows of 32 bytes
        for divisor in ("used", "pairwise"):
            want_k, want_n = rule(codes, False, 0.0, divisor)
            for rect in ((0, n, 0, n), (17, 30, 3, 45), (n - 1, 1, 0, n)):
                r0, r, c0, c = rect
                for device in (False, True):
                    k, m = eng.grm_block(r0, r, c0, c, divisor, pairs=True, device=device)
                    if device:
                        k, m = k.cpu().numpy(), m.cpu().numpy()
                    assert k.tobytes() == np.ascontiguousarray(want_k[r0:r0 + r, c0:c0 + c]).tobytes(), (vu, vx, divisor, rect)
                    assert np.array_equal(m, want_n[r0:r0 + r, c0:c0 + c]), (vu, vx, divisor, rect)
print("SEGMENTS-OK")
"""


def test_blocks_across_segment_boundaries():
    """V = 95, 96, 97 and 200 at N = 65 with segments of 96 rows, fed in ragged calls (the knob is read once per process)."""
    env = dict(os.environ)
    env["PCOA_GRM_SEGMENT_ROWS"] = "96"
    res = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests")}], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0 and "SEGMENTS-OK" in res.stdout, res.stdout[-3000:]


# ---- 3. and 4. rounded cohorts ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rounded():
    rng = np.random.default_rng(260)
    return {"bn": balding_nichols(rng, 260, 1000), "edge": edge_rows(random_codes(rng, 300, 130))}


def tiled(eng, n, divisor, bh, bw, r_first=0, c_first=0):
    """the whole matrix from blocks of bh x bw, the first row / column of blocks r_first / c_first wide where given"""
    out = np.full((n, n), np.nan)
    r_edges = ([0, r_first] if r_first else [0]) + list(range((r_first or 0) + bh, n, bh)) + [n]
    c_edges = ([0, c_first] if c_first else [0]) + list(range((c_first or 0) + bw, n, bw)) + [n]
    for ra, rb in zip(r_edges[:-1], r_edges[1:]):
        for ca, cb in zip(c_edges[:-1], c_edges[1:]):
            out[ra:rb, ca:cb] = eng.grm_block(ra, rb - ra, ca, cb - ca, divisor)
    return out


@pytest.mark.parametrize("name", ["bn", "edge"])
def test_symmetry_cut_independence_and_accuracy_on_rounded_cohorts(P, rule, rounded, name):
    codes = rounded[name]
    v, n = codes.shape
    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(n, grm=True) as other:
        fill(eng, codes)
        fill(other, codes, cuts=[1, 7, 130, 131])
        for divisor in DIVISORS:
            k, cnt = block(eng, (0, n, 0, n), divisor)
            assert same_bits(k, np.ascontiguousarray(k.T)), divisor                       # exact symmetry
            assert same_bits(block(eng, (0, n, 0, n), divisor, device=True)[0], k)        # two runs, either pointer kind
            assert same_bits(tiled(eng, n, divisor, 64, 64), k)
            assert same_bits(tiled(eng, n, divisor, 50, 70, r_first=7, c_first=13), k)    # blocks at odd offsets
            assert same_bits(block(other, (0, n, 0, n), divisor)[0], k)                   # other accumulate call sizes
            assert same_bits(eng.grm_dense(divisor, block=100), k)
            want_k, want_n = rule(codes, False, 0.0, divisor)
            assert np.array_equal(cnt, want_n)
            bound = entry_bound(codes, False, 0.0, want_n, divisor)
            err = np.abs(k - want_k)
            share = float((err[bound > 0] / bound[bound > 0]).max())
            print("%s %s: largest share of the entry bound %.3g" % (name, divisor, share))
            assert np.all(err <= bound), (divisor, share)
        if name == "edge":   # sample 1 is never called: a zero row, column and diagonal under both divisors
            for divisor in DIVISORS:
                k = eng.grm_block(0, n, 0, n, divisor)
                assert not k[1].any() and not k[:, 1].any()
        # min_maf changes M' and the matrix as the rule says
        m0 = eng.grm_info()[1]
        eng.grm_set_min_maf(0.2)
        m1 = eng.grm_info()[1]
        assert 0 < m1 < m0
        for divisor in DIVISORS:
            k, cnt = block(eng, (0, n, 0, n), divisor)
            want_k, want_n = rule(codes, False, 0.2, divisor)
            assert np.array_equal(cnt, want_n) and np.all(np.abs(k - want_k) <= entry_bound(codes, False, 0.2, want_n, divisor))
        eng.grm_set_min_maf(0.0)
        assert same_bits(eng.grm_block(0, n, 0, n, "used"), block(other, (0, n, 0, n), "used")[0])


# ---- 5. the tie to the rest of the GRM path ---------------------------------------------------------------------------------
def test_the_dense_k_agrees_with_the_product_and_with_compute(P, rule):
    import torch
    rng = np.random.default_rng(3000)
    n, v = 260, 3000
    codes = balding_nichols(rng, n, v)
    x = rng.standard_normal(n)
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, codes)
        k = eng.grm_dense("used")
        y = eng.grm_matvec_device(torch.from_numpy(x).cuda()).cpu().numpy()
        comps, lam, _ = eng.compute(2)
    _, want_n = rule(codes, False, 0.0, "used")
    tol = entry_bound(codes, False, 0.0, want_n, "used") @ np.abs(x) + spec_grm_bound(codes, False, x)
    assert np.all(np.abs(k @ x - y) <= tol)
    w, vec = np.linalg.eigh(k)
    assert np.allclose(lam, w[::-1][:2], rtol=1e-6, atol=0)
    want = vec[:, ::-1][:, :2]
    assert np.abs(align_sign(comps, want) - want).max() < 1e-6


# ---- 6. state ---------------------------------------------------------------------------------------------------------------
def test_refusals_state_and_statistics(P):
    import torch
    L = P._lib
    lib = L.load()
    n, v = 130, 300
    rng = np.random.default_rng(6)
    codes = random_codes(rng, v, n)
    x = torch.from_numpy(rng.standard_normal(n)).cuda()
    out = np.zeros((n, n))
    vp = ctypes.c_void_p

    def raw(ctx, r0, r, c0, c, div, k=True, pairs=False):
        cnt = np.zeros((n, n), dtype=np.int32)
        return lib.pcoa_grm_block(ctx, r0, r, c0, c, div, vp(out.ctypes.data) if k else None, vp(cnt.ctypes.data) if pairs else None, 0)

    assert raw(None, 0, 1, 0, 1, 0) == L.PCOA_ERR_INVALID_ARG and b"pcoa_grm_block" in lib.pcoa_last_error(None)
    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(n) as full, P.PcoaEngine(n, operator=True) as op, \
            P.PcoaEngine(n, grm_study=True) as study:
        fill(eng, codes)
        fill(study, codes)
        counts0, y0, c0 = eng.grm_counts(), eng.grm_matvec_device(x).cpu().numpy(), eng.compute(2)
        eng.reset_timings()
        for args in ((0, 0, 0, 1, 0), (0, 1, 0, -1, 0), (-1, 2, 0, 1, 0), (0, n + 1, 0, 1, 0), (n - 1, 2, 0, 1, 0), (0, 1, 5, n - 4, 0),
                     (0, 1, 0, 1, 2), (0, 1, 0, 1, -1)):
            assert raw(eng._ctx, *args) == L.PCOA_ERR_INVALID_ARG, args
            assert b"pcoa_grm_block" in lib.pcoa_last_error(eng._ctx) and len(lib.pcoa_last_error(eng._ctx)) > 30
        assert raw(eng._ctx, 0, 1, 0, 1, 0, k=False) == L.PCOA_ERR_INVALID_ARG and b"NULL" in lib.pcoa_last_error(eng._ctx)
        for other, word in ((full, "full engine"), (op, "operator")):
            with pytest.raises(P.PcoaError) as ei:
                other.grm_block(0, 1, 0, 1)
            assert ei.value.code == L.PCOA_ERR_STATE and word in str(ei.value)
        with pytest.raises(P.PcoaError) as ei:
            study.grm_block(0, 1, 0, 1)
        assert ei.value.code == L.PCOA_ERR_STATE and "no weights of its own" in str(ei.value)
        assert eng.grm_block_stats()["grm_block_calls"] == 0
        # the calls count: num alone, num and n, n alone, PAIRWISE without out_pairs (n is needed all the same)
        eng.grm_block(3, 40, 0, 50)
        eng.grm_block(3, 40, 0, 50, pairs=True)
        eng.grm_pairs_block(3, 40, 0, 50)
        eng.grm_block(3, 40, 0, 50, "pairwise")
        st = eng.grm_block_stats()
        assert st["grm_block_calls"] == 4 and st["grm_block_flops"] == 2.0 * 40 * 50 * v * 6 and st["grm_block_seconds"] > 0
        # nothing of the ctx moved
        assert np.array_equal(eng.grm_counts(), counts0) and same_bits(eng.grm_matvec_device(x).cpu().numpy(), y0)
        c1 = eng.compute(2)
        assert same_bits(c1[0], c0[0]) and same_bits(c1[1], c0[1]) and c1[2] == c0[2]
        # M' = 0, as pcoa_compute reports it
        eng.reset()
        eng.accumulate_plink_bed(pack_bed(np.full((5, n), 3, np.uint8)))
        with pytest.raises(P.PcoaError) as ei:
            eng.grm_block(0, 1, 0, 1)
        assert ei.value.code == L.PCOA_ERR_STATE and "none of the 5 variants" in str(ei.value)
        eng.reset()
        fill(eng, codes)
        assert same_bits(eng.grm_matvec_device(x).cpu().numpy(), y0)


# ---- 7. hosts ---------------------------------------------------------------------------------------------------------------
def test_both_hosts_write_the_same_grm_files(tmp_path, rule):
    from test_grm_cpu import _run_driver, _run_python
    g = load_golden("tile260")
    n = write_golden_plink(g, str(tmp_path / "tile260"))
    path = str(tmp_path / "tile260") + ".bed"
    raw = np.fromfile(path, dtype=np.uint8)[3:].reshape(-1, (n + 3) // 4)
    codes = ((raw[:, :, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(raw.shape[0], -1)[:, :n]
    m = spec_grm_weights(spec_grm_counts(codes, False))[3]
    assert m < 1 << 23
    il = np.tril_indices(n)
    files = {}
    for tag, run in (("cpp", _run_driver), ("py", _run_python)):
        plain = run(["--input-path", path, "--grm"])
        assert plain.returncode == 0 and "GRM written" not in plain.stderr, plain.stderr[-2000:]
        for divisor in DIVISORS:
            prefix = str(tmp_path / ("%s_%s" % (tag, divisor)))
            res = run(["--input-path", path, "--grm", "--grm-output-path", prefix] +
                      (["--grm-output-divisor", divisor] if divisor == "pairwise" else []))
            assert res.returncode == 0, res.stderr[-2000:]
            assert res.stdout == plain.stdout                                      # the coordinates do not move
            nbytes = 2 * 4 * (n * (n + 1) // 2)
            assert "GRM written: %d samples, %d used variants, divisor %s, %d bytes" % (n, m, divisor, nbytes) in res.stderr
            files[tag, divisor] = tuple(open(prefix + ext, "rb").read() for ext in (".grm.bin", ".grm.N.bin", ".grm.id"))
    for divisor in DIVISORS:
        assert files["cpp", divisor] == files["py", divisor], divisor
    want_ids = "".join("tile260\tS%04d\n" % i for i in range(n)).encode()
    got = {}
    for divisor in DIVISORS:
        kb, nb, ids = files["cpp", divisor]
        assert ids == want_ids
        k32, n32 = np.frombuffer(kb, dtype="<f4"), np.frombuffer(nb, dtype="<f4")
        want_k, want_n = rule(codes, False, 0.0, divisor)
        assert np.array_equal(n32, want_n[il].astype(np.float32))                  # the N file is exact
        bound = entry_bound(codes, False, 0.0, want_n, divisor)[il]
        assert np.all(np.abs(k32.astype(np.float64) - want_k[il]) <= 2.0 ** -24 * np.abs(want_k[il]) + bound + 2.0 ** -150)
        got[divisor] = (k32, want_n[il], want_k[il])
    # pairwise differs from used exactly where a pair has a missing call (M' < 2^23: the two quotients are more than a float32
    # spacing apart wherever n < M' and num != 0)
    differs = got["used"][0] != got["pairwise"][0]
    n_low = got["used"][1]
    assert not differs[n_low == m].any()
    assert differs[(n_low != m) & (np.abs(got["used"][2]) > 1e-30)].all()

"""GPU tests of the KING-robust kinship screen on the 2-bit store of a GRM engine (pcoa_grm_king_block, pcoa_grm_king_pairs).  The
reference is numpy throughout -- variants_pca.grm_king_rule / grm_king_pairs_rule, which test_grm_king_cpu.py holds to a double
loop -- and every comparison is exact: the counts are integers.  The pair list is also held byte for byte to pcoa_king_pairs on
five plane engines fed the same .bed rows."""
import contextlib
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import king_cohort as K
from conftest import ROOT, load_pkg
from grm_qc_cohort import spec_used
from test_grm_cpu import edge_rows, pack_bed, random_codes, spec_grm_counts
from test_grm_king_cpu import tie_codes

pytestmark = pytest.mark.gpu

BANDS = (0, 64, 128)


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def vp():
    return load_pkg("variants_pca")


def fill(eng, codes, ref_is_a1=False, cuts=None):
    rows = pack_bed(codes)
    edges = [0] + sorted(cuts or []) + [rows.shape[0]]
    for a, b in zip(edges[:-1], edges[1:]):
        eng.accumulate_plink_bed(np.ascontiguousarray(rows[a:b]), ref_is_a1=ref_is_a1)
    eng.sync()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def as_i32(m):
    assert int(np.abs(m).max(initial=0)) < 2 ** 31
    return np.ascontiguousarray(m.astype(np.int32))


def check_counts(eng, want, rows_kind, where):
    """The full square, ragged rectangles, the symmetry, the diagonal, NULL outputs and device outputs against `want`, the three
    int64 matrices of the rule."""
    n = eng.n
    want = [as_i32(w) for w in want]
    got = eng.grm_king_block(0, n, 0, n, rows_kind)
    for g, w, name in zip(got, want, ("hethet", "ibs0", "het_sum")):
        assert g.dtype == np.int32 and same_bits(g, w), (where, name, int((g != w).sum()))
        assert np.array_equal(g, g.T), (where, name)                                            # (i, j) == (j, i)
    h = np.diagonal(got[0])
    assert not np.diagonal(got[1]).any() and np.array_equal(np.diagonal(got[2]), 2 * h), where
    rects = [(17, min(67, n) - 17, 3, n - 3), (n - 1, 1, 0, n), (0, n, n - 1, 1), (min(63, n - 2), 2, min(31, n - 2), 2)]
    if n > 64:
        rects += [(64, n - 64, 0, 64), (0, 64, 64, n - 64), (60, 5, 62, 3)]
    for r0, r, c0, c in rects:
        blk = eng.grm_king_block(r0, r, c0, c, rows_kind)
        mirror = eng.grm_king_block(c0, c, r0, r, rows_kind)
        for g, m, w in zip(blk, mirror, want):
            assert same_bits(g, np.ascontiguousarray(w[r0:r0 + r, c0:c0 + c])), (where, r0, r, c0, c)
            assert np.array_equal(g, m.T), (where, r0, r, c0, c)
    # any subset of the outputs: what is asked for is the same, what is not is not touched
    r0, r, c0, c = 1, min(40, n - 1), 2, n - 2
    for mask in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1)):
        out = eng.grm_king_block(r0, r, c0, c, rows_kind, *[bool(m) for m in mask])
        for o, m, w in zip(out, mask, want):
            assert (o is None) == (not m)
            if m:
                assert same_bits(o, np.ascontiguousarray(w[r0:r0 + r, c0:c0 + c])), (where, mask)
    dev = eng.grm_king_block(r0, r, c0, c, rows_kind, device=True)
    for o, w in zip(dev, want):
        assert o.is_cuda and same_bits(o.cpu().numpy(), np.ascontiguousarray(w[r0:r0 + r, c0:c0 + c])), where


# ---- 1. counts, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 33, 63, 64, 65, 130, 1025])
def test_counts_equal_the_rule_bit_for_bit(P, vp, n):
    """All-missing, all-het and monomorphic rows, a sample that is never called, ragged last words and a last k-step of 1, 5, 2 and
    3 rows; the store's coding either way round; every row, the rows used under a min MAF and under an LD mask."""
    L = P._lib
    rng = np.random.default_rng(2500 + n)
    with P.PcoaEngine(n, grm=True) as eng:
        for v in (1, 5, 66, 515):
            codes = edge_rows(random_codes(rng, v, n, missing=0.1))
            want_all = vp.grm_king_rule(codes)
            for ref_is_a1 in (False, True):
                eng.reset()
                eng.grm_set_min_maf(0.0)
                fill(eng, codes, ref_is_a1)
                check_counts(eng, want_all, "all", (n, v, ref_is_a1, "all"))
                counts = spec_grm_counts(codes, ref_is_a1)
                for how in ("min_maf", "ld"):
                    if how == "min_maf":
                        eng.grm_set_min_maf(0.2)
                        used = spec_used(counts, n, min_maf=0.2)
                    else:
                        eng.grm_set_min_maf(0.0)
                        eng.grm_ld_prune(20, 0.1)
                        used = spec_used(counts, n, keep=eng.grm_ld_mask())
                    assert eng.grm_info()[1] == int(used.sum())
                    if v == 1:      # its one row is monomorphic: no integer lies between 0 and V, and no row is the library's refusal
                        assert used.sum() == 0
                        with pytest.raises(P.PcoaError) as ei:
                            eng.grm_king_block(0, n, 0, n, "used")
                        assert ei.value.code == L.PCOA_ERR_STATE and "none of the 1 variants" in str(ei.value)
                        continue
                    assert 0 < used.sum() < v, (n, v, how)
                    check_counts(eng, vp.grm_king_rule(codes, used), "used", (n, v, ref_is_a1, how))
                    check_counts(eng, want_all, "all", (n, v, ref_is_a1, how, "all"))          # ALL does not look at used_v
                eng.grm_ld_clear()


# ---- 2. pairs: the rule and the plane path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,v", K.SIZES)
def test_pairs_equal_the_rule_and_the_five_plane_screen(P, vp, n, v):
    code = K.codes(n, v)
    lo, hi = K.margins(vp, code)
    assert (round(lo, 3), round(hi, 3)) == K.KNOWN[n]
    want = vp.grm_king_pairs_rule(code, K.CUTOFF)
    assert [(int(p["i"]), int(p["j"])) for p in want] == K.planted_pairs(n)
    h = (code == 2).sum(axis=0).astype(np.int64)
    with contextlib.ExitStack() as stack:
        planes = [stack.enter_context(P.PcoaEngine(n)) for _ in range(5)]
        P.PcoaEngine.accumulate_plink_bed_king(planes, K.bed_rows(code))
        plane_pairs, plane_found, plane_v, plane_het = P.PcoaEngine.king_pairs(planes, K.CUTOFF, capacity=want.size + 3)
    assert plane_found == want.size and plane_v == v and np.array_equal(plane_het, h)
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, code, cuts=[1, 37, v - 5])
        for band in BANDS:
            got, found, n_rows, het = eng.grm_king_pairs(K.CUTOFF, rows="all", band_rows=band, capacity=want.size + 3, het=True)
            assert found == want.size and n_rows == v, (n, band)
            assert same_bits(got, want), (n, band)
            assert got.tobytes() == plane_pairs.tobytes(), (n, band)
            assert het.dtype == np.int64 and np.array_equal(het, h), (n, band)
        # other cutoffs: longer lists, in order
        for x in (0.0221, 0.0442):          # (both below the largest unplanted kinship of every size: K.KNOWN)
            longer = vp.grm_king_pairs_rule(code, x)
            got, found, _ = eng.grm_king_pairs(x, band_rows=64, capacity=longer.size)
            assert found == longer.size > want.size and same_bits(got, longer), (n, x)


def test_the_tie_at_one_half_is_reported(P, vp):
    codes = tie_codes()
    with P.PcoaEngine(codes.shape[1], grm=True) as eng:
        fill(eng, codes)
        got, found, _ = eng.grm_king_pairs(0.5)
        assert found == 1 and same_bits(got, vp.grm_king_pairs_rule(codes, 0.5))
        assert (int(got["i"][0]), int(got["j"][0])) == (0, 1) and int(got["het_sum"][0]) == 2 * int(got["hethet"][0])


# ---- 3. segments ------------------------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(tests)r)
from conftest import load_pkg
from test_grm_cpu import edge_rows, pack_bed, random_codes
P = load_pkg()
vp = load_pkg("variants_pca")
rng = np.random.default_rng(96)
n, v = 130, 300
codes = edge_rows(random_codes(rng, v, n, missing=0.1))
codes[:, 77] = codes[:, 5]
rows = pack_bed(codes)
with P.PcoaEngine(n, grm=True) as eng:
    for a, b in ((0, 50), (50, 97), (97, 300)):
        eng.accumulate_plink_bed(np.ascontiguousarray(rows[a:b]))
    info = eng.grm_info()
    assert info[2] == -(-v // 96) * 96 * 48, info   # segments of 96 rows; 130 samples: 3 x 64 slots, 16 a word
    eng.grm_set_min_maf(0.1)
    counts = np.stack([(codes != 1).sum(axis=1), (codes == 2).sum(axis=1), (codes == 0).sum(axis=1)], axis=1)
    a = counts[:, 1] + 2 * counts[:, 2]
    used = (counts[:, 0] > 0) & (a > 0) & (a < 2 * counts[:, 0]) & (np.minimum(a, 2 * counts[:, 0] - a) >= 0.1 * (2.0 * counts[:, 0]))
    assert eng.grm_info()[1] == used.sum() and 0 < used.sum() < v
    for kind, mask in (("all", None), ("used", used)):
        want = vp.grm_king_rule(codes, mask)
        got = eng.grm_king_block(0, n, 0, n, kind)
        part = eng.grm_king_block(17, 50, 3, n - 3, kind)
        for g, p, w in zip(got, part, want):
            assert np.array_equal(g, w) and np.array_equal(p, w[17:67, 3:]), kind
        for x in (0.0442, 0.177):
            pairs = vp.grm_king_pairs_rule(codes, x, mask)
            assert pairs.size > 0
            for band in (0, 64, 128):
                got, found, n_rows = eng.grm_king_pairs(x, rows=kind, band_rows=band)
                assert found == pairs.size and got.tobytes() == pairs.tobytes() and n_rows == (v if mask is None else used.sum()), (kind, x, band)
print("SEGMENTS-OK")
"""


def test_counts_and_pairs_across_segment_boundaries():
    """V = 300 at N = 130 in four segments of 96 rows, fed in ragged calls (the knob is read once per process): the counts of a
    segment are added to what the segments before left in the output."""
    env = dict(os.environ)
    env["PCOA_GRM_SEGMENT_ROWS"] = "96"
    code = CHILD % {"tests": os.path.join(ROOT, "tests")}
    res = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, timeout=300)
    assert res.returncode == 0 and "SEGMENTS-OK" in res.stdout, res.stdout[-3000:]


# ---- 4. capacity ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge():
    return edge_rows(random_codes(np.random.default_rng(2600), 300, 130, missing=0.1))


def test_capacity_returns_a_prefix_and_the_full_count(P, vp, edge):
    n = edge.shape[1]
    lib = P._lib.load()
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, edge)
        full, found, _ = eng.grm_king_pairs(0.0221, band_rows=64)
        assert found == full.size and found > 100 and same_bits(full, vp.grm_king_pairs_rule(edge, 0.0221))
        for cap in (0, 1, found - 1):
            buf = np.zeros(found + 3, dtype=P.PcoaEngine.KING_PAIR_DTYPE)
            buf["i"], buf["j"], buf["hethet"], buf["ibs0"], buf["het_sum"] = -7, -8, -9, -10, -11
            got = ctypes.c_int64(-1)
            rc = lib.pcoa_grm_king_pairs(eng._ctx, 0, 0.0221, 64, ctypes.c_void_p(buf.ctypes.data) if cap else None, cap,
                                         ctypes.byref(got), None, None)
            assert rc == 0 and got.value == found, cap
            assert same_bits(buf[:cap], full[:cap]), cap
            tail = buf[cap:]
            assert np.all(tail["i"] == -7) and np.all(tail["j"] == -8) and np.all(tail["hethet"] == -9), cap
            assert np.all(tail["ibs0"] == -10) and np.all(tail["het_sum"] == -11), cap
        pairs, nf, _ = eng.grm_king_pairs(0.0221, capacity=0)
        assert pairs.size == 0 and nf == found


# ---- 5. state ---------------------------------------------------------------------------------------------------------------
def test_the_screen_follows_the_state_of_the_ctx_and_leaves_it_alone(P, vp):
    code = K.codes(260, 2000)
    v, n = code.shape
    counts = spec_grm_counts(code, False)

    def check(e, codes, used, what, x=0.0884):
        for kind, mask in (("all", None), ("used", used)):
            want = vp.grm_king_pairs_rule(codes, x, mask)
            got, found, n_rows, het = e.grm_king_pairs(x, rows=kind, band_rows=128, het=True)
            assert want.size > 0 and found == want.size and same_bits(got, want), (what, kind)
            rows = codes if mask is None else codes[mask]
            assert n_rows == rows.shape[0] and np.array_equal(het, (rows == 2).sum(axis=0)), (what, kind)
            blk = e.grm_king_block(5, 70, 60, e.n - 60, kind)
            for g, w in zip(blk, vp.grm_king_rule(codes, mask)):
                assert np.array_equal(g, w[5:75, 60:]), (what, kind)

    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(n, grm_study=True) as study:
        fill(eng, code)
        fill(study, code)
        c0 = eng.compute(2)
        check(eng, code, spec_used(counts, n), "plain")
        c1 = eng.compute(2)
        assert same_bits(c1[0], c0[0]) and same_bits(c1[1], c0[1]) and c1[2] == c0[2]
        keep = np.setdiff1d(np.arange(n), [7, 50, 201, 259, 64])
        with eng.grm_subset(keep) as sub:
            sub_codes = np.ascontiguousarray(code[:, keep])
            check(sub, sub_codes, spec_used(spec_grm_counts(sub_codes, False), keep.size), "subset")
        eng.grm_set_min_maf(0.2)
        used = spec_used(counts, n, min_maf=0.2)
        assert 0 < used.sum() < v and eng.grm_info()[1] == used.sum()
        check(eng, code, used, "min_maf")
        eng.grm_set_min_maf(0.0)
        eng.grm_set_variant_filters(max_missing=0.1)
        used = spec_used(counts, n, max_missing=0.1)
        assert 0 < used.sum() < v and eng.grm_info()[1] == used.sum()
        check(eng, code, used, "filters")
        eng.grm_set_variant_filters()
        cand, kept = eng.grm_ld_prune(20, 0.1)
        assert 0 < kept < cand
        check(eng, code, spec_used(counts, n, keep=eng.grm_ld_mask()), "ld")
        eng.grm_ld_clear()
        check(eng, code, spec_used(counts, n), "cleared")
        c2 = eng.compute(2)
        assert same_bits(c2[0], c0[0]) and same_bits(c2[1], c0[1])
        # a study ctx has a store and no used_v: every row counts
        want = vp.grm_king_pairs_rule(code, K.CUTOFF)
        got, found, n_rows = study.grm_king_pairs(K.CUTOFF, rows="all")
        assert found == want.size and same_bits(got, want) and n_rows == v
        for g, w in zip(study.grm_king_block(0, 40, 200, 60, "all"), vp.grm_king_rule(code)):
            assert np.array_equal(g, w[:40, 200:])


# ---- 6. refusals and statistics ---------------------------------------------------------------------------------------------
def test_refusals_and_statistics(P, vp, edge):
    L = P._lib
    lib = L.load()
    v, n = edge.shape
    vpt = ctypes.c_void_p
    buf = np.zeros(16, dtype=P.PcoaEngine.KING_PAIR_DTYPE)
    out = [np.zeros((n, n), dtype=np.int32) for _ in range(3)]

    def pairs(ctx, kind=0, x=0.177, band=0, dst=True, cap=16, found=True):
        got = ctypes.c_int64(0)
        return lib.pcoa_grm_king_pairs(ctx, kind, x, band, vpt(buf.ctypes.data) if dst else None, cap, ctypes.byref(got) if found else None,
                                       None, None)

    def block(ctx, kind=0, r0=0, r=4, c0=0, c=4, outs=(1, 1, 1)):
        ptrs = [vpt(o.ctypes.data) if m else None for o, m in zip(out, outs)]
        return lib.pcoa_grm_king_block(ctx, kind, r0, r, c0, c, ptrs[0], ptrs[1], ptrs[2], 0)

    assert pairs(None) == L.PCOA_ERR_INVALID_ARG and b"pcoa_grm_king_pairs: ctx is NULL" in lib.pcoa_last_error(None)
    assert block(None) == L.PCOA_ERR_INVALID_ARG and b"pcoa_grm_king_block: ctx is NULL" in lib.pcoa_last_error(None)
    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(n) as full, P.PcoaEngine(n, operator=True) as op, \
            P.PcoaEngine(n, grm_study=True) as study:
        fill(eng, edge)
        fill(study, edge)
        c0 = eng.compute(2)
        eng.reset_timings()
        for kw in (dict(found=False), dict(kind=2), dict(kind=-1), dict(x=float("nan")), dict(x=float("inf")), dict(x=0.0), dict(x=-0.1),
                   dict(x=0.5000001), dict(band=-64), dict(band=32), dict(band=100), dict(cap=-1), dict(dst=False)):
            assert pairs(eng._ctx, **kw) == L.PCOA_ERR_INVALID_ARG, kw
            assert b"pcoa_grm_king_pairs: " in lib.pcoa_last_error(eng._ctx) and len(lib.pcoa_last_error(eng._ctx)) > 30
        for kw in (dict(kind=2), dict(r=0), dict(c=0), dict(r0=-1), dict(c0=-1), dict(r0=n - 3), dict(c0=n - 3), dict(r=n + 1),
                   dict(outs=(0, 0, 0))):
            assert block(eng._ctx, **kw) == L.PCOA_ERR_INVALID_ARG, kw
            assert b"pcoa_grm_king_block: " in lib.pcoa_last_error(eng._ctx) and len(lib.pcoa_last_error(eng._ctx)) > 30
        for other, word in ((full, "full engine"), (op, "operator")):
            for call in (lambda e: e.grm_king_pairs(0.177), lambda e: e.grm_king_block(0, 4, 0, 4)):
                with pytest.raises(P.PcoaError) as ei:
                    call(other)
                assert ei.value.code == L.PCOA_ERR_STATE and word in str(ei.value) and "not a GRM ctx" in str(ei.value)
        for call in (lambda e: e.grm_king_pairs(0.177, rows="used"), lambda e: e.grm_king_block(0, 4, 0, 4, "used")):
            with pytest.raises(P.PcoaError) as ei:
                call(study)
            assert ei.value.code == L.PCOA_ERR_STATE and "PCOA_GRM_ROWS_USED on a GRM study ctx" in str(ei.value)
        with pytest.raises(ValueError):
            eng.grm_king_pairs(0.177, rows="some")
        st = eng.grm_king_stats()
        assert st["grm_king_calls"] == 0 and st["grm_king_bands"] == 0 and st["grm_king_bytes"] == 0 and st["grm_king_block_calls"] == 0
        assert st["grm_king_macs"] == 0 and st["grm_king_seconds"] == 0
        # the ctx is usable after every refusal; the statistics advance: 130 rows in bands of 64 are 3 bands of 3, 2 and 1 tiles of
        # 64 x 64, over the one segment's 300 rows in k-steps of 32
        want = vp.grm_king_pairs_rule(edge, 0.0442)
        got, found, _ = eng.grm_king_pairs(0.0442, band_rows=64)
        assert found == want.size > 0 and same_bits(got, want)
        st = eng.grm_king_stats()
        assert st["grm_king_calls"] == 1 and st["grm_king_bands"] == 3 and st["grm_king_block_calls"] == 0
        assert st["grm_king_macs"] == 4.0 * 64 * 64 * (3 + 2 + 1) * 320
        assert st["grm_king_bytes"] >= 12 * (64 * 130 + 64 * 66 + 2 * 2) and st["grm_king_seconds"] >= st["grm_king_screen_seconds"] > 0
        eng.grm_king_pairs(0.0442)
        eng.grm_king_block(0, n, 0, n)
        st2 = eng.grm_king_stats()
        assert st2["grm_king_calls"] == 2 and st2["grm_king_bands"] == 4 and st2["grm_king_block_calls"] == 1
        assert st2["grm_king_macs"] == st["grm_king_macs"] + 2 * 4.0 * 192 * 192 * 320
        c1 = eng.compute(2)
        assert same_bits(c1[0], c0[0]) and same_bits(c1[1], c0[1]) and c1[2] == c0[2]
        # no counted row
        eng.reset()
        for kind in ("all", "used"):
            with pytest.raises(P.PcoaError) as ei:
                eng.grm_king_pairs(0.177, rows=kind)
            assert ei.value.code == L.PCOA_ERR_STATE and "none of the 0 variants" in str(ei.value)
        eng.accumulate_plink_bed(pack_bed(np.full((5, n), 3, np.uint8)))
        with pytest.raises(P.PcoaError) as ei:
            eng.grm_king_pairs(0.177, rows="used")
        assert ei.value.code == L.PCOA_ERR_STATE and "none of the 5 variants" in str(ei.value)
        assert eng.grm_king_pairs(0.177, rows="all")[1:] == (0, 5)                            # five rows without a het: no pair
        eng.reset()
        fill(eng, edge)
        assert eng.grm_king_pairs(0.0442, band_rows=64)[1] == found


# ---- 7. hosts ---------------------------------------------------------------------------------------------------------------
def test_both_hosts_screen_remove_and_project_alike(tmp_path, vp):
    code = K.codes(K.HOST_N, K.HOST_V)
    n = K.HOST_N
    names = [K.name_of(i) for i in range(n)]
    prefix = str(tmp_path / "set" / "cohort")
    K.write_plink(code, prefix, names)
    want = vp.grm_king_pairs_rule(code, K.CUTOFF)
    assert [(int(p["i"]), int(p["j"])) for p in want] == K.planted_pairs(n)
    gone = vp.related_removal(want, n)
    assert 0 < gone.size < n - 32
    outs = {}
    for tag, run in (("cpp", K.run_driver), ("py", K.run_python)):
        f = str(tmp_path / ("king_%s.tsv" % tag))
        res = run(["--input-path", prefix + ".bed", "--grm", "--grm-king-cutoff", "0.177", "--grm-king-rows", "all",
                   "--grm-king-output-path", f, "--grm-king-remove", "--grm-project-removed"])
        assert res.returncode == 0, res.stderr[-2000:]
        outs[tag] = (open(f, "rb").read(), [ln for ln in res.stderr.splitlines() if ln.startswith("GRM KING:")], res.stdout)
    assert outs["cpp"][0] == outs["py"][0]                                        # the pair files, byte for byte
    assert outs["cpp"][1] == outs["py"][1] == ["GRM KING: %d pair(s) with kinship >= 0.177 over %d row(s) (rows all), removed %d sample(s)"
                                               % (want.size, K.HOST_V, gone.size)]
    assert outs["cpp"][2] == outs["py"][2]                                        # the coordinates
    # the file --king-cutoff writes for the same fileset through five plane engines
    f = str(tmp_path / "king_planes.tsv")
    res = K.run_driver(["--input-path", prefix + ".bed", "--king-cutoff", "0.177", "--king-output-path", f])
    assert res.returncode == 0, res.stderr[-2000:]
    assert open(f, "rb").read() == outs["cpp"][0]
    assert len(outs["cpp"][0].decode().splitlines()) == 1 + want.size
    # every sample gets a row: the kept ones, then the removed ones placed on their axes
    known = set(names)
    rows = [ln.split("\t")[0] for ln in outs["cpp"][2].splitlines() if ln.split("\t")[0] in known]
    stay = np.setdiff1d(np.arange(n), gone)
    assert rows == [names[i] for i in stay] + [names[i] for i in gone]

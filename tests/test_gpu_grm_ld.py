"""GPU tests of the LD prune of a GRM engine's resident store (pcoa_grm_ld_*, --grm-ld-window).  Masks and counts
are compared EXACTLY with the numpy rule of tests/grm_ld_cohort.py: the rule is integer up to one comparison and leaves no room
for a tolerance.  The shapes are those at which tests/test_grm_ld_cpu.py shows that a kernel which ignores missing calls, or a
pass that is not greedy, gives another mask."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import grm_ld_cohort as C
from conftest import ROOT, align_sign, load_pkg
from test_grm_cpu import pack_bed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return load_pkg()


def kernel_constant(name):
    """a constexpr int of grm_ld.hip: the tests of the kernel's edges take its tile and chunk sizes from the kernel"""
    src = open(os.path.join(ROOT, "spark-examples_amd", "csrc", "grm_ld.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


BAND_TILE_ROWS = kernel_constant("GLD_TR")               # target rows of a band tile
BAND_CHUNK_SAMPLES = kernel_constant("GLD_KW") * 16      # samples of the sample axis the band kernel stages per step


@functools.lru_cache(maxsize=None)
def cohort(n, v, seed=None):
    g = C.cohort(n, v, 100 + n if seed is None else seed)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def exceeds(n, v, t, seed=None):
    return C.exceeds_matrix(cohort(n, v, seed), t)


def want_of(n, v, w, t, breaks=(), seed=None, min_maf=0.0):
    g = cohort(n, v, seed)
    cand = C.candidates(g, min_maf)
    keep = C.greedy(exceeds(n, v, t, seed), cand, w, breaks)
    return keep, int(cand.sum()), int(keep.sum()), C.window_pairs(v, w, breaks)


def fill(eng, g, form="host", cuts=None):
    """host: rows with garbage in the padding slots and three extra row bytes; device: a torch tensor of the plain rows"""
    codes = C.to_codes(g)
    rows = pack_bed(codes, 3, np.random.default_rng(9)) if form == "host" else pack_bed(codes)
    edges = [0] + sorted(cuts or []) + [rows.shape[0]]
    for a, b in zip(edges[:-1], edges[1:]):
        part = np.ascontiguousarray(rows[a:b])
        if form == "device":
            import torch
            part = torch.from_numpy(part).cuda()
        eng.accumulate_plink_bed(part)
    eng.sync()


def check(eng, want, w, t, breaks=()):
    keep, cand, kept, pairs = want
    got = eng.grm_ld_prune(w, t, breaks)
    mask = eng.grm_ld_mask()
    st = eng.grm_ld_stats()
    assert np.array_equal(mask, keep), (np.flatnonzero(mask != keep)[:10], w, t)
    assert got == (cand, kept)
    assert (st["grm_ld_variants"], st["grm_ld_candidates"], st["grm_ld_kept"], st["grm_ld_pairs"]) == (keep.size, cand, kept, pairs)
    assert eng.grm_info()[1] == kept
    return mask


# ---- the five shapes, two input forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("n,v,w,t", C.SHAPES)
def test_mask_counts_and_pairs_equal_the_rule(P, n, v, w, t, form):
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, cohort(n, v), form)
        check(eng, want_of(n, v, w, t), w, t)


# ---- edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 47, 48, 49, 63, 64, 65, BAND_CHUNK_SAMPLES - 1, BAND_CHUNK_SAMPLES, BAND_CHUNK_SAMPLES + 1])
def test_sample_axis_edges(P, n):
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, cohort(n, 130))
        check(eng, want_of(n, 130, 7, .5), 7, .5)


def test_window_edges(P):
    n, v = 70, 1100
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, cohort(n, v))
        for w in (1, 63, 64, 65, 1024):
            check(eng, want_of(n, v, w, .5), w, .5)


@pytest.mark.parametrize("v,w", [(BAND_TILE_ROWS - 1, 40), (BAND_TILE_ROWS, 40), (BAND_TILE_ROWS + 1, 40), (20, 50), (1, 5)])
def test_tile_row_edges_a_store_shorter_than_the_window_and_one_row(P, v, w):
    n = 70
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, cohort(n, v))
        check(eng, want_of(n, v, w, .5), w, .5)
        if v == 1:
            assert eng.grm_ld_mask().tolist() == [True] and eng.grm_ld_stats()["grm_ld_pairs"] == 0


def test_cov_needs_int64(P):
    """N = 70,000: n p passes 2^31 for in-window pairs whose r^2 lies within a factor 2 of t, so a kernel that forms cov in int32
    decides them from garbage."""
    n, v, w, t = 70000, 130, 7, .5
    g = cohort(n, v)
    band, n_p, ratio = C.exceeds_band(g, w, t, stats=True)
    assert np.any((n_p > 2 ** 31) & (ratio > t / 2) & (ratio < 2 * t))
    cand = C.candidates(g)
    keep = C.greedy_band(band, cand, w)
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, g)
        check(eng, (keep, int(cand.sum()), int(keep.sum()), C.window_pairs(v, w)), w, t)


# ---- segments -------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(tests)r)
import grm_ld_cohort as C
from conftest import load_pkg
from test_grm_cpu import pack_bed
P = load_pkg()
n, v = 130, 700
g = C.cohort(n, v, 100 + n)
rows = pack_bed(C.to_codes(g))
with P.PcoaEngine(n, grm=True) as eng:
    for a, b in ((0, 50), (50, 97), (97, 500), (500, v)):
        eng.accumulate_plink_bed(np.ascontiguousarray(rows[a:b]))
    info = eng.grm_info()
    assert info[0] == v and info[2] == -(-v // 96) * 96 * 48, info   # segments of 96 rows of 48 bytes
    for w in (64, 65, 200):
        keep, cand, kept, pairs = C.rule(g, w, .5)
        assert eng.grm_ld_prune(w, .5) == (cand, kept)
        mask = eng.grm_ld_mask()
        assert np.array_equal(mask, keep), w
        assert eng.grm_ld_stats()["grm_ld_pairs"] == pairs and eng.grm_info()[1] == kept
        print("MASK %%d %%s" %% (w, np.packbits(mask).tobytes().hex()))
print("SEGMENTS-OK")
"""


def test_windows_across_segment_boundaries(P):
    """Segments of 96 rows: a window of 64 or 65 straddles one boundary, a window of 200 more than two whole segments.  The mask
    equals the rule and the mask of an engine with the default segment size."""
    env = dict(os.environ)
    env["PCOA_GRM_SEGMENT_ROWS"] = "96"
    res = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests")}], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0 and "SEGMENTS-OK" in res.stdout, res.stdout[-3000:]
    masks = dict((int(m.group(1)), m.group(2)) for m in re.finditer(r"MASK (\d+) ([0-9a-f]+)", res.stdout))
    n, v = 130, 700
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, cohort(n, v))
        for w in (64, 65, 200):
            eng.grm_ld_prune(w, .5)
            assert np.packbits(eng.grm_ld_mask()).tobytes().hex() == masks[w], w


def test_ragged_calls_give_the_same_mask(P):
    n, v, w, t = 130, 1000, 64, .5
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, cohort(n, v), cuts=[1, 7, 64, 65, 333, 999])
        check(eng, want_of(n, v, w, t), w, t)


# ---- breaks, thresholds, min_maf ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("breaks", [(1,), (699,), (1, 64, 65, 300, 699), (350,)])
def test_a_prune_with_breaks_equals_separate_engines(P, breaks):
    n, v, w, t = 70, 700, 7, .2
    g = cohort(n, v)
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, g)
        mask = check(eng, want_of(n, v, w, t, breaks), w, t, breaks)
    parts = []
    edges = [0] + list(breaks) + [v]
    with P.PcoaEngine(n, grm=True) as eng:
        for a, b in zip(edges[:-1], edges[1:]):
            eng.reset()
            fill(eng, g[a:b])
            eng.grm_ld_prune(w, t)
            parts.append(eng.grm_ld_mask())
    assert np.array_equal(np.concatenate(parts), mask)
    assert not np.array_equal(mask, want_of(n, v, w, t)[0]) or breaks in ((1,), (699,))   # (a break in the middle moves the mask)


@pytest.mark.parametrize("t", [0.0, 1.0])
def test_thresholds_at_the_ends_equal_the_rule(P, t):
    n, v, w = 130, 1000, 64
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, cohort(n, v))
        mask = check(eng, want_of(n, v, w, t), w, t)
    cand = C.candidates(cohort(n, v))
    assert (mask.sum() < cand.sum()) if t == 0.0 else True   # rows 8 and 9 are duplicates: r^2 = 1 > 0, but not > 1


def test_a_row_below_min_maf_is_no_candidate_and_blocks_nobody(P):
    """Rows 20 and 22 are near copies, row 21 between them has a minor-allele frequency of 4 / 140.  Under min_maf = 0.1 row 21
    is removed and blocks nobody; the window counts store rows, so with W = 1 row 22 sees row 21 alone and is kept, with W = 2 it
    sees row 20 and is removed."""
    n, v = 70, 60
    rng = np.random.default_rng(7)
    g = np.array(cohort(n, v, 7))
    base = (rng.random(n) < .4).astype(np.int8) + (rng.random(n) < .4).astype(np.int8)
    g[20] = base
    g[22] = base
    g[22, :2] = -1
    g[21] = 0
    g[21, 10:14] = 1
    g.setflags(write=False)
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, g)
        eng.grm_set_min_maf(0.1)
        masks = {}
        for w in (1, 2):
            keep, cand, kept, pairs = C.rule(g, w, .5, min_maf=0.1)
            masks[w] = check(eng, (keep, cand, kept, pairs), w, .5)
            assert cand < C.candidates(g).sum() and not keep[21]
        assert masks[1][20] and masks[1][22] and masks[2][20] and not masks[2][22]
        eng.grm_set_min_maf(0.0)
        keep0 = C.rule(g, 1, .5)
        check(eng, keep0, 1, .5)
        assert keep0[0][21]


# ---- downstream -----------------------------------------------------------------------------------------------------------------
def test_every_grm_consumer_sees_the_pruned_store(P):
    from test_gpu_grm_dense import entry_bound
    rule_k = load_pkg("variants_pca").grm_dense_rule
    n, v, w, t = 260, 1000, 65, .8
    g = cohort(n, v)
    codes = C.to_codes(g)
    keep = want_of(n, v, w, t)[0]
    want_k, want_n = rule_k(codes[keep], False, 0.0, "used")
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, g)
        check(eng, want_of(n, v, w, t), w, t)
        k = eng.grm_dense("used")
        assert np.all(np.abs(k - want_k) <= entry_bound(codes[keep], False, 0.0, want_n, "used"))
        comps, lam, _ = eng.compute(2)
        assert np.array_equal(eng.grm_ld_mask(), keep)                       # the mask is kept across compute
        ev, vec = np.linalg.eigh(want_k)
        assert np.allclose(lam, ev[::-1][:2], rtol=1e-6, atol=0)
        want_vec = vec[:, ::-1][:, :2]
        assert np.abs(align_sign(comps, want_vec) - want_vec).max() < 1e-6
        wts = eng.grm_weights(comps, lam, scaled=True)
        assert not wts[~keep].any() and wts[keep].any(axis=1).all()
        own, _ = eng.grm_project(eng, comps, lam)
        assert np.abs(own - comps).max() < 1e-9


# ---- the life of the mask -------------------------------------------------------------------------------------------------------
def test_mask_lifetime(P):
    from test_gpu_grm import product
    n, v = 70, 700
    g = cohort(n, v)
    unpruned = int(C.candidates(g).sum())
    rows = pack_bed(C.to_codes(g))
    x = np.random.default_rng(5).standard_normal(n)
    with P.PcoaEngine(n, grm=True) as eng:
        fill(eng, g)

        def prune():
            return check(eng, want_of(n, v, 7, .2), 7, .2)

        def dropped():
            with pytest.raises(P.PcoaError) as ei:
                eng.grm_ld_mask()
            return ei.value.code == P._lib.PCOA_ERR_STATE and "no keep mask" in str(ei.value)

        def twin_product(store, window=None, min_maf=0.0):
            """a product of this engine, right after a transition, has the bits of a fresh engine brought straight to the same
            state: the store's rows in one call, min_maf, and the prune where one is installed"""
            with P.PcoaEngine(n, grm=True) as twin:
                if store.shape[0]:
                    fill(twin, store)
                twin.grm_set_min_maf(min_maf)
                if window is not None:
                    twin.grm_ld_prune(window, .2)
                want = product(twin, x)
            return product(eng, x).tobytes() == want.tobytes()

        assert dropped() and eng.grm_info()[1] == unpruned                   # nothing installed yet
        assert twin_product(g)
        first = prune()
        assert twin_product(g, 7)
        eng.grm_set_min_maf(0.0)                                             # the same value keeps it
        assert twin_product(g, 7)
        eng.compute(2)
        assert np.array_equal(eng.grm_ld_mask(), first) and eng.grm_info()[1] == first.sum()
        assert twin_product(g, 7)
        check(eng, want_of(n, v, 64, .2), 64, .2)                            # a second prune is a first prune with that window
        assert twin_product(g, 64)
        prune()
        assert twin_product(g, 7)
        eng.grm_ld_clear()
        assert twin_product(g)
        assert dropped() and eng.grm_info()[1] == unpruned
        prune()
        eng.grm_set_min_maf(0.05)                                            # another value drops it
        assert twin_product(g, min_maf=0.05)
        assert dropped() and eng.grm_info()[1] == int(C.candidates(g, 0.05).sum())
        eng.grm_set_min_maf(0.0)
        assert twin_product(g)
        prune()
        eng.accumulate_plink_bed(np.ascontiguousarray(rows[:3]))             # an append drops it
        assert twin_product(np.concatenate([g, g[:3]]))
        assert dropped() and eng.grm_info()[:2] == (v + 3, unpruned + int(C.candidates(g[:3]).sum()))
        eng.reset()
        fill(eng, g)
        prune()
        eng.reset()                                                          # and so does a reset
        assert twin_product(g[:0])
        assert dropped() and eng.grm_info()[0] == 0
        assert eng.grm_ld_prune(5, .5) == (0, 0) and eng.grm_ld_mask().size == 0   # V = 0
        fill(eng, g)
        assert twin_product(g)
        assert dropped()
        prune()
        assert twin_product(g, 7)


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_ctx_the_store_and_an_earlier_mask_as_they_were(P):
    import ctypes
    import torch
    L = P._lib
    lib = L.load()
    n, v = 70, 700
    g = cohort(n, v)
    x = torch.from_numpy(np.random.default_rng(3).standard_normal(n)).cuda()
    i64 = ctypes.c_int64

    def raw(ctx, w, t, breaks=None, nb=None):
        arr = (i64 * max(len(breaks or ()), 1))(*(breaks or ()))
        return lib.pcoa_grm_ld_prune(ctx, w, ctypes.c_double(t), arr if breaks is not None else None,
                                     len(breaks or ()) if nb is None else nb, None, None)

    with P.PcoaEngine(n, grm=True) as eng, P.PcoaEngine(n) as full, P.PcoaEngine(n, operator=True) as op, \
            P.PcoaEngine(n, grm_study=True) as study:
        fill(eng, g)
        fill(study, g)
        first = check(eng, want_of(n, v, 7, .2), 7, .2)
        y0 = eng.grm_matvec_device(x).cpu().numpy()
        bad = [(0, .5, None, None), (L.PCOA_LD_MAX_WINDOW + 1, .5, None, None), (-3, .5, None, None), (7, -0.1, None, None),
               (7, 1.5, None, None), (7, float("nan"), None, None), (7, .5, None, 2), (7, .5, [5], -1), (7, .5, [0], None),
               (7, .5, [v], None), (7, .5, [5, 5], None), (7, .5, [9, 4], None), (7, .5, [-1], None)]
        for w, t, breaks, nb in bad:
            assert raw(eng._ctx, w, t, breaks, nb) == L.PCOA_ERR_INVALID_ARG, (w, t, breaks, nb)
            assert b"pcoa_grm_ld_prune" in lib.pcoa_last_error(eng._ctx)
        for other, word in ((full, "full engine"), (op, "operator")):
            for call in (lambda: other.grm_ld_prune(7, .5), lambda: other.grm_ld_mask(0, 0), lambda: other.grm_ld_clear()):
                with pytest.raises(P.PcoaError) as ei:
                    call()
                assert ei.value.code == L.PCOA_ERR_STATE and word in str(ei.value)
        with pytest.raises(P.PcoaError) as ei:
            study.grm_ld_prune(7, .5)
        assert ei.value.code == L.PCOA_ERR_STATE and "study" in str(ei.value)
        for args in ((-1, 2), (0, v + 1), (v, 1)):
            with pytest.raises(P.PcoaError) as ei:
                eng.grm_ld_mask(*args)
            assert ei.value.code == L.PCOA_ERR_INVALID_ARG
        with pytest.raises(P.PcoaError) as ei:   # the carrier pruner stays refused on a GRM ctx
            eng.ld_pruner(7, .5, accumulate=False)
        assert ei.value.code == L.PCOA_ERR_STATE
        # the mask, M' and a product are what they were
        assert np.array_equal(eng.grm_ld_mask(), first) and eng.grm_info()[1] == first.sum()
        assert eng.grm_matvec_device(x).cpu().numpy().tobytes() == y0.tobytes()
        assert np.array_equal(eng.grm_ld_mask(5, 20), first[5:25])


# ---- hosts ----------------------------------------------------------------------------------------------------------------------
def write_plink(prefix, g, contigs):
    n = g.shape[1]
    with open(prefix + ".fam", "w") as f:
        for i in range(n):
            f.write("FAM%d S%04d 0 0 0 -9\n" % (i, i))
    with open(prefix + ".bim", "w") as f:
        for k in range(g.shape[0]):
            f.write("%s\trs%d\t0\t%d\tC\tA\n" % (contigs[k], k, 1000 + 7 * k))
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6c, 0x1b, 0x01]))
        f.write(pack_bed(C.to_codes(g)).tobytes())


def coords_of(stdout):
    rows = [line.split("\t") for line in stdout.splitlines() if line.count("\t") == 3]
    return np.array([[float(r[-2]), float(r[-1])] for r in rows])


def test_both_hosts_prune_write_the_mask_and_decompose_the_kept_variants(tmp_path):
    from test_grm_cpu import _run_driver, _run_python
    n, v, w, t, cut = 70, 300, 7, .2, 140
    g = np.array(cohort(n, v, 170))
    g[cut:cut + 3] = g[cut - 3:cut]            # the first rows of contig 2 repeat the last of contig 1
    contigs = ["1"] * cut + ["2"] * (v - cut)
    keep, cand, kept, _ = C.rule(g, w, t, breaks=(cut,))
    assert not np.array_equal(keep, C.rule(g, w, t)[0])                      # without the break the mask is another
    write_plink(str(tmp_path / "two"), g, contigs)
    write_plink(str(tmp_path / "kept"), g[keep], [c for c, k in zip(contigs, keep) if k])
    want_file = "".join("%d\t%s\t%d\trs%d\t%d\n" % (k, contigs[k], 1000 + 7 * k, k, 1 if keep[k] else 0) for k in range(v))
    for tag, run in (("cpp", _run_driver), ("py", _run_python)):
        out = str(tmp_path / ("mask_%s.tsv" % tag))
        res = run(["--input-path", str(tmp_path / "two.bed"), "--all-references", "--grm", "--grm-ld-window", str(w), "--grm-ld-r2", str(t),
                   "--grm-ld-output-path", out])
        assert res.returncode == 0, res.stderr[-2000:]
        assert "GRM LD pruning: kept %d of %d candidate variants (%d in the store), window %d, r2 %g" % (kept, cand, v, w, t) \
            in res.stdout, res.stdout[:500]
        assert open(out).read() == want_file
        plain = run(["--input-path", str(tmp_path / "kept.bed"), "--all-references", "--grm"])
        assert plain.returncode == 0, plain.stderr[-2000:]
        a, b = coords_of(res.stdout), coords_of(plain.stdout)
        assert a.shape == (n, 2) and b.shape == (n, 2)
        assert np.abs(align_sign(a, b) - b).max() < 1e-6

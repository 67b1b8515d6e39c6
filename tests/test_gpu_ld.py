"""GPU tests of the LD pruner (pcoa_ld_*, csrc/ld.hip): the keep mask and the counts in the stats equal the numpy statement of
the rule in ld_cohort.py EXACTLY -- integers and three fp64 products, nothing to tolerate -- with the bits of samples >= N and
every pad word set; every split of the rows over calls, .bed rows, host and device pointers give the same mask; a break equals
two runs; PCOA_LD_ACCUMULATE leaves the S (or the store) of the kept rows; every error leaves the ctx and the carried rows
usable."""
import ctypes

import numpy as np
import pytest

from conftest import ROOT, align_sign, load_pkg
from ld_cohort import decode_bed, encode_bed, ld_cohort, ld_pairs, ld_rule, pack_rows

pytestmark = pytest.mark.gpu

# (n, V, W, t).  The band kernel stages 16 words = 512 samples of the sample axis at a time and a workgroup owns 64 target rows:
# n = 2,504 and 4,100 take 5 and 9 such steps, n = 600 two with a ragged second (19 words), and V = 131 = 2 x 64 + 3,
# 300 = 4 x 64 + 44, 700, 1,000 all leave a ragged last tile; W = 65 / 200 / 1,024 span 2 / 4 / 16 distance tiles of 64
SHAPES = [(33, 300, 1, 0.5), (70, 700, 7, 0.2), (130, 1000, 64, 0.5), (260, 1000, 65, 0.8), (2504, 600, 50, 0.2),
          (4100, 300, 200, 0.5), (600, 131, 9, 0.3)]

_REF = {}


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def L():
    return load_pkg("_lib")


def reference(n, v, w, t, breaks=()):
    """(x, keep) of the shape's cohort, computed once and never modified."""
    key = (n, v, w, t, tuple(breaks))
    if key not in _REF:
        x = ld_cohort(n, v, 1000 + n)
        x.setflags(write=False)
        keep = ld_rule(x, w, t, breaks)
        keep.setflags(write=False)
        _REF[key] = (x, keep)
    return _REF[key]


def to_dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dtype) if dtype is not None else a).cuda()


def feed(pr, bits, cuts=None, in_dev=False):
    """The rows in calls that end at `cuts` (None: one call); the concatenated mask."""
    edges = [0] + sorted(set(c for c in (cuts or []) if 0 < c < len(bits))) + [len(bits)]
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        part = bits[a:b]
        out.append(pr.bits(to_dev(part, np.int32) if in_dev else part))
    return np.concatenate(out) if out else np.zeros(0, dtype=bool)


def check_stats(st, x, keep, w, breaks=(), times=1):
    n = x.shape[1]
    a = x.sum(axis=1)
    assert st["ld_variants"] == times * len(x)
    assert st["ld_kept"] == times * int(keep.sum())
    assert st["ld_monomorphic"] == times * int(((a == 0) | (a == n)).sum())
    assert st["ld_pairs"] == times * ld_pairs(len(x), w, breaks)


# ---- 1. the rule, exactly ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,v,w,t", SHAPES)
def test_mask_and_counts_equal_the_rule(P, n, v, w, t):
    """Host and device pointers, the dense pitch and a padded one; tail bits and pad words are all ones."""
    x, keep = reference(n, v, w, t)
    assert not keep[3] and not keep[5] and not (keep[8] and keep[9] and t < 1)
    rng = np.random.default_rng(n)
    calls = 0
    with P.PcoaEngine(n) as eng:
        for pad in (0, 3):
            bits = pack_rows(x, n, pad_words=pad, garbage=rng)
            for in_dev in (False, True):
                eng.reset_timings()
                with eng.ld_pruner(w, t, accumulate=False) as pr:
                    got = feed(pr, bits, in_dev=in_dev)
                    st = pr.stats()
                calls += 1
                print("n=%d V=%d W=%d t=%g pad=%d dev=%d: kept %d of %d, %d differ" % (n, v, w, t, pad, in_dev, got.sum(), v,
                                                                                     (got != keep).sum()))
                assert got.dtype == np.bool_ and np.array_equal(got, keep), (pad, in_dev, np.flatnonzero(got != keep)[:10])
                assert pr.last_kept == int(keep.sum())
                check_stats(st, x, keep, w)
                assert st["ld_band_seconds"] > 0 and st["ld_resolve_seconds"] > 0 and st["ld_count_seconds"] > 0
        assert not eng.gram().any()      # a dry run: S is untouched


# ---- 2. independence of the split -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,v,w,t", [(70, 700, 7, 0.2), (130, 1000, 64, 0.5), (260, 1000, 65, 0.8), (2504, 600, 50, 0.2)])
def test_every_split_of_the_rows_equals_one_call(P, n, v, w, t):
    x, keep = reference(n, v, w, t)
    bits = pack_rows(x, n)
    blocks = np.cumsum([1, 63, 64, w - 1]).tolist()               # 1 + 63 + 64 + (W - 1) + rest
    singles = list(range(1, 2 * w + 1))                           # single rows for the first 2 W
    with P.PcoaEngine(n) as eng:
        for i, cuts in enumerate((blocks, singles)):
            with eng.ld_pruner(w, t, accumulate=False) as pr:
                got = feed(pr, bits, cuts, in_dev=bool(i))
            assert np.array_equal(got, keep), (cuts[:6], np.flatnonzero(got != keep)[:10])


# ---- 3. breaks and reset ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,v,w,t", [(130, 1000, 64, 0.5), (2504, 600, 50, 0.2)])
def test_a_break_equals_two_runs_and_reset_drops_the_tail(P, n, v, w, t):
    x, keep = reference(n, v, w, t)
    bits = pack_rows(x, n)
    a = x.sum(axis=1)
    cut = int(np.flatnonzero(~keep & (a > 0) & (a < n) & (np.arange(v) >= v // 2))[0])   # a row that an earlier row removes
    first, second = ld_rule(x[:cut], w, t), ld_rule(x[cut:], w, t)
    assert np.array_equal(np.concatenate([first, second]), ld_rule(x, w, t, breaks=[cut]))
    assert not np.array_equal(np.concatenate([first, second]), keep)     # the break matters on this cohort
    with P.PcoaEngine(n) as eng, eng.ld_pruner(w, t, accumulate=False) as pr:
        got = [pr.bits(bits[:cut])]
        pr.break_contig()
        got.append(pr.bits(bits[cut:]))
        assert np.array_equal(got[0], first) and np.array_equal(got[1], second)
        check_stats(pr.stats(), x, np.concatenate([first, second]), w, breaks=[cut])
        eng.reset()                                                      # pcoa_reset: the next row starts a new window too
        assert np.array_equal(pr.bits(bits[cut:]), second)
        assert np.array_equal(pr.bits(bits[:cut]), ld_rule(np.concatenate([x[cut:], x[:cut]]), w, t)[v - cut:])


# ---- 4. PLINK rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,v,w,t", [(33, 300, 1, 0.5), (70, 700, 7, 0.2), (2504, 600, 50, 0.2)])     # N % 4 = 1, 2, 0
def test_bed_rows_equal_their_decoded_bitsets(P, n, v, w, t):
    x, _ = reference(n, v, w, t)
    rng = np.random.default_rng(77 + n)
    with P.PcoaEngine(n) as eng:
        for a1 in (False, True):
            missing = rng.random((v, n)) < 0.02
            bed = encode_bed(x, n, missing=missing, ref_is_a1=a1, rng=rng)
            carriers = decode_bed(bed, n, ref_is_a1=a1)
            want = ld_rule(carriers, w, t)
            with eng.ld_pruner(w, t, accumulate=False) as pr:
                from_bits = pr.bits(pack_rows(carriers, n))
            with eng.ld_pruner(w, t, accumulate=False) as pr:
                host = np.concatenate([pr.plink_bed(bed[:100], ref_is_a1=a1), pr.plink_bed(bed[100:], ref_is_a1=a1)])
            with eng.ld_pruner(w, t, accumulate=False) as pr:
                dev = pr.plink_bed(to_dev(bed), ref_is_a1=a1)
            assert np.array_equal(from_bits, want) and np.array_equal(host, want) and np.array_equal(dev, want), (n, a1)


# ---- 5. thresholds ----------------------------------------------------------------------------------------------------------
def test_threshold_one_keeps_every_polymorphic_row(P):
    n, v, w = 130, 1000, 64
    x = np.array(reference(n, v, w, 0.5)[0])
    x[20] = 1 - x[19]                                  # a complement next to its row, beside the duplicate at 8 / 9
    a = x.sum(axis=1)
    poly = (a > 0) & (a < n)
    assert np.array_equal(ld_rule(x, w, 1.0), poly)
    with P.PcoaEngine(n) as eng, eng.ld_pruner(w, 1.0, accumulate=False) as pr:
        got = pr.bits(pack_rows(x, n))
    assert np.array_equal(got, poly) and got[8] and got[9] and got[19] and got[20]


def test_threshold_zero_removes_every_row_with_a_nonzero_d(P):
    n, v, w = 130, 1000, 64
    x, _ = reference(n, v, w, 0.5)
    want = ld_rule(x, w, 0.0)
    assert 0 < want.sum() < 0.2 * v
    with P.PcoaEngine(n) as eng, eng.ld_pruner(w, 0.0, accumulate=False) as pr:
        got = pr.bits(pack_rows(x, n))
    assert np.array_equal(got, want)


def test_the_largest_window(P, L):
    n, v, w, t = 130, 1100, L.PCOA_LD_MAX_WINDOW, 0.5
    assert w == 1024
    x, keep = reference(n, v, w, t)
    bits = pack_rows(x, n)
    with P.PcoaEngine(n) as eng:
        with eng.ld_pruner(w, t, accumulate=False) as pr:
            one = pr.bits(bits)
            check_stats(pr.stats(), x, keep, w)
        with eng.ld_pruner(w, t, accumulate=False) as pr:
            parts = feed(pr, bits, [1, 500, 1030, 1031], in_dev=True)
    assert np.array_equal(one, keep) and np.array_equal(parts, keep)


# ---- 6. PCOA_LD_ACCUMULATE --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,v,w,t", [(130, 1000, 64, 0.5), (2504, 600, 50, 0.2)])
def test_accumulate_gives_the_s_of_the_kept_rows(P, n, v, w, t):
    """Fed in many small calls: the compacted buffer is rewritten by every call while the pre-pass of the call before is the
    only thing that orders its reads."""
    x, keep = reference(n, v, w, t)
    bits = pack_rows(x, n)
    cuts = list(range(7, v, 37))
    with P.PcoaEngine(n) as ref:
        ref.accumulate_bits(bits[keep])
        want = ref.gram()
    assert want.any()
    with P.PcoaEngine(n) as eng:
        with eng.ld_pruner(w, t) as pr:
            got = feed(pr, bits, cuts, in_dev=True)
            assert np.array_equal(got, keep)
            assert np.array_equal(eng.gram(), want)
        eng.reset()
        with eng.ld_pruner(w, t) as pr:                     # one call, host rows, all-ones tails
            assert np.array_equal(pr.bits(pack_rows(x, n, pad_words=2, garbage=np.random.default_rng(1))), keep)
        assert np.array_equal(eng.gram(), want)
        eng.reset()
        with eng.ld_pruner(w, t, accumulate=False) as pr:
            assert np.array_equal(feed(pr, bits, cuts), keep)
        assert not eng.gram().any()


def test_accumulate_on_an_operator_ctx_stores_exactly_the_kept_rows(P):
    n, v, w, t = 130, 1000, 64, 0.5
    x, keep = reference(n, v, w, t)
    bits = pack_rows(x, n)
    u = np.random.default_rng(9).integers(-8, 9, size=(n, 8)).astype(np.float64)
    with P.PcoaEngine(n) as full:
        full.accumulate_bits(bits[keep])
        comps_f, lam_f, nz_f = full.compute(2)
    with P.PcoaEngine(n, operator=True) as eng:
        with eng.ld_pruner(w, t) as pr:
            assert np.array_equal(feed(pr, bits, list(range(7, v, 37))), keep)
        assert eng.operator_info()[0] == int(keep.sum())
        with eng.loadings(u, None, centre=False, unit=False) as ld:      # integer vectors: the store's rows, exactly and in order
            assert np.array_equal(ld.operator(), x[keep].astype(np.float64) @ u)
        comps, lam, nz = eng.compute(2)
    assert nz == nz_f and np.max(np.abs(lam - lam_f) / np.abs(lam_f)) < 1e-6
    assert np.abs(align_sign(comps, comps_f) - comps_f).max() < 1e-6


# ---- 7. errors --------------------------------------------------------------------------------------------------------------
def test_every_error_leaves_the_ctx_and_the_carried_rows_usable(P, L):
    n, v, w, t = 70, 700, 7, 0.2
    x, keep = reference(n, v, w, t)
    bits = pack_rows(x, n)
    lib = L.load()
    kept = ctypes.c_int64(0)
    buf = np.zeros(v, dtype=np.uint8)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    with P.PcoaEngine(n) as eng:
        ctx = eng._ctx
        assert lib.pcoa_ld_bits(ctx, ptr(bits), 3, 3, 0, ptr(buf), ctypes.byref(kept)) == L.PCOA_ERR_STATE
        assert lib.pcoa_ld_plink_bed(ctx, ptr(bits), 3, 18, 0, 0, ptr(buf), ctypes.byref(kept)) == L.PCOA_ERR_STATE
        assert lib.pcoa_ld_break(ctx) == L.PCOA_ERR_STATE and lib.pcoa_ld_end(ctx) == 0
        for window, r2 in ((0, 0.2), (-1, 0.2), (1025, 0.2), (7, -0.01), (7, 1.01), (7, float("nan"))):
            assert lib.pcoa_ld_begin(ctx, window, r2, 0) == L.PCOA_ERR_INVALID_ARG, (window, r2)
        assert lib.pcoa_ld_begin(ctx, 7, 0.2, 2) == L.PCOA_ERR_INVALID_ARG
        with eng.ld_pruner(w, t, accumulate=False) as pr:
            got = [pr.bits(bits[:5])]                                   # shorter than the window: the tail is carried
            assert lib.pcoa_ld_begin(ctx, 0, 0.2, 0) == L.PCOA_ERR_INVALID_ARG     # a refused begin leaves the pruner as it was
            assert lib.pcoa_ld_bits(ctx, None, 3, 3, 0, ptr(buf), ctypes.byref(kept)) == L.PCOA_ERR_INVALID_ARG
            assert lib.pcoa_ld_bits(ctx, ptr(bits), -1, 3, 0, ptr(buf), ctypes.byref(kept)) == L.PCOA_ERR_INVALID_ARG
            assert lib.pcoa_ld_bits(ctx, ptr(bits), 3, 2, 0, ptr(buf), ctypes.byref(kept)) == L.PCOA_ERR_INVALID_ARG
            assert "ld_words" in eng._lib.pcoa_last_error(ctx).decode()
            assert lib.pcoa_ld_plink_bed(ctx, ptr(bits), 3, 17, 0, 0, ptr(buf), ctypes.byref(kept)) == L.PCOA_ERR_INVALID_ARG
            assert lib.pcoa_ld_plink_bed(ctx, ptr(bits), 3, 18, 0, 2, ptr(buf), ctypes.byref(kept)) == L.PCOA_ERR_INVALID_ARG
            assert lib.pcoa_ld_plink_bed(ctx, None, 3, 18, 0, 0, ptr(buf), ctypes.byref(kept)) == L.PCOA_ERR_INVALID_ARG
            assert lib.pcoa_get_ld_stats(ctx, None, 64) == L.PCOA_ERR_INVALID_ARG
            assert lib.pcoa_ld_bits(ctx, ptr(bits), 0, 3, 0, None, None) == 0       # nothing to do is not an error
            got.append(pr.bits(bits[5:]))
            assert np.array_equal(np.concatenate(got), keep)
            # NULL outputs are allowed; the rows still pass through the window
            assert lib.pcoa_ld_break(ctx) == 0
            assert lib.pcoa_ld_bits(ctx, ptr(bits), 100, 3, 0, None, None) == 0
            assert np.array_equal(pr.bits(bits[100:]), keep[100:])
    with pytest.raises(P.PcoaError):
        with P.PcoaEngine(n, gram_kernel="f32") as f32:
            f32.ld_pruner(w, t, accumulate=True)


# ---- 8. hosts ---------------------------------------------------------------------------------------------------------------
def host_rows(res):
    assert res.returncode == 0, res.stderr[-2000:]
    return [ln for ln in res.stdout.splitlines() if ln.count("\t") == 3]


@pytest.mark.parametrize("gram", ["stored", "implicit"])
def test_both_hosts_prune_a_fileset_of_two_contigs(gram, tmp_path):
    """--ld-output-path of both hosts, line for line, is the numpy rule with a break at the contig change; the coordinates are
    those of a run over a fileset that holds only the kept variants."""
    from ld_cohort import write_plink
    from test_operator_cpu import _run_driver, _run_python
    n, v, w, t = 70, 700, 7, 0.2
    x, keep_whole = reference(n, v, w, t)
    a = x.sum(axis=1)
    cut = int(np.flatnonzero(~keep_whole & (a > 0) & (a < n) & (np.arange(v) >= v // 2))[0])   # the break un-removes this row
    keep = ld_rule(x, w, t, breaks=[cut])
    assert keep[cut] and not keep_whole[cut]
    contigs = ["1"] * cut + ["2"] * (v - cut)
    (tmp_path / "all").mkdir()          # the same stem in two directories: the hosts print it as the dataset of every sample
    (tmp_path / "kept").mkdir()
    meta = write_plink(str(tmp_path / "all" / "cohort"), x, contigs)
    write_plink(str(tmp_path / "kept" / "cohort"), x[keep], [c for c, k in zip(contigs, keep) if k])
    want = "".join("%d\t%s\t%d\t%s\t%d\n" % (i, m[0], m[1], m[2], int(k)) for i, (m, k) in enumerate(zip(meta, keep)))
    mono = int(((a == 0) | (a == n)).sum())
    for run in (_run_driver, _run_python):
        out = str(tmp_path / ("mask-%s.tsv" % run.__name__))
        pruned = run(["--input-path", str(tmp_path / "all" / "cohort.bed"), "--all-references", "--gram", gram, "--ld-window", str(w), "--ld-r2",
                      str(t), "--ld-output-path", out])
        plain = run(["--input-path", str(tmp_path / "kept" / "cohort.bed"), "--all-references", "--gram", gram])
        rows = host_rows(pruned)
        assert len(rows) == n and rows == host_rows(plain), run.__name__
        assert "LD pruning: kept %d of %d variants (%d monomorphic)" % (keep.sum(), v, mono) in pruned.stdout
        assert "LD pruning" not in plain.stdout
        assert open(out).read() == want, run.__name__

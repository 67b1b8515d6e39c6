"""GPU tests of PCoA over a sample subset (pcoa_create_subset, PcoaEngine.subset, --outlier-iterations): S of a subset is
S[I, I] of the source to the last bit -- at the kernel's tile edges, past 2^31 entries, with an int64 part --, a subset is an
ordinary engine that gives the bits a fresh engine over the reduced cohort gives, errors leave the source usable, and both
hosts run the outlier rounds of tests/subset_cohort.py to the sets the oracle finds on the CPU (test_subset_cpu.py)."""
import re

import numpy as np
import pytest

import subset_cohort as C
from conftest import align_sign, int_gram, load_golden, load_oracle, load_pkg

pytestmark = pytest.mark.gpu

# the gather kernel's workgroup shape (csrc/pcoa_internal.h: kSubsetTileCols, kSubsetBandRows): a workgroup takes 32 dst rows
# x 1,024 dst columns, four rows in flight at a time, four columns per lane
TILE_COLS, BAND_ROWS = 1024, 32


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def L():
    return load_pkg("_lib")


@pytest.fixture(scope="module")
def ingest():
    return load_pkg("ingest")


def random_keep(rng, n, m):
    return np.sort(rng.choice(n, size=m, replace=False)).astype(np.int32)


def random_bits(rng, ingest, n, v, density=0.3):
    x = (rng.random((v, n)) < density).astype(np.float32)
    return x, ingest.pack_bits(x)


# ---- 1. exact S ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged16", "pops40", "tile130", "tile260"])
def test_subset_gram_is_the_sub_matrix_of_the_source(P, name):
    g = load_golden(name)
    n = int(g["n_samples"])
    rng = np.random.default_rng(40 + n)
    with P.PcoaEngine(n) as full:
        full.accumulate_calls(g["sample_idx"], g["row_offsets"])
        want = full.gram()
        assert np.array_equal(want, g["similarity"])
        sizes = sorted(set([1, 2, 3, n - 1] + [m for m in (n // 2 + r for r in range(4))] + [m for m in (31, 33) if m < n]))
        assert set(m % 4 for m in sizes) == {0, 1, 2, 3}
        keeps = [np.arange(n, dtype=np.int32), np.array([n // 2], dtype=np.int32), np.array([0], dtype=np.int32),
                 np.array([n - 1], dtype=np.int32)] + [random_keep(rng, n, m) for m in sizes]
        for keep in keeps:
            with full.subset(keep) as sub:
                assert sub.n == keep.size and sub.cols == keep.size
                assert np.array_equal(sub.gram(), want[np.ix_(keep, keep)]), keep
                t = sub.timings()
                assert t["subset_bytes"] == 8 * keep.size ** 2 and t["subset_seconds"] >= 0 and t["gram_i64_live"] == 0
                assert t["gram_variants"] == full.timings()["gram_variants"]
        assert np.array_equal(full.gram(), want)
        assert full.timings()["subset_bytes"] == 0          # counted on the engine the call returned


@pytest.mark.parametrize("m", [31, 33])
def test_subset_computes_on_either_side_of_the_dense_solver(P, m):
    """pops40 cut to 31 samples is solved by the dense Householder solver, to 33 by the Lanczos path (N >= 32): either way the
    eigenpairs are the oracle's for S[I, I] (smoke()'s bounds: eigenvalues 1e-6 relative, components 1e-6 in norm)."""
    oracle = load_oracle()
    g = load_golden("pops40")
    keep = random_keep(np.random.default_rng(m), 40, m)
    with P.PcoaEngine(40) as full:
        full.accumulate_calls(g["sample_idx"], g["row_offsets"])
        with full.subset(keep) as sub:
            comps, lam, nz = sub.compute(2)
            method = sub.timings()["eig_method"]
    ref = oracle.compute_pca(g["similarity"][np.ix_(keep, keep)], 2)
    assert method == 2 if m < 32 else method in (1, 2)
    assert nz == ref["nonzero_rows"] and np.allclose(lam, ref["eigenvalues"], rtol=1e-6)
    assert np.linalg.norm(align_sign(comps, ref["components"]) - ref["components"], axis=0).max() < 1e-6


# ---- 2. tile edges ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_cohort(P, ingest):
    rng = np.random.default_rng(2100)
    x, bits = random_bits(rng, ingest, 2100, 256)
    eng = P.PcoaEngine(2100)
    eng.accumulate_bits(bits)
    want = eng.gram()
    assert np.array_equal(want, int_gram(x))
    yield eng, want
    eng.close()


@pytest.mark.parametrize("m", [BAND_ROWS - 1, BAND_ROWS, BAND_ROWS + 1, TILE_COLS - 1, TILE_COLS, TILE_COLS + 1,
                               2 * TILE_COLS + 3, 2100])
def test_subset_at_the_edges_of_a_column_tile_and_a_row_band(edge_cohort, m):
    """m just below, at and just above one row band (32) and one column tile (1,024) of the gather kernel, beyond two tiles,
    and the identity: every entry is compared."""
    eng, want = edge_cohort
    keep = random_keep(np.random.default_rng(m), 2100, m)
    with eng.subset(keep) as sub:
        assert np.array_equal(sub.gram(), want[np.ix_(keep, keep)])


# ---- 3. the int64 part ----------------------------------------------------------------------------------------------------------
def test_subset_of_an_int64_gram(P, ingest):
    """An S whose entries among samples 10..13 lie beyond 2^31 keeps its int64 part through load_gram.  A subset that keeps one
    of them is exact and still int64; one that drops them all is exact and back in the int32 matrix (narrowed_to_int32
    advances on the subset).  With more variants accumulated on top (int32 partial beside the int64 total) both are summed."""
    n = 70
    rng = np.random.default_rng(64)
    s = rng.integers(0, 1 << 20, size=(n, n), dtype=np.int64)
    s[10:14, 10:14] = rng.integers(1 << 33, 1 << 40, size=(4, 4), dtype=np.int64)
    s = s + s.T
    big = np.arange(10, 14)
    with P.PcoaEngine(n) as full:
        full.load_gram(s)
        assert full.timings()["gram_i64_live"] == 1
        for extra in (0, 64):
            if extra:
                x, bits = random_bits(rng, ingest, n, extra)
                full.accumulate_bits(bits)
                s = s + int_gram(x)
            assert np.array_equal(full.gram(), s)
            with_big = np.sort(np.concatenate([random_keep(rng, 10, 5), [12], 14 + random_keep(rng, 56, 21)])).astype(np.int32)
            with full.subset(with_big) as sub:
                assert np.array_equal(sub.gram(), s[np.ix_(with_big, with_big)])
                t = sub.timings()
                assert t["gram_i64_live"] == 1 and t["narrowed_to_int32"] == 0
                assert t["subset_bytes"] == (8 + 16) * with_big.size ** 2
            without = np.setdiff1d(np.arange(n), big).astype(np.int32)
            with full.subset(without) as sub:
                assert np.array_equal(sub.gram(), s[np.ix_(without, without)])
                t = sub.timings()
                assert t["gram_i64_live"] == 0 and t["narrowed_to_int32"] == 1
                comps, lam, _ = sub.compute(2)
                assert np.all(np.isfinite(comps)) and np.all(np.isfinite(lam))
            assert np.array_equal(full.gram(), s) and full.timings()["gram_i64_live"] == 1


# ---- 4. the same answer as the reduced cohort ---------------------------------------------------------------------------------
def planted_bits(rng, n, v):
    """Four populations with their own carrier frequencies per variant: three clear leading eigenvalues at any n."""
    pop = np.sort(rng.integers(0, 4, size=n))
    f = rng.uniform(0.05, 0.5, (v, 4)).astype(np.float32)
    return rng.random((v, n), dtype=np.float32) < f[:, pop]


def same_answer(P, ingest, n, v, removed, num_pc, read_all):
    rng = np.random.default_rng(n)
    x = planted_bits(rng, n, v)
    keep = np.setdiff1d(np.arange(n), rng.choice(n, size=removed, replace=False)).astype(np.int32)
    with P.PcoaEngine(n) as full, P.PcoaEngine(keep.size) as fresh:
        full.accumulate_bits(ingest.pack_bits(x))
        fresh.accumulate_bits(ingest.pack_bits(x[:, keep]))
        with full.subset(keep) as sub:
            if read_all:
                assert np.array_equal(sub.gram(), fresh.gram())
            else:   # N^2 int64 entries are 2 GB a side: row bands of both, every entry still compared
                for r0 in range(0, keep.size, 2048):
                    rows = min(2048, keep.size - r0)
                    assert np.array_equal(sub.gram_block(r0, 0, rows, keep.size), fresh.gram_block(r0, 0, rows, keep.size)), r0
            got, want = sub.compute(num_pc), fresh.compute(num_pc)
            ts, tf = sub.timings(), fresh.timings()
    assert ts["gram_i64_live"] == 0 and tf["gram_i64_live"] == 0
    assert got[2] == want[2]
    assert np.array_equal(got[1], want[1]), (got[1], want[1])           # the same S, n and code path: the same bits
    assert np.array_equal(got[0], want[0])
    return ts, tf


def test_subset_computes_what_a_fresh_engine_over_the_kept_columns_computes(P, ingest):
    ts, tf = same_answer(P, ingest, 700, 4000, 37, 3, True)
    assert ts["eig_method"] == tf["eig_method"]


def test_subset_computes_the_same_bits_on_the_upper_triangle_forms(P, ingest):
    """N = 16,420 keeping 16,388: from 16,384 samples (N % 4 == 0, no int64 part) computePca reads only the upper triangle of
    S for its row sums and mat-vecs (matvec_form 1) -- a subset must be as symmetric as a fresh S to give the same bits."""
    ts, tf = same_answer(P, ingest, 16420, 512, 32, 3, False)
    assert ts["matvec_form"] == 1 and tf["matvec_form"] == 1


# ---- 5. 64-bit offsets ----------------------------------------------------------------------------------------------------------
def test_subset_past_two_to_the_31_entries(P, ingest):
    """N = 46,400 (N^2 = 2.15e9 > 2^31), 37 samples removed: the top-left block, the bottom-right block (dst and src offsets
    beyond 2^31) and a block across a removed index against the numpy Gram of the kept columns."""
    n, v = 46400, 256
    rng = np.random.default_rng(46400)
    x = rng.random((v, n), dtype=np.float32) < 0.3
    gone = np.sort(rng.choice(n, size=37, replace=False))
    gone[17] = 23211 if 23211 not in gone else gone[17]
    gone = np.unique(gone)
    keep = np.setdiff1d(np.arange(n), gone).astype(np.int32)
    m = keep.size
    assert (m - 1) * m > 2 ** 31 and int(keep[-1]) * n > 2 ** 31
    xk = x[:, keep].astype(np.float32)
    across = int(np.searchsorted(keep, 23211))                           # keep[across - 1] < 23211 < keep[across]
    assert keep[across] - keep[across - 1] >= 2
    with P.PcoaEngine(n) as full:
        full.accumulate_bits(ingest.pack_bits(x))
        with full.subset(keep) as sub:
            for r0, c0 in ((0, 0), (m - 64, m - 64), (across - 32, across - 32), (m - 64, 0), (across - 32, m - 64)):
                got = sub.gram_block(r0, c0, 64, 64)
                assert np.array_equal(got, int_gram_block(xk, r0, c0, 64)), (r0, c0)
            t = sub.timings()
            assert t["subset_bytes"] == 8 * m * m and t["subset_seconds"] > 0
        assert np.array_equal(full.gram_block(n - 64, n - 64, 64, 64), int_gram_block(x.astype(np.float32), n - 64, n - 64, 64))


def int_gram_block(x, r0, c0, w):
    a = np.asarray(x[:, r0:r0 + w], dtype=np.float64)
    b = np.asarray(x[:, c0:c0 + w], dtype=np.float64)
    return (a.T @ b).astype(np.int64)                                    # 0/1 entries, a few hundred rows: exact


# ---- 6. a subset is an engine -------------------------------------------------------------------------------------------------
def test_a_subset_is_an_engine(P, ingest):
    n = 300
    rng = np.random.default_rng(300)
    xa, bits_a = random_bits(rng, ingest, n, 256)
    xb, bits_b = random_bits(rng, ingest, n, 192, density=0.2)
    sa, sb = int_gram(xa), int_gram(xb)
    i1 = random_keep(rng, n, 257)
    i2 = random_keep(rng, 257, 130)
    with P.PcoaEngine(n) as a, P.PcoaEngine(n) as b:
        a.accumulate_bits(bits_a)
        b.accumulate_bits(bits_b)
        with a.subset(i1) as sub:
            # subset again: the composition of the two keep sets
            with sub.subset(i2) as sub2, a.subset(i1[i2]) as direct:
                assert np.array_equal(sub2.gram(), sa[np.ix_(i1[i2], i1[i2])])
                assert np.array_equal(sub2.gram(), direct.gram())
            # accumulate 128 more variants over the m samples
            xm, bits_m = random_bits(rng, ingest, 257, 128)
            sub.accumulate_bits(bits_m)
            assert np.array_equal(sub.gram(), sa[np.ix_(i1, i1)] + int_gram(xm))
            assert sub.timings()["gram_variants"] == a.timings()["gram_variants"] + 128
            b_rows, _, nz, _ = sub.center()
            assert nz == 257 and np.all(np.isfinite(b_rows))
        # reduce_from between two subsets of two engines = the subset of the sum
        with a.subset(i1) as sub_a, b.subset(i1) as sub_b:
            sub_a.reduce_from(sub_b)
            assert np.array_equal(sub_a.gram(), (sa + sb)[np.ix_(i1, i1)])
            assert np.array_equal(sub_b.gram(), sb[np.ix_(i1, i1)])
        # src reads back unchanged after all of this, and is still fed
        assert np.array_equal(a.gram(), sa) and np.array_equal(b.gram(), sb)
        a.reduce_from(b)
        with a.subset(i1) as sub:
            assert np.array_equal(sub.gram(), (sa + sb)[np.ix_(i1, i1)])


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------
def test_bad_keep_sets_are_invalid_arguments_and_leave_the_source_usable(P, L):
    g = load_golden("pops40")
    with P.PcoaEngine(40) as full:
        full.accumulate_calls(g["sample_idx"], g["row_offsets"])
        want = full.compute(2)
        for keep in ([3, 2, 5], [1, 4, 4, 9], [0, 1, 40], [-1, 3], [], [5, 6, 7, 6]):
            with pytest.raises(P.PcoaError) as ei:
                full.subset(keep)
            assert ei.value.code == L.PCOA_ERR_INVALID_ARG and "pcoa_create_subset" in str(ei.value), keep
            got = full.compute(2)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(full.gram(), g["similarity"])


def test_a_strip_owner_and_an_operator_cannot_be_subset(P, L, ingest):
    g = load_golden("pops40")
    E = load_pkg("engine")
    x = np.zeros((len(g["row_offsets"]) - 1, 40), dtype=np.float32)
    for v in range(x.shape[0]):
        x[v, g["sample_idx"][g["row_offsets"][v]:g["row_offsets"][v + 1]]] = 1
    bits = ingest.pack_bits(x)
    keep = np.arange(0, 40, 2, dtype=np.int32)
    with P.PcoaEngine(40, strip=(0, 40)) as owner:
        owner.accumulate_bits(bits)
        with pytest.raises(P.PcoaError) as ei:
            owner.subset(keep)
        assert ei.value.code == L.PCOA_ERR_STATE and "strip" in str(ei.value)
        comps, lam, nz = E.compute_strips([owner], 2)
        assert nz == 40 and np.all(np.isfinite(lam))
    with P.PcoaEngine(40, operator=True) as op:
        op.accumulate_bits(bits)
        with pytest.raises(P.PcoaError) as ei:
            op.subset(keep)
        assert ei.value.code == L.PCOA_ERR_STATE and "operator" in str(ei.value)
        comps, lam, nz = op.compute(2)
        assert nz == 40 and np.all(np.isfinite(lam))


# ---- 8. the hosts -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filesets(tmp_path_factory):
    """The planted cohort as a PLINK fileset, and -- under the same file name, so that the dataset column agrees -- the filesets
    with the samples deleted that the rounds of each sigma (and of one round at 1.8) remove."""
    d = tmp_path_factory.mktemp("outliers")
    x = C.planted_cohort()
    names = [C.name_of(i) for i in range(C.N)]
    out = {}
    cuts = dict(("all%.1f" % s, [i for r in rounds for i in r]) for s, rounds in C.EXPECTED.items())
    cuts["one1.8"] = C.EXPECTED[1.8][0]
    cuts["full"] = []
    for tag, gone in cuts.items():
        keep = [i for i in range(C.N) if i not in gone]
        prefix = str(d / tag / "cohort")
        C.write_plink(x[:, keep], prefix, [names[i] for i in keep])
        out[tag] = prefix + ".bed"
    return out


def rows_of(res):
    assert res.returncode == 0, res.stderr
    rows = [ln for ln in res.stdout.splitlines() if ln.count("\t") == 3]
    return rows


def rounds_of(res):
    got = []
    for ln in res.stderr.splitlines():
        if ln.startswith("Outlier round "):
            head, _, tail = ln.partition(" sample(s)")
            k, count = int(head.split()[2].rstrip(":")), int(head.split()[4])
            assert k == len(got) + 1
            removed = [int(nm[1:]) for nm in tail.lstrip(": ").split(", ")] if tail else []
            assert len(removed) == count
            got.append(removed)
    return got


_runs = {}


def run_once(host, path, extra=()):
    key = (host, path, tuple(extra))
    if key not in _runs:
        _runs[key] = (C.run_driver if host == "driver" else C.run_python)(["--input-path", path] + list(extra))
    return _runs[key]


@pytest.mark.parametrize("host", ["driver", "python"])
@pytest.mark.parametrize("sigma", sorted(C.EXPECTED))
def test_hosts_run_the_outlier_rounds(filesets, host, sigma):
    """--outlier-iterations 5: the names removed per round are the sets the oracle finds on the CPU, the rows are byte for byte
    those of the same host without the flags on the fileset with those samples deleted, and "Non zero rows" comes once."""
    res = run_once(host, filesets["full"], ("--outlier-iterations", "5", "--outlier-sigma", "%.1f" % sigma))
    rows = rows_of(res)
    assert rounds_of(res) == C.EXPECTED[sigma], res.stderr
    kept = C.N - sum(len(r) for r in C.EXPECTED[sigma])
    assert len(rows) == kept
    assert res.stdout.count("Non zero rows in matrix") == 1 and "Non zero rows in matrix: %d / %d." % (kept, kept) in res.stdout
    # the closing line still reports the Gram kernels' time, which ran on an engine the rounds have replaced
    closing = re.search(r"Variants accumulated: (\d+); Gram kernel ([0-9.]+) ms", res.stderr)
    assert closing and int(closing.group(1)) > 0 and float(closing.group(2)) > 0, res.stderr
    plain = run_once(host, filesets["all%.1f" % sigma])
    assert "Outlier round" not in plain.stderr
    assert "\n".join(rows).encode() == "\n".join(rows_of(plain)).encode()


@pytest.mark.parametrize("sigma", sorted(C.EXPECTED))
def test_both_hosts_emit_the_same_rows(filesets, sigma):
    extra = ("--outlier-iterations", "5", "--outlier-sigma", "%.1f" % sigma)
    assert rows_of(run_once("driver", filesets["full"], extra)) == rows_of(run_once("python", filesets["full"], extra))


def test_one_round_keeps_the_samples_of_the_later_rounds(filesets):
    res = run_once("driver", filesets["full"], ("--outlier-iterations", "1", "--outlier-sigma", "1.8"))
    rows = rows_of(res)
    assert rounds_of(res) == C.EXPECTED[1.8][:1]
    names = [r.split("\t")[0] for r in rows]
    assert C.name_of(9) in names and len(rows) == C.N - 3 and not set(names) & set(C.name_of(i) for i in C.EXPECTED[1.8][0])
    assert rows == rows_of(run_once("driver", filesets["one1.8"]))


def test_outlier_rounds_behind_a_two_engine_reduction(filesets):
    """--gpus 2 --gpu-map 0,0 --reduce peer: the rounds run on engine 0 after the full-layout reduction; the same rows."""
    extra = ("--outlier-iterations", "5", "--outlier-sigma", "1.8")
    res = run_once("driver", filesets["full"], extra + ("--gpus", "2", "--gpu-map", "0,0", "--reduce", "peer"))
    assert rounds_of(res) == C.EXPECTED[1.8]
    assert rows_of(res) == rows_of(run_once("driver", filesets["full"], extra))

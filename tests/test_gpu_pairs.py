"""GPU tests of the related-pairs screen (pcoa_similar_pairs, PcoaEngine.similar_pairs, --related-min-jaccard): the reference
is variants_pca.related_pairs_rule in numpy, applied to the very S the engine returns from gram(); every test compares the
WHOLE pair list (i, j, shared) and n_found -- on the goldens, at the kernel's tile and band edges, with an int64 part, at every
capacity, past 2^31 entries --, the screen is reproducible and leaves the engine as it was, errors leave it usable, and both
hosts screen and reduce the cohort of tests/related_cohort.py to the pairs the rule finds on the CPU (test_pairs_cpu.py)."""
import ctypes
import re

import numpy as np
import pytest

import related_cohort as R
from conftest import int_gram, load_golden, load_pkg

pytestmark = pytest.mark.gpu

# the scan kernels' workgroup shape (csrc/pcoa_internal.h: kPairsTileCols, kPairsBandRows): a workgroup takes 32 rows x 1,024
# columns, a lane four consecutive columns
TILE_COLS, BAND_ROWS = 1024, 32


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def L():
    return load_pkg("_lib")


@pytest.fixture(scope="module")
def vp():
    return load_pkg("variants_pca")


@pytest.fixture(scope="module")
def ingest():
    return load_pkg("ingest")


def random_bits(rng, ingest, n, v, density=0.3):
    x = (rng.random((v, n)) < density).astype(np.float32)
    return x, ingest.pack_bits(x)


def same_pairs(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def check_against_rule(eng, vp, s, x):
    """The whole list, n_found and diag of one screen against the numpy rule on s."""
    want = vp.related_pairs_rule(s, x)
    pairs, n_found, diag = eng.similar_pairs(x, capacity=max(1, s.shape[0] * (s.shape[0] - 1) // 2 + 3))
    assert n_found == want.size, (x, n_found, want.size)
    assert same_pairs(pairs, want), x
    assert np.array_equal(diag, np.diagonal(s))
    return want


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged16", "pops40", "tile130", "tile260"])
def test_pairs_of_the_goldens_are_the_rule_s(P, vp, name):
    g = load_golden(name)
    n = int(g["n_samples"])
    with P.PcoaEngine(n) as eng:
        eng.accumulate_calls(g["sample_idx"], g["row_offsets"])
        s = eng.gram()
        assert np.array_equal(s, g["similarity"])
        for x in (1.0, 0.5, 0.25, 1e-9):
            want = check_against_rule(eng, vp, s, x)
            if x == 1e-9:   # the dense case: every pair that shares a variant
                assert want.size == int(np.count_nonzero(np.triu(s, 1))) > 0
        assert np.array_equal(eng.gram(), s)


# ---- 2. tile and band edges ---------------------------------------------------------------------------------------------------
def edge_matrix(n):
    """(S, the pairs that hit at X = 0.5): a symmetric background that never hits (diagonals 1,000..2,000, off-diagonals
    0..50: J < 0.06), planted entries S = (d_i + d_j) // 3 + 1 (3 S > d_i + d_j, so S >= U / 2) at the corners of the matrix, at
    the first column-tile edge and on both sides of every row-band edge, and samples 10, 11, 12 with d = 30: S(10, 11) = 20 sits
    ON the threshold (U = 40) and is reported, S(10, 12) = 19 (U = 41) is not."""
    rng = np.random.default_rng(n)
    a = rng.integers(0, 51, size=(n, n), dtype=np.int64)
    s = np.triu(a, 1)
    s = s + s.T
    d = rng.integers(1000, 2001, size=n, dtype=np.int64)
    planted = set()
    if n >= 2:
        planted |= {(0, 1), (0, n - 1), (n - 2, n - 1)}
    for i, j in ((TILE_COLS - 1, TILE_COLS), (TILE_COLS, TILE_COLS + 1)):
        if j < n:
            planted.add((i, j))
    for edge in range(BAND_ROWS, n, BAND_ROWS):
        for i, j in ((edge - 1, min(edge + 7, n - 1)), (edge, min(edge + 9, n - 1))):
            if i < j:
                planted.add((i, j))
    if n >= 31:
        d[10:13] = 30
        planted.add((10, 11))
    np.fill_diagonal(s, d)
    for i, j in planted:
        s[i, j] = s[j, i] = (d[i] + d[j]) // 3 + 1
    if n >= 31:
        s[10, 11] = s[11, 10] = 20
        s[10, 12] = s[12, 10] = 19
        s[11, 12] = s[12, 11] = 3
    return s, sorted(planted)


EDGE_SIZES = [1, 2, 31, 33, 1023, 1024, 1025, 1026, 2051, 2100]   # (1,026: a row pitch of 2 mod 4 over more than one tile)


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_pairs_at_the_edges_of_a_column_tile_and_a_row_band(P, vp, n):
    s, planted = edge_matrix(n)
    want = vp.related_pairs_rule(s, 0.5)
    assert [(int(p["i"]), int(p["j"])) for p in want] == planted          # the fixture plants what it says, nothing else hits
    if n >= 31:
        assert (10, 11) in planted and (10, 12) not in planted
    with P.PcoaEngine(n) as eng:
        eng.load_gram(s)
        assert np.array_equal(eng.gram(), s)
        check_against_rule(eng, vp, s, 0.5)
        if n == 1:
            pairs, n_found, diag = eng.similar_pairs(1e-9)
            assert n_found == 0 and pairs.size == 0 and list(diag) == [int(s[0, 0])]


def test_the_edge_sizes_cover_every_row_pitch():
    assert set(n % 4 for n in EDGE_SIZES if n > TILE_COLS) == {0, 1, 2, 3}


# ---- 3. the int64 part ----------------------------------------------------------------------------------------------------------
def test_pairs_of_an_int64_gram(P, vp, ingest):
    """An S whose entries among samples 10..13 lie beyond 2^33 keeps its int64 part through load_gram; with more variants
    accumulated on top an int32 partial sits beside the int64 total.  Pairs and diag are those of the summed matrix."""
    n = 70
    rng = np.random.default_rng(64)
    s = rng.integers(0, 1 << 20, size=(n, n), dtype=np.int64)
    s[10:14, 10:14] = rng.integers(1 << 33, 1 << 40, size=(4, 4), dtype=np.int64)
    s = s + s.T
    with P.PcoaEngine(n) as eng:
        eng.load_gram(s)
        assert eng.timings()["gram_i64_live"] == 1
        for extra in (0, 64):
            if extra:
                x, bits = random_bits(rng, ingest, n, extra)
                eng.accumulate_bits(bits)
                s = s + int_gram(x)
            assert np.array_equal(eng.gram(), s) and eng.timings()["gram_i64_live"] == 1
            wants = [check_against_rule(eng, vp, s, x) for x in (0.5, 0.25, 1e-9)]
            assert 0 < wants[0].size < wants[1].size < wants[2].size
            assert all((w["shared"] > 2 ** 33).any() for w in wants)       # entries that only the int64 part holds are reported
            assert np.array_equal(eng.gram(), s)


# ---- 4. capacity ----------------------------------------------------------------------------------------------------------------
def test_pairs_at_every_capacity(P, L, vp, ingest):
    n = 300
    rng = np.random.default_rng(300)
    x, bits = random_bits(rng, ingest, n, 256)
    sentinel = np.array([(-7, -7, -7)], dtype=vp.PAIR_DTYPE)[0]
    with P.PcoaEngine(n) as eng:
        eng.accumulate_bits(bits)
        s = eng.gram()
        full = vp.related_pairs_rule(s, 1e-9)
        assert 40000 < full.size <= 44850
        for cap in (0, 1, 63, 64, 65, full.size - 1, full.size, full.size + 7):
            buf = np.full(cap + 16, sentinel, dtype=vp.PAIR_DTYPE)
            found = ctypes.c_int64(-1)
            rc = eng._lib.pcoa_similar_pairs(eng._ctx, 1e-9, ctypes.c_void_p(buf.ctypes.data), cap, ctypes.byref(found), None)
            assert rc == L.PCOA_OK and found.value == full.size, (cap, rc, found.value)
            k = min(full.size, cap)
            assert same_pairs(buf[:k], full[:k]), cap
            assert np.all(buf[k:] == sentinel), cap
        pairs, n_found, _ = eng.similar_pairs(1e-9, capacity=100)          # the binding hands back the written prefix
        assert n_found == full.size and same_pairs(pairs, full[:100])
        pairs, n_found, _ = eng.similar_pairs(1e-9, capacity=0)
        assert n_found == full.size and pairs.size == 0


# ---- 5. past 2^31 entries -------------------------------------------------------------------------------------------------------
def test_pairs_past_two_to_the_31_entries(P, vp, ingest):
    """N = 46,400 (N^2 = 2.15e9 > 2^31) with 256 random variants; samples 46,399 and 46,390 are copies of samples 3 and 46,380.
    At X = 0.9 exactly those two pairs are reported (row 46,380 starts beyond 2^31 entries).  Numpy checks it from the rows of
    the four samples involved plus 200,000 random other pairs."""
    n, v = 46400, 256
    rng = np.random.default_rng(46400)
    x = rng.random((v, n), dtype=np.float32) < 0.3
    x[:, 46399] = x[:, 3]
    x[:, 46390] = x[:, 46380]
    assert 46380 * n > 2 ** 31
    d = x.sum(axis=0).astype(np.int64)
    xf = x.astype(np.float32)
    expect = [(3, 46399, int(d[3])), (46380, 46390, int(d[46380]))]
    # the rows of the samples involved, against every column
    for a in (3, 46399, 46380, 46390):
        shared = (xf[:, a] @ xf).astype(np.int64)
        u = d[a] + d - shared
        hit = np.nonzero((u > 0) & (shared.astype(np.float64) >= 0.9 * u.astype(np.float64)))[0]
        partner = {3: 46399, 46399: 3, 46380: 46390, 46390: 46380}[a]
        assert sorted(hit) == sorted([a, partner]), a
    # a random sample of other pairs: none comes near
    xt = np.ascontiguousarray(x.T)
    i, j = rng.integers(0, n, size=200000), rng.integers(0, n, size=200000)
    ok = (i != j) & ~np.isin(i, (3, 46399, 46380, 46390))
    i, j = i[ok], j[ok]
    shared = np.count_nonzero(xt[i] & xt[j], axis=1).astype(np.int64)
    u = d[i] + d[j] - shared
    assert not np.any(shared.astype(np.float64) >= 0.9 * u.astype(np.float64))
    with P.PcoaEngine(n) as eng:
        eng.accumulate_bits(ingest.pack_bits(x))
        pairs, n_found, diag = eng.similar_pairs(0.9, capacity=64)
        t = eng.timings()
    assert n_found == 2 and [(int(p["i"]), int(p["j"]), int(p["shared"])) for p in pairs] == expect
    assert np.array_equal(diag, d)
    assert t["pairs_bytes"] >= 4 * (n * (n - 1) // 2) and t["pairs_seconds"] > 0


# ---- 6. reproducible and side-effect free ---------------------------------------------------------------------------------------
def test_the_screen_is_reproducible_and_leaves_the_engine_as_it_was(P, vp):
    x = R.related_cohort(260, 2000)
    callsets = [list(np.nonzero(r)[0]) for r in x]
    with P.PcoaEngine(260) as one, P.PcoaEngine(260) as seven:
        one.accumulate_callsets(callsets)
        cuts = np.linspace(0, len(callsets), 8).astype(int)
        for a, b in zip(cuts[:-1], cuts[1:]):
            seven.accumulate_callsets(callsets[a:b])
        before = one.compute(2)
        assert one.timings()["pairs_bytes"] == 0 and one.timings()["pairs_calls"] == 0
        first = one.similar_pairs(0.25)
        second = one.similar_pairs(0.25)
        other = seven.similar_pairs(0.25)
        assert first[1] == second[1] == other[1] and first[1] > 6
        assert first[0].tobytes() == second[0].tobytes() == other[0].tobytes()
        assert first[2].tobytes() == second[2].tobytes() == other[2].tobytes()
        assert same_pairs(first[0], vp.related_pairs_rule(one.gram(), 0.25))
        after = one.compute(2)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before[:2], after[:2])) and before[2] == after[2]
        t = one.timings()
        assert t["pairs_bytes"] > 0 and t["pairs_seconds"] >= 0 and t["pairs_calls"] == 2
        # the count pass reads the blocks above the diagonal once per call; the write pass only the cells with a hit
        assert t["pairs_bytes"] >= 2 * 4 * (260 * 259 // 2) and t["pairs_bytes"] <= 2 * 2 * 4 * 260 * 260


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def test_a_strip_owner_and_an_operator_cannot_be_screened(P, L, ingest):
    g = load_golden("pops40")
    E = load_pkg("engine")
    x = np.zeros((len(g["row_offsets"]) - 1, 40), dtype=np.float32)
    for v in range(x.shape[0]):
        x[v, g["sample_idx"][g["row_offsets"][v]:g["row_offsets"][v + 1]]] = 1
    bits = ingest.pack_bits(x)
    with P.PcoaEngine(40, strip=(0, 40)) as owner:
        owner.accumulate_bits(bits)
        with pytest.raises(P.PcoaError) as ei:
            owner.similar_pairs(0.5)
        assert ei.value.code == L.PCOA_ERR_STATE and "strip" in str(ei.value) and "pcoa_similar_pairs" in str(ei.value)
        comps, lam, nz = E.compute_strips([owner], 2)
        assert nz == 40 and np.all(np.isfinite(lam))
    with P.PcoaEngine(40, operator=True) as op:
        op.accumulate_bits(bits)
        with pytest.raises(P.PcoaError) as ei:
            op.similar_pairs(0.5)
        assert ei.value.code == L.PCOA_ERR_STATE and "operator" in str(ei.value) and "pcoa_similar_pairs" in str(ei.value)
        comps, lam, nz = op.compute(2)
        assert nz == 40 and np.all(np.isfinite(lam))


def test_bad_arguments_are_invalid_and_leave_the_engine_usable(P, L, vp):
    g = load_golden("pops40")
    with P.PcoaEngine(40) as eng:
        eng.accumulate_calls(g["sample_idx"], g["row_offsets"])
        want = eng.compute(2)
        ref = vp.related_pairs_rule(g["similarity"], 0.25)
        buf = np.zeros(1024, dtype=vp.PAIR_DTYPE)
        out, found = ctypes.c_void_p(buf.ctypes.data), ctypes.c_int64(-3)
        call = eng._lib.pcoa_similar_pairs
        bad = [(float("nan"), out, 1024, ctypes.byref(found)), (0.0, out, 1024, ctypes.byref(found)),
               (-0.5, out, 1024, ctypes.byref(found)), (1.5, out, 1024, ctypes.byref(found)),
               (float("inf"), out, 1024, ctypes.byref(found)), (0.5, out, -1, ctypes.byref(found)), (0.5, out, 1024, None),
               (0.5, None, 1024, ctypes.byref(found))]
        for x, o, cap, f in bad:
            assert call(eng._ctx, x, o, cap, f, None) == L.PCOA_ERR_INVALID_ARG, (x, cap)
            assert b"pcoa_similar_pairs" in eng._lib.pcoa_last_error(eng._ctx)
            assert found.value == -3 and not buf.view(np.uint8).any()
            pairs, n_found, _ = eng.similar_pairs(0.25)
            assert n_found == ref.size and same_pairs(pairs, ref)
        with pytest.raises(P.PcoaError) as ei:
            eng.similar_pairs(0.5, capacity=-4)
        assert ei.value.code == L.PCOA_ERR_INVALID_ARG
        got = eng.compute(2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(eng.gram(), g["similarity"])


# ---- 8. the hosts ---------------------------------------------------------------------------------------------------------------
X = "%.2f" % R.THRESHOLD
ON = ("--related-min-jaccard", X)


@pytest.fixture(scope="module")
def cohort(tmp_path_factory, vp):
    """The n = 260 cohort as a PLINK fileset and as a VCF, the fileset with the samples of related_removal deleted (under the
    same file name, so that the dataset column agrees), and what the rule says about it."""
    d = tmp_path_factory.mktemp("related")
    n = R.HOST_N
    x = R.related_cohort(n, R.HOST_V)
    R.margins(x)                                                          # a fixture that does not discriminate fails here
    names = [R.name_of(i) for i in range(n)]
    s = int_gram(x.astype(np.float32))
    pairs = vp.related_pairs_rule(s, R.THRESHOLD)
    gone = [int(i) for i in vp.related_removal(pairs, n)]
    keep = [i for i in range(n) if i not in gone]
    R.write_plink(x, str(d / "full" / "cohort"), names)
    R.write_plink(x[:, keep], str(d / "cut" / "cohort"), [names[i] for i in keep])
    R.write_vcf(x, str(d / "cohort.vcf"), names)
    lines = ["name_i\tname_j\tshared\td_i\td_j\tjaccard"]
    for p in pairs:
        i, j, sh = int(p["i"]), int(p["j"]), int(p["shared"])
        lines.append("%s\t%s\t%d\t%d\t%d\t%s" % (names[i], names[j], sh, s[i, i], s[j, j],
                                                 vp.java_double_to_string(sh / float(s[i, i] + s[j, j] - sh))))
    line = "Related pairs: %d at jaccard >= %s; removed %%d sample(s)%%s" % (pairs.size, vp.java_double_to_string(R.THRESHOLD))
    return {"full": str(d / "full" / "cohort.bed"), "cut": str(d / "cut" / "cohort.bed"), "vcf": str(d / "cohort.vcf"),
            "dir": d, "pairs": pairs, "gone": gone, "file": "\n".join(lines) + "\n",
            "reported": line % (0, ""), "removed": line % (len(gone), ": " + ", ".join(names[i] for i in gone))}


def rows_of(res):
    assert res.returncode == 0, res.stderr
    return [ln for ln in res.stdout.splitlines() if ln.count("\t") == 3]


def related_line(res):
    lines = [ln for ln in res.stderr.splitlines() if ln.startswith("Related pairs:")]
    assert len(lines) == 1, res.stderr
    return lines[0]


_runs = {}


def run_once(host, path, extra=()):
    key = (host, path, tuple(extra))
    if key not in _runs:
        _runs[key] = (R.run_driver if host == "driver" else R.run_python)(["--input-path", path] + list(extra))
    return _runs[key]


def test_the_planted_pairs_are_what_the_rule_reports(cohort):
    assert [(int(p["i"]), int(p["j"])) for p in cohort["pairs"]] == R.planted_pairs(R.HOST_N)
    assert cohort["gone"] == sorted(b for _, b in R.planted_pairs(R.HOST_N))


@pytest.mark.parametrize("host", ["driver", "python"])
def test_hosts_report_the_pairs(cohort, host):
    """Without --remove-related the screen only reports: the stderr line, the pair file, and the rows of a run without the
    flags."""
    out = str(cohort["dir"] / ("pairs-%s.tsv" % host))
    res = run_once(host, cohort["full"], ON + ("--related-output-path", out))
    rows = rows_of(res)
    assert related_line(res) == cohort["reported"]
    assert open(out).read() == cohort["file"]
    assert res.stdout.count("Non zero rows in matrix") == 1
    assert rows == rows_of(run_once(host, cohort["full"])) and len(rows) == R.HOST_N


def test_both_hosts_write_the_same_bytes(cohort):
    files = []
    for host in ("driver", "python"):
        run_once(host, cohort["full"], ON + ("--related-output-path", str(cohort["dir"] / ("pairs-%s.tsv" % host))))
        files.append(open(str(cohort["dir"] / ("pairs-%s.tsv" % host)), "rb").read())
    assert files[0] == files[1] == cohort["file"].encode()
    # the same cohort as a VCF: the same line and the same pairs (the names are the VCF's columns)
    out = str(cohort["dir"] / "pairs-vcf.tsv")
    res = run_once("driver", cohort["vcf"], ON + ("--related-output-path", out))
    assert res.returncode == 0, res.stderr
    assert related_line(res) == cohort["reported"] and open(out).read() == cohort["file"]


@pytest.mark.parametrize("host", ["driver", "python"])
def test_hosts_remove_the_related_samples(cohort, host):
    """--remove-related: the rows are byte for byte those of the same host, without the flags, on the fileset with the samples
    of related_removal deleted; "Non zero rows" comes once, for the final cohort."""
    res = run_once(host, cohort["full"], ON + ("--remove-related",))
    rows = rows_of(res)
    kept = R.HOST_N - len(cohort["gone"])
    assert related_line(res) == cohort["removed"]
    assert len(rows) == kept
    assert res.stdout.count("Non zero rows in matrix") == 1 and "Non zero rows in matrix: %d / %d." % (kept, kept) in res.stdout
    closing = re.search(r"Variants accumulated: (\d+); Gram kernel ([0-9.]+) ms", res.stderr)
    assert closing and int(closing.group(1)) > 0 and float(closing.group(2)) > 0, res.stderr
    plain = run_once(host, cohort["cut"])
    assert "Related pairs" not in plain.stderr
    assert "\n".join(rows).encode() == "\n".join(rows_of(plain)).encode()


def test_both_hosts_emit_the_same_rows_and_line(cohort):
    a = run_once("driver", cohort["full"], ON + ("--remove-related",))
    b = run_once("python", cohort["full"], ON + ("--remove-related",))
    assert rows_of(a) == rows_of(b) and related_line(a) == related_line(b)


@pytest.mark.parametrize("host", ["driver", "python"])
def test_more_pairs_than_the_job_takes_stop_it(cohort, host):
    res = run_once(host, cohort["full"], ON + ("--related-max-pairs", "2"))
    assert res.returncode != 0
    assert "%d pairs" % cohort["pairs"].size in res.stderr and "--related-max-pairs" in res.stderr
    assert "--related-min-jaccard" in res.stderr and not rows_of_or_none(res)


def rows_of_or_none(res):
    return [ln for ln in res.stdout.splitlines() if ln.count("\t") == 3]


def test_the_screen_behind_a_two_engine_reduction(cohort):
    """--gpus 2 --gpu-map 0,0 --reduce peer: the screen runs on engine 0 after the full-layout reduction; the same rows."""
    extra = ON + ("--remove-related",)
    res = run_once("driver", cohort["full"], extra + ("--gpus", "2", "--gpu-map", "0,0", "--reduce", "peer"))
    assert related_line(res) == cohort["removed"]
    assert rows_of(res) == rows_of(run_once("driver", cohort["full"], extra))


@pytest.mark.parametrize("host", ["driver", "python"])
def test_the_screen_goes_before_the_outlier_rounds(cohort, host):
    res = run_once(host, cohort["full"], ON + ("--remove-related", "--outlier-iterations", "2"))
    rows = rows_of(res)
    assert related_line(res) == cohort["removed"]
    assert res.stdout.count("Non zero rows in matrix") == 1
    lines = res.stderr.splitlines()
    first_round = [k for k, ln in enumerate(lines) if ln.startswith("Outlier round 1:")]
    assert first_round and first_round[0] > lines.index(related_line(res))          # the screen first, then the rounds
    names = [r.split("\t")[0] for r in rows]
    assert not set(names) & set(R.name_of(i) for i in cohort["gone"]) and len(rows) <= R.HOST_N - len(cohort["gone"])
    assert names == sorted(names)

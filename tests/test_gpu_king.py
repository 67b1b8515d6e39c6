"""GPU tests of the KING-robust kinship screen (pcoa_accumulate_plink_bed_king, pcoa_king_pairs, --king-cutoff).  The reference is
numpy throughout: variants_pca.king_planes / king_counts / king_pairs_rule (test_king_cpu.py holds them to a triple loop over
genotype codes).  Every comparison is exact -- each plane's S against the numpy Gram of the plane, the WHOLE pair list with its
three counts, n_found, V and the het counts against the rule -- except the hosts' components after --king-remove, which are held
to a run on the fileset written without the removed samples within the suite's 1e-6 eigenpair tolerance."""
import ctypes
import os
from contextlib import ExitStack

import numpy as np
import pytest

import king_cohort as K
from conftest import load_pkg

pytestmark = pytest.mark.gpu

PCOA_ERR_INVALID_ARG, PCOA_ERR_STATE = -1, -8
CUTOFFS = (0.0442, 0.177, 0.354)          # third, first and duplicate / twin degree


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def L():
    return load_pkg("_lib")


@pytest.fixture(scope="module")
def vp():
    return load_pkg("variants_pca")


def five(P, stack, n, **kw):
    return [stack.enter_context(P.PcoaEngine(n, **kw)) for _ in range(5)]


def random_codes(n, v, seed, missing=0.1):
    """uint8 [v][n] of .bed codes: Hardy-Weinberg genotypes at a per-variant frequency, then missing calls."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, size=(v, 1))
    code = K.CODE_OF_DOSAGE[(rng.random((v, n)) < p).astype(np.int64) + (rng.random((v, n)) < p)]
    code[rng.random((v, n)) < missing] = 1
    return code


def grams_of(vp, code):
    return [K.gram(p) for p in vp.king_planes(code)]


def same_pairs(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def check_against_rule(P, vp, planes, grams, x):
    """The whole list, n_found, V and the het counts of one screen against the numpy rule on the five matrices."""
    want = vp.king_pairs_rule(grams, x)
    v, h, _, _, _ = vp.king_counts(grams)
    pairs, n_found, got_v, het = P.PcoaEngine.king_pairs(planes, x, capacity=want.size + 3)
    assert n_found == want.size, (x, n_found, want.size)
    assert same_pairs(pairs, want), x
    assert got_v == v and np.array_equal(het, h)
    return want


# ------------------------------------------------------------------------------------------------------- 1. decode + accumulate
CALL_ROWS = 37


@pytest.mark.parametrize("v", [1, 131, 1000])
@pytest.mark.parametrize("n", [5, 63, 65, 260])
def test_king_decode_and_accumulate(P, vp, n, v):
    import torch
    code = random_codes(n, v, seed=1000 * n + v, missing=0.15)
    rows = K.bed_rows(code)
    want = grams_of(vp, code)
    nb = rows.shape[1]
    with ExitStack() as stack:
        planes = five(P, stack, n)

        def check(what):
            for name, eng, g in zip(vp.KING_PLANES, planes, want):
                s = eng.gram()
                assert np.array_equal(s, g), "N = %d, V = %d, %s: plane %s differs from its numpy Gram in %d entries" % (
                    n, v, what, name, int((s != g).sum()))
                eng.reset()

        P.PcoaEngine.accumulate_plink_bed_king(planes, rows)
        check("host rows")
        wide = np.random.default_rng(n + v).integers(0, 256, size=(v, nb + 5), dtype=np.uint8)   # what lies behind a row is not its own
        wide[:, :nb] = rows
        dev = torch.from_numpy(wide).cuda()
        P.PcoaEngine.accumulate_plink_bed_king(planes, dev[:, :nb])
        check("device rows, row_bytes = %d" % (nb + 5))
        pinned = torch.from_numpy(rows).pin_memory()
        P.PcoaEngine.accumulate_plink_bed_king(planes, pinned, asynchronous=True)
        check("pinned queued rows")
        for v0 in range(0, v, CALL_ROWS):
            P.PcoaEngine.accumulate_plink_bed_king(planes, rows[v0:v0 + CALL_ROWS])
        check("calls of %d rows" % CALL_ROWS)
        del pinned, dev


# ------------------------------------------------------------------------------------------------------- 2. the screen on loaded matrices
_loaded = {}


def loaded_case(vp, n):
    """The five Grams of random codes over 48 variants -- few enough that chance alone puts pairs above the lowest cutoff --
    with duplicates in the first and the last two columns and a sample that shares half its genotypes with another, so that
    every cutoff reports pairs, the last row band and column tile included."""
    if n not in _loaded:
        code = random_codes(n, 48, seed=n)
        code[:, 1] = code[:, 0]
        code[:, n - 1] = code[:, n - 2]
        code[:24, 3] = code[:24, 2]
        _loaded[n] = grams_of(vp, code)
    return _loaded[n]


@pytest.mark.parametrize("n", [6, 63, 260, 1025, 2052])
def test_screen_of_loaded_matrices_is_the_rule_s(P, vp, n):
    """Both load paths (N % 4 == 0 or not), one to three column tiles of 1,024, one to 65 row bands of 32."""
    grams = loaded_case(vp, n)
    with ExitStack() as stack:
        planes = five(P, stack, n)
        for eng, g in zip(planes, grams):
            eng.load_gram(g)
        sizes = [check_against_rule(P, vp, planes, grams, x).size for x in CUTOFFS]
        assert sizes[0] >= sizes[1] >= sizes[2] >= 2                      # the two duplicates at least
        if n >= 63:
            assert sizes[0] > sizes[1]
        for eng, g in zip(planes, grams):                                # the matrices are unchanged
            assert np.array_equal(eng.gram(), g)


# ------------------------------------------------------------------------------------------------------- 3. capacity
def test_capacity(P, vp):
    n = 260
    grams = loaded_case(vp, n)
    want = vp.king_pairs_rule(grams, 0.0442)
    assert want.size > 20
    with ExitStack() as stack:
        planes = five(P, stack, n)
        for eng, g in zip(planes, grams):
            eng.load_gram(g)
        pairs, n_found, v, het = P.PcoaEngine.king_pairs(planes, 0.0442, capacity=0)           # count only
        assert pairs.size == 0 and n_found == want.size and v == 48
        lib, first, arr = P.PcoaEngine._king_planes(planes)
        cap = want.size // 2
        buf = np.zeros(want.size + 4, dtype=P.PcoaEngine.KING_PAIR_DTYPE)
        buf["i"] = -7                                                                           # a prefix, the rest untouched
        found = ctypes.c_int64(0)
        assert lib.pcoa_king_pairs(arr, 0.0442, ctypes.c_void_p(buf.ctypes.data), cap, ctypes.byref(found), None, None) == 0
        assert found.value == want.size and same_pairs(buf[:cap], want[:cap]) and (buf["i"][cap:] == -7).all()
        pairs, n_found, _, _ = P.PcoaEngine.king_pairs(planes, 0.0442, capacity=n * n)          # more than there are pairs
        assert n_found == want.size and same_pairs(pairs, want)


# ------------------------------------------------------------------------------------------------------- 4. the threshold
def test_the_threshold_on_the_device(P, vp):
    """num / het_sum = (12 - 4) / 32 = 0.25 exactly (test_king_cpu.threshold_codes): reported at 0.25, not one ulp above."""
    code = np.zeros((40, 3), dtype=np.uint8)
    code[:12, 0] = 2; code[:12, 1] = 2
    code[12:16, 0] = 2; code[12:16, 1] = 3
    code[16:20, 0] = 0; code[16:20, 1] = 2
    code[20:22, 0] = 0; code[20:22, 1] = 3
    code[22:, 0] = 3; code[22:, 1] = 3
    grams = grams_of(vp, code)
    with ExitStack() as stack:
        planes = five(P, stack, 3)
        P.PcoaEngine.accumulate_plink_bed_king(planes, K.bed_rows(code))
        at = check_against_rule(P, vp, planes, grams, 0.25)
        assert [tuple(int(t) for t in p) for p in at.tolist()] == [(0, 1, 12, 2, 32)]
        assert check_against_rule(P, vp, planes, grams, float(np.nextafter(0.25, 1.0))).size == 0


# ------------------------------------------------------------------------------------------------------- 5. the cohort end to end
@pytest.mark.parametrize("n,v", K.SIZES[:2])
def test_the_cohort_end_to_end(P, vp, n, v):
    code = K.codes(n, v)
    grams = grams_of(vp, code)
    with ExitStack() as stack:
        planes = five(P, stack, n)
        P.PcoaEngine.accumulate_plink_bed_king(planes, K.bed_rows(code))
        want = check_against_rule(P, vp, planes, grams, K.CUTOFF)
        assert [(int(p["i"]), int(p["j"])) for p in want] == K.planted_pairs(n)
        kin = vp.king_kinship(want)
        assert kin.min() >= K.CUTOFF * (1 + K.MIN_MARGIN) and round(float(kin.min()), 3) == K.KNOWN[n][0]


# ------------------------------------------------------------------------------------------------------- 6. inconsistent planes
def test_planes_fed_different_rows_are_invalid(P, vp):
    n, v = 65, 200
    code = random_codes(n, v, seed=9)
    ingest = load_pkg("ingest")
    bits = [ingest.pack_bits(p) for p in vp.king_planes(code)]
    with ExitStack() as stack:
        planes = five(P, stack, n)
        for k, (eng, b) in enumerate(zip(planes, bits)):
            eng.accumulate_bits(b[:-1] if k == 3 else b)                  # R is fed one row fewer
        with pytest.raises(P.PcoaError) as err:
            P.PcoaEngine.king_pairs(planes, K.CUTOFF)
        assert err.value.code == PCOA_ERR_INVALID_ARG and "not fed the same rows" in str(err.value) and "V = r_i + a_i + hm_i" in str(err.value)
        with pytest.raises(ValueError, match="V = r_i"):
            vp.king_counts([e.gram() for e in planes])
        planes[3].accumulate_bits(bits[3][-1:])                           # the planes stay usable: the missing row, and the screen serves
        grams = grams_of(vp, code)
        check_against_rule(P, vp, planes, grams, K.CUTOFF)
        swapped = [planes[0], planes[3], planes[2], planes[1], planes[4]]   # R where M belongs and M where R belongs
        with pytest.raises(P.PcoaError) as err:
            P.PcoaEngine.king_pairs(swapped, K.CUTOFF)
        assert err.value.code == PCOA_ERR_INVALID_ARG and "not fed the same rows" in str(err.value)
        with pytest.raises(ValueError, match="not fed the same rows"):
            vp.king_counts([grams[0], grams[3], grams[2], grams[1], grams[4]])
        swapped = [planes[0], planes[4], planes[2], planes[3], planes[1]]   # likewise A and M
        with pytest.raises(P.PcoaError) as err:
            P.PcoaEngine.king_pairs(swapped, K.CUTOFF)
        assert err.value.code == PCOA_ERR_INVALID_ARG and "not fed the same rows" in str(err.value)
        check_against_rule(P, vp, planes, grams, K.CUTOFF)               # and after an error the right order serves again


@pytest.mark.parametrize("plane,names", [(3, "ibs0 < 0"), (2, "het_sum < 0"), (1, "s_hm < 0")])
def test_each_pairwise_check_is_named(P, vp, plane, names):
    """V is constant (the diagonals are untouched) and one off-diagonal entry of one matrix, in the last row band and column
    tile, is too large: G_R makes an ibs0 negative, G_HM a het_sum, G_M an s_hm -- and only that one."""
    n = 1025
    grams = [g.copy() for g in loaded_case(vp, n)]
    grams[plane][1000, 1024] += 1000
    grams[plane][1024, 1000] += 1000
    with pytest.raises(ValueError, match=names):
        vp.king_counts(grams)
    with ExitStack() as stack:
        planes = five(P, stack, n)
        for eng, g in zip(planes, grams):
            eng.load_gram(g)
        with pytest.raises(P.PcoaError) as err:
            P.PcoaEngine.king_pairs(planes, K.CUTOFF)
        assert err.value.code == PCOA_ERR_INVALID_ARG and names in str(err.value), str(err.value)
        for eng, g in zip(planes, grams):                                # nothing was changed by the refusal
            assert np.array_equal(eng.gram(), g)


def test_an_int64_plane_is_not_built(P, vp):
    n = 65
    grams = grams_of(vp, random_codes(n, 100, seed=4))
    with ExitStack() as stack:
        planes = five(P, stack, n)
        for k, (eng, g) in enumerate(zip(planes, grams)):
            eng.load_gram(g * (1 << 30) if k == 4 else g)                 # counts of tens: 2^30 times that leaves int32
        assert planes[4].timings()["gram_i64_live"] == 1
        with pytest.raises(P.PcoaError) as err:
            P.PcoaEngine.king_pairs(planes, K.CUTOFF)
        assert err.value.code == PCOA_ERR_STATE and "int64 part" in str(err.value) and "PCOA_KING_HOM_A2" in str(err.value)
        planes[4].load_gram(grams[4])                                     # usable afterwards
        check_against_rule(P, vp, planes, grams, K.CUTOFF)


# ------------------------------------------------------------------------------------------------------- 7. argument refusals
def test_every_argument_refusal(P, L, vp):
    n = 12
    code = random_codes(n, 30, seed=2)
    rows = K.bed_rows(code)
    grams = grams_of(vp, code)
    lib = L.load()
    king = P.PcoaEngine
    with ExitStack() as stack:
        planes = five(P, stack, n)
        other_n = stack.enter_context(P.PcoaEngine(n + 1))
        strip = stack.enter_context(P.PcoaEngine(n, strip=(0, 4)))
        operator = stack.enter_context(P.PcoaEngine(n, operator=True))
        f32 = stack.enter_context(P.PcoaEngine(n, gram_kernel="f32"))
        king.accumulate_plink_bed_king(planes, rows)

        def refused(bad, what, code_=PCOA_ERR_INVALID_ARG):
            for call in (lambda: king.king_pairs(bad, K.CUTOFF), lambda: king.accumulate_plink_bed_king(bad, rows)):
                with pytest.raises(P.PcoaError) as err:
                    call()
                assert err.value.code == code_ and what in str(err.value), str(err.value)

        refused(planes[:2] + [None] + planes[3:], "planes[2] (PCOA_KING_HET_OR_MISSING) is NULL")
        refused(planes[:4] + [planes[1]], "are the same ctx")
        refused(planes[:4] + [other_n], "has N = %d samples" % (n + 1))
        refused(planes[:3] + [strip] + planes[4:], "a strip owner")
        refused(planes[:1] + [operator] + planes[2:], "an operator ctx")
        refused(planes[:4] + [f32], "PCOA_FLAG_GRAM_F32_MFMA")
        for x in (0.0, -0.1, 0.51, float("nan"), float("inf")):
            with pytest.raises(P.PcoaError) as err:
                king.king_pairs(planes, x)
            assert err.value.code == PCOA_ERR_INVALID_ARG and "(0, 0.5]" in str(err.value)
        _, first, arr = king._king_planes(planes)
        found = ctypes.c_int64(-5)
        buf = np.zeros(4, dtype=king.KING_PAIR_DTYPE)
        msg = lambda: lib.pcoa_last_error(first._ctx)
        assert lib.pcoa_king_pairs(arr, K.CUTOFF, None, 0, None, None, None) == PCOA_ERR_INVALID_ARG and b"n_found_out is NULL" in msg()
        assert lib.pcoa_king_pairs(arr, K.CUTOFF, ctypes.c_void_p(buf.ctypes.data), -1, ctypes.byref(found), None, None) == PCOA_ERR_INVALID_ARG
        assert b"is negative" in msg()
        assert lib.pcoa_king_pairs(arr, K.CUTOFF, None, 4, ctypes.byref(found), None, None) == PCOA_ERR_INVALID_ARG and b"out_pairs is NULL" in msg()
        assert found.value == -5
        ptr = ctypes.c_void_p(rows.ctypes.data)
        assert lib.pcoa_accumulate_plink_bed_king(arr, None, 3, rows.shape[1], 0) == PCOA_ERR_INVALID_ARG and b"bed_rows is NULL" in msg()
        assert lib.pcoa_accumulate_plink_bed_king(arr, ptr, -1, rows.shape[1], 0) == PCOA_ERR_INVALID_ARG and b"n_variants < 0" in msg()
        assert lib.pcoa_accumulate_plink_bed_king(arr, ptr, 3, rows.shape[1] - 1, 0) == PCOA_ERR_INVALID_ARG and b"row_bytes" in msg()
        assert lib.pcoa_accumulate_plink_bed_king(arr, ptr, 3, rows.shape[1], 7) == PCOA_ERR_INVALID_ARG and b"is_device_ptr" in msg()
        assert lib.pcoa_accumulate_plink_bed_king(arr, ptr, 0, rows.shape[1], 0) == 0          # nothing to feed is no error
        check_against_rule(P, vp, planes, grams, K.CUTOFF)               # none of it touched a matrix


def test_planes_on_different_devices_are_refused(P):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("the different-devices refusal needs a second GPU")
    with ExitStack() as stack:
        planes = five(P, stack, 8)
        planes[2] = stack.enter_context(P.PcoaEngine(8, device=1))
        with pytest.raises(P.PcoaError) as err:
            P.PcoaEngine.king_pairs(planes, K.CUTOFF)
        assert err.value.code == PCOA_ERR_INVALID_ARG and "different devices" in str(err.value)


# ------------------------------------------------------------------------------------------------------- 8. state and statistics
def test_state_afterwards_and_statistics(P, vp):
    n = 260
    a, b = random_codes(n, 300, seed=21), random_codes(n, 170, seed=22)
    with ExitStack() as stack:
        planes = five(P, stack, n)
        assert planes[0].king_stats() == {"king_seconds": 0.0, "king_bytes": 0, "king_calls": 0}
        P.PcoaEngine.accumulate_plink_bed_king(planes, K.bed_rows(a))
        grams = grams_of(vp, a)
        first = check_against_rule(P, vp, planes, grams, 0.0884)
        st1 = planes[0].king_stats()
        assert st1["king_calls"] == 1 and st1["king_seconds"] > 0
        # one column tile: the count pass reads the nine bands' rows x 260 columns of five int32 matrices, the write pass the cells with a hit
        assert st1["king_bytes"] >= 20 * n * n and st1["king_bytes"] <= 2 * 20 * n * n
        assert same_pairs(check_against_rule(P, vp, planes, grams, 0.0884), first)              # reproducible
        for eng, g in zip(planes, grams):
            assert np.array_equal(eng.gram(), g)                                                # unchanged
        P.PcoaEngine.accumulate_plink_bed_king(planes, K.bed_rows(b))                           # and the planes go on accumulating
        grams = grams_of(vp, np.concatenate([a, b]))
        check_against_rule(P, vp, planes, grams, 0.0884)
        st3 = planes[0].king_stats()
        assert st3["king_calls"] == 3 and st3["king_bytes"] > st1["king_bytes"] and st3["king_seconds"] > st1["king_seconds"]
        assert planes[1].king_stats()["king_calls"] == 0                                        # the statistics live on planes[0]
        planes[0].reset_timings()
        assert planes[0].king_stats()["king_calls"] == 0


# ------------------------------------------------------------------------------------------------------- 9. both hosts
@pytest.fixture(scope="module")
def host_cohort(tmp_path_factory, vp):
    d = tmp_path_factory.mktemp("kinghosts")
    code = K.codes(K.HOST_N, K.HOST_V)
    names = [K.name_of(i) for i in range(K.HOST_N)]
    prefix = str(d / "set" / "cohort")
    K.write_plink(code, prefix, names)
    want = vp.king_pairs_rule(grams_of(vp, code), K.CUTOFF)
    gone = [int(i) for i in vp.related_removal(want, K.HOST_N)]
    keep = [i for i in range(K.HOST_N) if i not in gone]
    reduced = str(d / "reduced" / "cohort")
    K.write_plink(code[:, keep], reduced, [names[i] for i in keep])
    return {"bed": prefix + ".bed", "reduced": reduced + ".bed", "names": names, "dir": str(d), "want": want, "gone": gone, "keep": keep}


def components(stdout):
    rows = [ln.split("\t") for ln in stdout.splitlines() if ln.count("\t") == 3]
    return [r[0] for r in rows], np.array([[float(r[2]), float(r[3])] for r in rows])


@pytest.mark.parametrize("also", [(), ("--missing-calls", "pairwise")], ids=["shared", "pairwise"])
def test_both_hosts_screen_and_remove(host_cohort, vp, also):
    h = host_cohort
    assert [(int(p["i"]), int(p["j"])) for p in h["want"]] == K.planted_pairs(K.HOST_N)
    tag = "_".join(a.strip("-") for a in also) or "shared"
    files = dict((host, os.path.join(h["dir"], "king_%s_%s.tsv" % (host, tag))) for host in ("driver", "python"))
    runs = {}
    for host, run in (("driver", K.run_driver), ("python", K.run_python)):
        runs[host] = run(["--input-path", h["bed"], "--king-cutoff", "0.177", "--king-output-path", files[host], "--king-remove"] + list(also))
        assert runs[host].returncode == 0, runs[host].stderr
    line = "KING pairs: 10 at kinship >= 0.177; removed %d sample(s): %s" % (len(h["gone"]), ", ".join(h["names"][i] for i in h["gone"]))
    for host in ("driver", "python"):
        assert [ln for ln in runs[host].stderr.splitlines() if ln.startswith("KING pairs")] == [line], runs[host].stderr
    got = open(files["driver"], "rb").read()
    assert got == open(files["python"], "rb").read()
    kin = vp.king_kinship(h["want"])
    want_lines = ["name_i\tname_j\thethet\tibs0\thet_sum\tkinship"] + [
        "%s\t%s\t%d\t%d\t%d\t%s" % (h["names"][p["i"]], h["names"][p["j"]], p["hethet"], p["ibs0"], p["het_sum"], vp.java_double_to_string(float(k)))
        for p, k in zip(h["want"], kin)]
    assert got.decode().splitlines() == want_lines
    assert runs["driver"].stdout.encode() == runs["python"].stdout.encode()
    # the components after the removal: a run on the fileset written without the removed samples
    fresh = K.run_driver(["--input-path", h["reduced"]] + list(also))
    assert fresh.returncode == 0, fresh.stderr
    names_a, a = components(runs["driver"].stdout)
    names_b, b = components(fresh.stdout)
    assert names_a == names_b == [h["names"][i] for i in h["keep"]]
    for c in range(2):
        col = a[:, c] if np.dot(a[:, c], b[:, c]) >= 0 else -a[:, c]
        assert np.linalg.norm(col - b[:, c]) < 1e-6


def test_a_run_without_the_flag_prints_what_it_printed(host_cohort):
    """--king-cutoff without --king-remove screens and reports, and the coordinates are those of a run without the flag."""
    h = host_cohort
    a = K.run_driver(["--input-path", h["bed"], "--king-cutoff", "0.177"])
    b = K.run_driver(["--input-path", h["bed"]])
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    assert a.stdout.encode() == b.stdout.encode()
    assert "KING pairs: 10 at kinship >= 0.177; removed 0 sample(s)\n" in a.stderr and "KING pairs" not in b.stderr

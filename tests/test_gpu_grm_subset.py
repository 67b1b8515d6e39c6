"""GPU tests of the sample subsets of a GRM store (pcoa_create_grm_subset, pcoa_grm_rows): the gathered store
is the numpy statement of tests/grm_subset_cohort.py byte for byte, at every keep-list pattern, sample count, row count and
segment cut where the kernel takes another path; the result is indistinguishable, bit for bit in every later call, from an
engine that was fed the re-packed rows; "PCA on the kept, project the removed" needs nothing else; errors leave the source as it
was; and both hosts serve --grm-keep-samples / --grm-remove-samples / --grm-outlier-iterations / --grm-project-removed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import grm_subset_cohort as C
from conftest import ROOT, load_golden, load_pkg, write_golden_plink
from test_grm_cpu import balding_nichols, edge_rows, pack_bed, random_codes

pytestmark = pytest.mark.gpu

SEGMENT_KNOB = "PCOA_GRM_SEGMENT_ROWS"
TILE = 8            # grm_subset.hip's kGrmSubsetTileRows (held to the source by tests/test_grm_subset_cpu.py)


@pytest.fixture(scope="module")
def P():
    return load_pkg()


def fed(P, n, rows, ref_is_a1=True, study=False):
    eng = P.PcoaEngine(n, grm=not study, grm_study=study)
    eng.accumulate_plink_bed(rows, ref_is_a1=ref_is_a1)
    eng.sync()
    return eng


def cohort_rows(n, v, seed, garbage=True):
    """.bed rows of a random cohort with the edge rows (monomorphic, all-missing, all-het), garbage in the padding slots."""
    rng = np.random.default_rng(seed)
    codes = edge_rows(random_codes(rng, v, n, missing=0.1))
    return pack_bed(codes, 0, rng if garbage else None)


def legal(keep, study):
    return keep.size >= (1 if study else 32)


# ---- exact bytes ------------------------------------------------------------------------------------------------------------
SHAPES_N = [32, 33, 47, 48, 49, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 4100]


@pytest.mark.parametrize("n_src", SHAPES_N)
def test_rows_of_a_subset_are_the_specs_bytes_at_every_pattern(P, n_src):
    v = 11
    rows = cohort_rows(n_src, v, n_src)
    seen = 0
    for ref_is_a1 in (True, False):
        want_src = C.store_rows(rows, n_src, ref_is_a1)
        with fed(P, n_src, rows, ref_is_a1) as src:
            assert np.array_equal(src.grm_rows(), want_src)              # 00 tails whatever the padding slots of the input held
            for name, keep in C.keep_patterns(n_src, int(ref_is_a1)).items():
                want = C.spec_grm_subset_rows(want_src, n_src, keep)
                for study in (False, True):
                    if not legal(keep, study):
                        continue
                    with src.grm_subset(keep, study=study) as sub:
                        got = sub.grm_rows()
                        assert sub.n == keep.size and sub.grm_info()[0] == v
                    assert np.array_equal(got, want), (name, study, ref_is_a1)
                    if name == "identity":
                        assert np.array_equal(got, want_src)
                    seen += 1
            assert np.array_equal(src.grm_rows(), want_src)              # the source is as it was
    assert seen >= 2 * 9                                                 # every pattern as a study, both flags


@pytest.mark.parametrize("m", [1, 15, 16, 17, 63, 64, 65])
def test_a_study_subset_goes_down_to_one_sample(P, m):
    n_src, v = 130, 9
    rows = cohort_rows(n_src, v, 7 * m)
    rng = np.random.default_rng(m)
    want_src = C.store_rows(rows, n_src, False)
    with fed(P, n_src, rows, False) as src:
        for keep in (np.arange(m), np.arange(n_src - m, n_src), np.sort(rng.choice(n_src, size=m, replace=False))):
            keep = keep.astype(np.int32)
            with src.grm_subset(keep, study=True) as sub:
                assert np.array_equal(sub.grm_rows(), C.spec_grm_subset_rows(want_src, n_src, keep))
                assert np.array_equal(sub.grm_rows(2, 5), C.spec_grm_subset_rows(want_src[2:7], n_src, keep))


@pytest.mark.parametrize("v", [1, 2, TILE - 1, TILE, TILE + 1, 8 * TILE - 1, 8 * TILE, 8 * TILE + 1, 2047, 2048, 2049])
def test_row_counts_around_the_kernels_tiles(P, v):
    """A lane streams tiles of TILE rows; a launch deals one row stream per 8 tiles: V around both, and around 2,048."""
    for n_src in (33, 1025):
        rows = cohort_rows(n_src, v, v + n_src)
        want_src = C.store_rows(rows, n_src, bool(v & 1))
        pats = C.keep_patterns(n_src, v)
        with fed(P, n_src, rows, bool(v & 1)) as src:
            for name in ("one_mid_word", "random_50pct") + (("one_per_16",) if n_src == 1025 else ()):
                with src.grm_subset(pats[name], study=n_src == 33) as sub:
                    assert np.array_equal(sub.grm_rows(), C.spec_grm_subset_rows(want_src, n_src, pats[name])), (n_src, name)


# ---- indistinguishable from a fed engine ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src,m", [(260, 200), (1025, 1000)])
def test_a_subset_is_indistinguishable_from_an_engine_fed_the_repacked_rows(P, n_src, m):
    import torch
    v = 1500
    rng = np.random.default_rng(n_src)
    codes = edge_rows(balding_nichols(rng, n_src, v, missing=0.05))
    rows = pack_bed(codes, 0, rng)
    keep = np.sort(rng.choice(n_src, size=m, replace=False)).astype(np.int32)
    spec = C.spec_grm_subset_rows(C.store_rows(rows, n_src, False), n_src, keep)
    x = torch.from_numpy(rng.standard_normal(m)).cuda()
    with fed(P, n_src, rows, False) as src, src.grm_subset(keep) as sub, fed(P, m, spec, True) as ref:
        assert sub.grm_info() == ref.grm_info()
        assert np.array_equal(sub.grm_counts(), ref.grm_counts())
        ya, yb = sub.grm_matvec_device(x).cpu().numpy(), ref.grm_matvec_device(x).cpu().numpy()
        assert ya.tobytes() == yb.tobytes() and np.abs(ya).max() > 0       # padding that is not 01 would count as called here
        ka, na = sub.grm_block(17, 30, 3, 45, pairs=True)
        kb, nb = ref.grm_block(17, 30, 3, 45, pairs=True)
        assert ka.tobytes() == kb.tobytes() and np.array_equal(na, nb)
        ka, na = sub.grm_block(m - 40, 40, m - 33, 33, divisor="pairwise", pairs=True)   # the last word column and its padding
        kb, nb = ref.grm_block(m - 40, 40, m - 33, 33, divisor="pairwise", pairs=True)
        assert ka.tobytes() == kb.tobytes() and np.array_equal(na, nb)
        ca, la, nza = sub.compute(2)
        cb, lb, nzb = ref.compute(2)
        assert nza == nzb and np.array_equal(la, lb) and np.array_equal(ca, cb)
        assert sub.grm_ld_prune(20, 0.2) == ref.grm_ld_prune(20, 0.2)
        assert np.array_equal(sub.grm_ld_mask(), ref.grm_ld_mask())
        assert sub.grm_info() == ref.grm_info()


# ---- project the removed ----------------------------------------------------------------------------------------------------
def test_projecting_the_removed_samples_and_a_subset_of_a_subset(P):
    n_src, v = 260, 1200
    rng = np.random.default_rng(26)
    codes = balding_nichols(rng, n_src, v, missing=0.05)
    rows = pack_bed(codes, 0, rng)
    store = C.store_rows(rows, n_src, False)
    removed = np.sort(rng.choice(n_src, size=37, replace=False)).astype(np.int32)
    kept = np.setdiff1d(np.arange(n_src), removed).astype(np.int32)
    with fed(P, n_src, rows, False) as src, src.grm_subset(kept) as panel, src.grm_subset(removed, study=True) as study, \
            fed(P, removed.size, C.spec_grm_subset_rows(store, n_src, removed), True, study=True) as ref:
        comps, lam, _ = panel.compute(2)
        ca, na = panel.grm_project(study, comps, lam)
        cb, nb = panel.grm_project(ref, comps, lam)
        assert ca.shape == (37, 2) and ca.tobytes() == cb.tobytes() and np.array_equal(na, nb) and np.abs(ca).max() > 0
        # a subset of a subset is the subset of the composed list, either kind as the source
        inner = np.sort(rng.choice(kept.size, size=100, replace=False)).astype(np.int32)
        with panel.grm_subset(inner) as twice, src.grm_subset(kept[inner]) as once:
            assert np.array_equal(twice.grm_rows(), once.grm_rows())
            assert np.array_equal(twice.grm_rows(), C.spec_grm_subset_rows(store, n_src, kept[inner]))
        with study.grm_subset(np.arange(32, dtype=np.int32)) as from_study:      # a panel out of a study store
            assert np.array_equal(from_study.grm_rows(), C.spec_grm_subset_rows(store, n_src, removed[:32]))
            assert from_study.compute(2)[1].shape == (2,)


# ---- segments ---------------------------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(tests)r)
from conftest import load_pkg
import grm_subset_cohort as C
from test_grm_cpu import edge_rows, pack_bed, random_codes
P = load_pkg()
rng = np.random.default_rng(96)
n_src = 130
for v in (95, 96, 97, 200):
    rows = pack_bed(edge_rows(random_codes(rng, v, n_src, missing=0.1)), 0, rng)
    store = C.store_rows(rows, n_src, False)
    with P.PcoaEngine(n_src, grm=True) as src:
        for r0 in range(0, v, 41):                                 # ragged calls
            src.accumulate_plink_bed(rows[r0:r0 + 41])
        assert src.grm_info()[2] == -(-v // 96) * 96 * 48, src.grm_info()      # segments of 96 rows of 48 bytes
        for name, keep in C.keep_patterns(n_src, v).items():
            for study in (False, True):
                if keep.size < (1 if study else 32):
                    continue
                with src.grm_subset(keep, study=study) as sub:
                    pitch = ((keep.size + 3) // 4 + 15) // 16 * 16
                    assert sub.grm_info()[2] == -(-v // 96) * 96 * pitch
                    assert np.array_equal(sub.grm_rows(), C.spec_grm_subset_rows(store, n_src, keep)), (v, name)
                    assert np.array_equal(sub.grm_rows(90, v - 90), C.spec_grm_subset_rows(store[90:], n_src, keep))
print("SEGMENTS-OK")
"""


def test_subsets_across_segment_boundaries():
    """Segments of 96 rows on both sides (the knob is read once per process: a fresh child), V = 95, 96, 97, 200 in ragged calls."""
    env = dict(os.environ)
    env[SEGMENT_KNOB] = "96"
    res = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests")}], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0 and "SEGMENTS-OK" in res.stdout, res.stdout[-3000:]


def test_the_two_stores_cut_their_segments_at_different_rows(P):
    """N_src = 70,000 (rows of 17,504 bytes: 14,336 to a segment), every second sample kept (8,752 bytes: 28,672 to a segment),
    16,000 rows of random bytes -- every byte is four valid codes: the source holds two segments, the result one."""
    import torch
    n_src, v = 70000, 16000
    rng = np.random.default_rng(70)
    rows = rng.integers(0, 256, size=(v, n_src // 4), dtype=np.uint8)
    keep = np.arange(0, n_src, 2, dtype=np.int32)
    src_seg = (256 << 20) // 17504 // 2048 * 2048
    assert src_seg == 14336 and (256 << 20) // 8752 // 2048 * 2048 == 28672
    with P.PcoaEngine(n_src, grm=True) as src:
        src.accumulate_plink_bed(torch.from_numpy(rows).cuda(), ref_is_a1=True)
        assert src.grm_info()[2] == 2 * src_seg * 17504
        with src.grm_subset(keep) as sub:
            assert sub.grm_info()[2] == 28672 * 8752
            for r in (0, 1, src_seg - 2, src_seg - 1, src_seg, src_seg + 1, 7777, v - 2, v - 1):
                assert np.array_equal(sub.grm_rows(r, 1), C.spec_grm_subset_rows(rows[r:r + 1], n_src, keep)), r
            got = sub.grm_counts()
    lo, hi = rows & 0x03, (rows >> 4) & 0x03                     # the kept samples of a byte: slots 0 and 2
    want = np.stack([(lo != 1).sum(axis=1) + (hi != 1).sum(axis=1), (lo == 2).sum(axis=1) + (hi == 2).sum(axis=1),
                     (lo == 3).sum(axis=1) + (hi == 3).sum(axis=1)], axis=1).astype(np.int32)
    assert np.array_equal(got, want)


# ---- state and errors -------------------------------------------------------------------------------------------------------
def test_errors_leave_the_source_usable_and_state_follows_the_header(P):
    import torch
    L = P._lib
    lib = L.load()
    n_src, v = 130, 400
    rng = np.random.default_rng(13)
    codes = balding_nichols(rng, n_src, v, missing=0.05)
    codes[110:120] = codes[100:110]                        # rows that repeat the row ten places before them
    rows = pack_bed(codes)
    store = C.store_rows(rows, n_src, False)
    x = torch.from_numpy(rng.standard_normal(n_src)).cuda()
    i32 = ctypes.c_int32

    def raw(ctx, keep, n_keep=None, kind=0, out=True):
        arr = (i32 * max(len(keep or ()), 1))(*(keep or ()))
        got = ctypes.c_void_p(1)
        rc = lib.pcoa_create_grm_subset(ctypes.byref(got) if out else None, ctx, arr if keep is not None else None,
                                        len(keep or ()) if n_keep is None else n_keep, kind)
        assert not out or got.value is None                          # *out = NULL on every error
        return rc

    ok = list(range(40))
    with fed(P, n_src, rows, False) as src, P.PcoaEngine(n_src) as full, P.PcoaEngine(n_src, operator=True) as op:
        src.grm_set_min_maf(0.1)
        y0 = src.grm_matvec_device(x).cpu().numpy()
        stats0 = src.grm_subset_stats()
        assert stats0["grm_subset_calls"] == 0 and stats0["grm_subset_bytes"] == 0
        bad = [(None, 40, 0), (ok[:31], None, 0), ([], None, 1), (ok, None, 2), (ok, None, -1), ([-1] + ok, None, 0),
               (ok + [n_src], None, 0), (ok + [39], None, 0), (ok + [38], None, 1), (ok, -5, 1)]
        for keep, n_keep, kind in bad:
            assert raw(src._ctx, keep, n_keep, kind) == L.PCOA_ERR_INVALID_ARG, (keep, n_keep, kind)
            assert b"pcoa_create_grm_subset" in lib.pcoa_last_error(src._ctx)
        assert raw(src._ctx, ok, out=False) == L.PCOA_ERR_INVALID_ARG
        for other, word in ((full, "full engine"), (op, "operator")):
            assert raw(other._ctx, ok) == L.PCOA_ERR_STATE and word.encode() in lib.pcoa_last_error(other._ctx)
            with pytest.raises(P.PcoaError) as ei:
                other.grm_rows(0, 0)
            assert ei.value.code == L.PCOA_ERR_STATE and word in str(ei.value)
        for args in ((-1, 2), (0, v + 1), (v, 1)):
            with pytest.raises(P.PcoaError) as ei:
                src.grm_rows(*args)
            assert ei.value.code == L.PCOA_ERR_INVALID_ARG
        assert lib.pcoa_grm_rows(src._ctx, 0, 1, None) == L.PCOA_ERR_INVALID_ARG
        with pytest.raises(P.PcoaError) as ei:                       # the stored-S subset stays refused on a GRM ctx
            src.subset(np.arange(40))
        assert ei.value.code == L.PCOA_ERR_STATE
        assert src.grm_subset_stats() == stats0                      # no error counted
        assert src.grm_matvec_device(x).cpu().numpy().tobytes() == y0.tobytes()

        # min_maf is inherited, the LD mask is not
        cand, kept_rows = src.grm_ld_prune(10, 0.05)
        assert 0 < kept_rows < cand
        pruned = src.grm_info()[1]
        keep = np.delete(np.arange(n_src, dtype=np.int32), [3, 64, 129])
        spec = C.spec_grm_subset_rows(store, n_src, keep)
        with src.grm_subset(keep) as sub, fed(P, keep.size, spec, True) as ref:
            ref.grm_set_min_maf(0.1)
            with pytest.raises(P.PcoaError) as ei:
                sub.grm_ld_mask()
            assert ei.value.code == L.PCOA_ERR_STATE and "no keep mask" in str(ei.value)
            assert sub.grm_info() == ref.grm_info()
            ref.grm_set_min_maf(0.0)
            assert sub.grm_info()[1] < ref.grm_info()[1]             # (the cut-off does remove variants of this cohort)
            assert src.grm_info()[1] == pruned                       # the source keeps its mask
            st = src.grm_subset_stats()
            assert st["grm_subset_calls"] == 1 and st["grm_subset_bytes"] == v * (48 + 32) and st["grm_subset_seconds"] > 0
            assert sub.grm_subset_stats()["grm_subset_calls"] == 0
            # the source is fed further: the result does not change, the next subset sees the new rows
            before = sub.grm_rows()
            src.accumulate_plink_bed(rows[:7])
            assert np.array_equal(sub.grm_rows(), before) and sub.grm_info()[0] == v
            with src.grm_subset(keep, study=True) as later:
                assert later.grm_info()[0] == v + 7
                assert np.array_equal(later.grm_rows(v, 7), spec[:7])
            assert src.grm_subset_stats()["grm_subset_bytes"] == (2 * v + 7) * (48 + 32)
        # an empty store gives an empty result
        src.reset()
        with src.grm_subset(keep) as empty:
            assert empty.grm_info()[:2] == (0, 0) and empty.grm_rows().shape == (0, (keep.size + 3) // 4)
    # a result outlives its source
    with fed(P, n_src, rows, False) as src:
        sub = src.grm_subset(keep)
    with sub:
        assert np.array_equal(sub.grm_rows(), spec)


# ---- hosts ------------------------------------------------------------------------------------------------------------------
# Every line of a run's stdout is pinned per host: the kept samples' rows and the other lines to what the same host prints for
# --grm on a fileset written without the removed samples (where the hosts agree line for line: tests/test_gpu_grm.py), the removed
# samples' rows to the ABI-level projection.  So the two hosts agree line for line here too.
def rows_of(text):
    return [ln for ln in text.splitlines() if ln.count("\t") == 3]


def other_lines(text, n_from=None, n_to=None):
    out = [ln for ln in text.splitlines() if ln.count("\t") != 3]
    return [ln.replace("Matrix size: %d." % n_from, "Matrix size: %d." % n_to) for ln in out] if n_from else out


def pitch_bytes(n):
    return ((n + 3) // 4 + 15) // 16 * 16


def host(tag):
    from test_grm_cpu import _run_driver, _run_python
    return {"cpp": _run_driver, "py": _run_python}[tag]


@pytest.mark.parametrize("tag", ["cpp", "py"])
def test_hosts_decompose_the_listed_cohort_and_place_the_removed_samples(P, tmp_path, tag):
    """The tile260 golden: --grm --grm-remove-samples (and --grm-keep-samples with the complement) print, for the kept samples,
    the very text --grm prints on a fileset written with only those samples; .grm.id and the matrix files follow the cohort;
    --grm-project-removed appends the rows of the ABI-level projection."""
    import re
    from test_grm_project_cpu import read_fileset, write_fileset
    vp = load_pkg("variants_pca")
    run = host(tag)
    os.mkdir(str(tmp_path / "full"))
    os.mkdir(str(tmp_path / "kept"))
    full, only = str(tmp_path / "full" / "tile260"), str(tmp_path / "kept" / "tile260")     # the same stem: the same dataset column
    n = write_golden_plink(load_golden("tile260"), full)
    codes, bim, fam = read_fileset(full)
    gone = np.arange(3, n, 17)
    mask = np.zeros(n, dtype=bool)
    mask[gone] = True
    m = n - gone.size
    write_fileset(only, codes[:, ~mask], bim, [ln for ln, k in zip(fam, mask) if not k])
    names = [ln.split()[1] for ln in fam]
    with open(str(tmp_path / "remove.txt"), "w") as f:
        f.write("".join("%s\n" % names[i] for i in gone[::-1]))                           # any order, a blank line at the end
        f.write("\n")
    with open(str(tmp_path / "keep.txt"), "w") as f:
        f.write("".join("  %s \n" % names[i] for i in np.nonzero(~mask)[0]))
    # the ABI-level projection of the removed samples
    with P.PcoaEngine(n, grm=True) as eng:
        eng.accumulate_plink_bed(pack_bed(codes))
        with eng.grm_subset(np.nonzero(~mask)[0]) as panel, eng.grm_subset(gone, study=True) as study:
            comps, lam, _ = panel.compute(2)
            xy, called = panel.grm_project(study, comps, lam)
            used = panel.grm_info()[1]
    jd = vp.java_double_to_string
    want_removed = ["%s\ttile260\t%s\t%s" % (names[i], jd(float(xy[q, 0])), jd(float(xy[q, 1]))) for q, i in enumerate(gone)]
    want_line = "Projected %d removed samples over %d used variants (mean call share %.4f)" % (gone.size, used, float(called.mean()) / used)
    pa, pb = str(tmp_path / "plain"), str(tmp_path / "removed")
    plain = run(["--input-path", only + ".bed", "--all-references", "--grm", "--grm-output-path", pa])
    rem = run(["--input-path", full + ".bed", "--all-references", "--grm", "--grm-remove-samples", str(tmp_path / "remove.txt"),
               "--grm-output-path", pb])
    keep = run(["--input-path", full + ".bed", "--all-references", "--grm", "--grm-keep-samples", str(tmp_path / "keep.txt"),
                "--grm-project-removed"])
    for res in (plain, rem, keep):
        assert res.returncode == 0, res.stderr[-2000:]
    want = rows_of(plain.stdout)
    assert len(want) == m and rows_of(rem.stdout) == want
    assert other_lines(rem.stdout) == other_lines(plain.stdout, m, n) and "Non zero rows in matrix: %d / %d." % (m, m) in rem.stdout
    v = int(re.search(r"Standardised genotypes: \d+ of (\d+) variants used", rem.stderr).group(1))
    assert "GRM subset: kept %d of %d samples, %d bytes gathered\n" % (m, n, v * (pitch_bytes(n) + pitch_bytes(m))) in rem.stderr, \
        rem.stderr[-1500:]
    lines = re.findall(r"Standardised genotypes: .*", rem.stderr)
    assert len(lines) == 2 and lines[1] == re.findall(r"Standardised genotypes: .*", plain.stderr)[0]
    for ext in (".grm.id", ".grm.bin", ".grm.N.bin"):
        assert open(pa + ext, "rb").read() == open(pb + ext, "rb").read(), ext
    assert open(pb + ".grm.id").read() == "".join("tile260\t%s\n" % names[i] for i in np.nonzero(~mask)[0])
    got = rows_of(keep.stdout)
    assert got[:m] == want and got[m:] == want_removed and other_lines(keep.stdout) == other_lines(rem.stdout)
    assert want_line in keep.stderr and "Projected" not in rem.stderr, keep.stderr[-1500:]


@pytest.mark.parametrize("tag", ["cpp", "py"])
def test_hosts_remove_the_planted_outliers_in_round_one(tmp_path, tag):
    """A Balding-Nichols cohort plus three all-het samples (tests/test_grm_subset_cpu.py holds the rule's decisions with numpy's
    eigh): --grm-outlier-iterations 2 removes exactly those three in round 1 and nothing in round 2; the final rows are the text
    --grm prints on a fileset without them; the removed come back projected; --grm-ld-window prunes every round's engine."""
    from test_grm_project_cpu import write_fileset
    run = host(tag)
    codes, planted = C.planted_outlier_cohort()
    v, n = codes.shape
    os.mkdir(str(tmp_path / "full"))
    os.mkdir(str(tmp_path / "kept"))
    full, only = str(tmp_path / "full" / "planted"), str(tmp_path / "kept" / "planted")
    fam = ["FAM%d S%04d 0 0 0 -9" % (i, i) for i in range(n)]
    bim = ["1\trs%d\t0\t%d\tC\tA" % (k, 1000 + 7 * k) for k in range(v)]
    mask = np.zeros(n, dtype=bool)
    mask[planted] = True
    write_fileset(full, codes, bim, fam)
    write_fileset(only, codes[:, ~mask], bim, [ln for ln, k in zip(fam, mask) if not k])
    round1 = "Outlier round 1: removed 3 sample(s): %s\n" % ", ".join("S%04d" % i for i in planted)
    plain = run(["--input-path", only + ".bed", "--all-references", "--grm"])
    res = run(["--input-path", full + ".bed", "--all-references", "--grm", "--grm-outlier-iterations", "2", "--grm-project-removed"])
    ld = run(["--input-path", full + ".bed", "--all-references", "--grm", "--grm-outlier-iterations", "2", "--grm-ld-window", "5",
              "--grm-ld-r2", "0.5"])
    for r in (plain, res, ld):
        assert r.returncode == 0, r.stderr[-2000:]
    assert round1 in res.stderr and "Outlier round 2: removed 0 sample(s)\n" in res.stderr and "Outlier round 3" not in res.stderr
    assert "GRM subset: kept %d of %d samples, %d bytes gathered\n" % (n - 3, n, v * (pitch_bytes(n) + pitch_bytes(n - 3))) in res.stderr
    assert "GRM subset: kept 3 of %d samples, %d bytes gathered\n" % (n, v * (pitch_bytes(n) + 16)) in res.stderr
    assert res.stderr.count("GRM subset:") == 2 and res.stderr.count("Standardised genotypes:") == 2
    assert "Projected 3 removed samples over " in res.stderr
    got = rows_of(res.stdout)
    assert got[:n - 3] == rows_of(plain.stdout) and [ln.split("\t")[0] for ln in got[n - 3:]] == ["S%04d" % i for i in planted]
    assert len(got) == n and other_lines(res.stdout) == other_lines(plain.stdout, n - 3, n)
    # with the prune: both rounds' engines are pruned, and the planted samples go all the same
    assert round1 in ld.stderr and ld.stdout.count("GRM LD pruning: kept ") == 2 and len(rows_of(ld.stdout)) == n - 3

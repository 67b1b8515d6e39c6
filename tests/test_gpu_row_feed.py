"""The row feed of the C ABI (csrc/row_feed.h) under its four users -- accumulation, loadings, LD pruning and the two-engine
.bed read -- at the smallest shapes that take every boundary through MORE THAN ONE CHUNK: the staging slot wraps inside a call,
a slot regrows while it is marked used, padded rows take the 2-D copy, and the calls_decoded / calls_read handshake runs
across chunks.  N = 70 throughout: 3 words per bitset row, 18 bytes per .bed row, so a .bed chunk outgrows a slot sized by
bitsets; the row counts sit just past two slots.  Integer and boolean results are compared exactly; the loadings are held to
loadings_cohort.summation_bound, the bound of test_gpu_loadings."""
import numpy as np
import pytest

from conftest import int_gram, load_pkg
from ld_cohort import ld_cohort, ld_rule_banded
from loadings_cohort import centred_eig, decode_bed, encode_bed, loadings_rule, pack_rows, planted_cohort, summation_bound

pytestmark = pytest.mark.gpu

N, WORDS, BED_BYTES = 70, 3, 18
SLOT_ROWS = 1 << 17                                                   # rows of a bitset / .bed staging slot
LD_CHUNK = min(1 << 16, ((256 << 20) // (WORDS * 4)))                 # pcoa_ld_begin's chunk at this N: the row cap binds
V_LD = 2 * LD_CHUNK + 77
V_BIG = 2 * SLOT_ROWS + 5
LD_WINDOW, LD_R2 = 5, 0.5


@pytest.fixture(scope="module")
def P():
    return load_pkg()


def to_dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dtype) if dtype is not None else a).cuda()


@pytest.fixture(scope="module")
def ld_case():
    """(x [V_LD, 70], keep): the cohort of case 1 and its keep mask by the banded rule, computed once."""
    x = ld_cohort(N, V_LD, 7070)
    keep = ld_rule_banded(x, LD_WINDOW, LD_R2)
    keep.setflags(write=False)
    x.setflags(write=False)
    return x, keep


@pytest.fixture(scope="module")
def loadings_case():
    """(x [V_BIG, 70], u, lam, want, bound) of case 2, computed once."""
    x = planted_cohort(N, V_BIG)
    u, lam = centred_eig(x, 2)
    want = loadings_rule(x, u, lam)
    bound = summation_bound(x, u, lam, want)
    for a in (x, u, lam, want, bound):
        a.setflags(write=False)
    return x, u, lam, want, bound


def inside(got, want, bound):
    return bool((np.abs(np.asarray(got).astype(np.longdouble) - want) <= bound).all())


# ---- 1. LD pruning over three chunks ----------------------------------------------------------------------------------------
def test_ld_pruning_over_three_chunks_is_the_same_from_every_source(P, ld_case):
    x, keep = ld_case
    assert LD_CHUNK == 1 << 16 and 2 * LD_CHUNK < V_LD <= 3 * LD_CHUNK
    dense = pack_rows(x, N)
    padded = pack_rows(x, N, pad_words=2)
    padded[:, WORDS:] = 0xa5a5a5a5
    bed = encode_bed(x, N)
    assert dense.shape[1] == WORDS and padded.shape[1] == WORDS + 2 and bed.shape[1] == BED_BYTES
    want_gram = int_gram(x[keep])
    n_kept = int(keep.sum())
    assert 0.25 * V_LD < n_kept < 0.75 * V_LD
    feeds = [("host bitsets, dense", lambda pr: [pr.bits(dense)]),
             ("host bitsets, ld_words = 5", lambda pr: [pr.bits(padded)]),
             ("host .bed rows", lambda pr: [pr.plink_bed(bed)]),
             ("device bitsets", lambda pr: [pr.bits(to_dev(dense, np.int32))]),
             ("host bitsets, calls of 50,000", None)]
    with P.PcoaEngine(N) as eng:
        for what, feed in feeds:
            eng.reset()
            with eng.ld_pruner(LD_WINDOW, LD_R2, accumulate=True) as pr:
                seen0 = pr.stats()["ld_variants"]
                if feed is not None:
                    masks = feed(pr)
                    kept = pr.last_kept
                else:
                    masks, kept = [], 0
                    for v0 in range(0, V_LD, 50000):
                        masks.append(pr.bits(dense[v0:v0 + 50000]))
                        kept += pr.last_kept
                seen = pr.stats()["ld_variants"] - seen0
            got = np.concatenate(masks)
            assert seen == V_LD, what                   # > 2 chunks of LD_CHUNK rows went through the pruner
            assert got.dtype == bool and np.array_equal(got, keep), "%s: %d rows differ" % (what, int((got != keep).sum()))
            assert kept == n_kept, what
            assert np.array_equal(eng.gram(), want_gram), what


# ---- 2. loadings over three chunks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_out", [False, True])
def test_loadings_over_three_chunks_stay_inside_the_summation_bound(P, loadings_case, device_out):
    x, u, lam, want, bound = loadings_case
    dense = pack_rows(x, N)
    padded = pack_rows(x, N, pad_words=2, garbage=np.random.default_rng(2))
    bed = encode_bed(x, N)
    assert np.array_equal(decode_bed(bed[:1000], N), x[:1000])
    with P.PcoaEngine(N) as eng, eng.loadings(u, lam) as ld:
        feeds = [("host bitsets, dense", lambda: ld.bits(dense, device_out=device_out)),
                 ("host bitsets, padded", lambda: ld.bits(padded, device_out=device_out)),
                 ("host .bed rows", lambda: ld.plink_bed(bed, device_out=device_out)),
                 ("device .bed rows", lambda: ld.plink_bed(to_dev(bed), device_out=device_out))]
        for what, feed in feeds:
            seen0 = ld.stats()["loadings_variants"]
            got = feed()
            got = got.cpu().numpy() if device_out else got
            assert ld.stats()["loadings_variants"] - seen0 == V_BIG, what
            assert got.shape == want.shape and inside(got, want, bound), what


# ---- 3. two engines from one read, over three chunks --------------------------------------------------------------------------
@pytest.mark.parametrize("ref_is_a1", [False, True])
def test_two_engines_from_one_read_over_three_chunks(P, ref_is_a1):
    import torch
    rng = np.random.default_rng(303 + int(ref_is_a1))
    x = rng.random((V_BIG + 1000, N)) < 0.12
    missing = rng.random(x.shape) < 0.10
    rows = encode_bed(x, N, missing=missing, ref_is_a1=ref_is_a1, rng=rng)
    carriers = decode_bed(rows, N, ref_is_a1=ref_is_a1)
    assert np.array_equal(carriers, x & ~missing)
    rows, extra = rows[:V_BIG], rows[V_BIG:]
    want_s, want_q = int_gram(carriers[:V_BIG]), int_gram(missing[:V_BIG])
    extra_s = int_gram(carriers[V_BIG:])
    half = V_BIG // 2
    pinned = [torch.from_numpy(rows[:half]).pin_memory(), torch.from_numpy(rows[half:]).pin_memory()]

    def pageable(eng, q):
        eng.accumulate_plink_bed_calls(rows, q, ref_is_a1=ref_is_a1)
        return 1

    def device(eng, q):
        eng.accumulate_plink_bed_calls(to_dev(rows), q, ref_is_a1=ref_is_a1)
        return 1

    def queued(eng, q):
        for _ in range(2):
            for t in pinned:
                eng.accumulate_plink_bed_calls(t, q, ref_is_a1=ref_is_a1, asynchronous=True)
        return 2

    with P.PcoaEngine(N) as eng, P.PcoaEngine(N) as q:
        for feed in (pageable, device, queued):
            times = feed(eng, q)
            # no sync in between: the next decode into the carrier rows runs behind whatever still reads the last chunk
            eng.accumulate_plink_bed(extra, ref_is_a1=ref_is_a1)
            eng.sync()
            assert np.array_equal(eng.gram(), times * want_s + extra_s), feed.__name__
            assert np.array_equal(q.gram(), times * want_q), feed.__name__
            eng.reset()
            q.reset()


# ---- 4. one ring, four users ------------------------------------------------------------------------------------------------
def test_one_ring_serves_four_users_in_turn(P, ld_case, loadings_case):
    rng = np.random.default_rng(404)
    x1 = rng.random((2 * SLOT_ROWS + 4097, N)) < 0.1
    x_load, u, lam, want, bound = loadings_case
    v2 = SLOT_ROWS + 5
    x_ld = ld_case[0][:LD_CHUNK + 9]
    keep = ld_rule_banded(x_ld, LD_WINDOW, LD_R2)
    x4 = rng.random((SLOT_ROWS + 5, N)) < 0.1
    with P.PcoaEngine(N) as eng:
        eng.accumulate_bits(pack_rows(x1, N))
        with eng.loadings(u, lam) as ld:
            got_w = ld.plink_bed(encode_bed(x_load[:v2], N))         # 2^17 x 18 B: both slots regrow while marked used
        with eng.ld_pruner(LD_WINDOW, LD_R2, accumulate=True) as pr:
            got_keep = pr.bits(pack_rows(x_ld, N))
        eng.accumulate_plink_bed(encode_bed(x4, N, rng=rng))
        got = eng.gram()
    assert inside(got_w, want[:v2], bound[:v2])
    assert np.array_equal(got_keep, keep)
    assert np.array_equal(got, int_gram(x1) + int_gram(x_ld[keep]) + int_gram(x4))

"""GPU tests of the band passes over a strip (csrc/center.hip): strip_band_kernel<MATVEC, HAS64> + strip_finish_kernel behind
pcoa_strip_col_sums / pcoa_strip_matvec / pcoa_strip_matvec_device, and project_band_kernel<K, HAS64> + project_finish_kernel
behind pcoa_project, at the edges of their launch shape: row tails of the 4-deep software pipeline behind a 256-row band, the
FULL / masked split of a 256-column wave, the 1,024-column workgroup, every K chunk.  The twins, the cohorts and the shape
lists (each value tied to its constant) live in tests/strip_cohort.py; tests/test_strip_band_cpu.py holds them to int64
arithmetic and to a long-double sum without a GPU.

Exact cohorts compare with int64 arithmetic (a wrong term fails), rounded cohorts with the ordered twin BIT FOR BIT (a wrong
order or a fused operation fails).  Smallest strip owner: n = 1, strip (0, 1).  pcoa_project refuses num_pc > n_ref, so the
reference sizes below 15 (1, 4, 5) run with n_ref components instead of 15."""
import numpy as np
import pytest

import strip_cohort as C
from conftest import load_pkg

pytestmark = pytest.mark.gpu

STRIPS = C.strip_shapes()
PROJECTS = C.project_shapes()
_id = lambda v: "-".join(str(a) for a in v) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def E():
    return load_pkg("engine")


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _strip_engine(E, n, col0, s, big):
    e = E.PcoaEngine(n, strip=(col0, s.shape[1]))
    e.load_gram(s)
    assert e.timings()["gram_i64_live"] == (1 if big else 0)
    return e


def _still_serves(e, s):
    """after the passes the engine reads back a corner of what was loaded"""
    r, c = min(8, s.shape[0]), min(8, s.shape[1])
    assert np.array_equal(e.gram_block(s.shape[0] - r, s.shape[1] - c, r, c), s[s.shape[0] - r:, s.shape[1] - c:])


# ------------------------------------------------------------------------------------------------------------ the strip passes
@pytest.mark.parametrize("big", [False, True], ids=["i32", "i64"])
@pytest.mark.parametrize("shape", STRIPS, ids=_id)
def test_col_sums_and_the_exact_matvec_are_the_int64_arithmetic(E, shape, big):
    n, col0, cols = shape
    s = C.strip_of(n, col0, cols, big)
    v, means, mm = C.exact_strip_inputs(n)
    with _strip_engine(E, n, col0, s, big) as e:
        assert np.array_equal(e.strip_col_sums(), C.twin_strip_col_sums(s))
        got = e.strip_matvec(v, means, mm)
        assert np.array_equal(got, C.int_strip_matvec(s, col0, v, means, mm))
        assert _same_bytes(got, e.strip_matvec(v, means, mm))
        assert np.array_equal(e.strip_col_sums(), C.twin_strip_col_sums(s))      # the two passes share the workspace
        _still_serves(e, s)


def _rounded_matvec(E, shape, big):
    import torch
    n, col0, cols = shape
    s = C.strip_of(n, col0, cols, big)
    v, means, mm = C.rounded_strip_inputs(n)
    want = C.twin_strip_matvec(s, col0, v, means, mm)
    with _strip_engine(E, n, col0, s, big) as e:
        got = e.strip_matvec(v, means, mm)
        assert np.array_equal(got, want), (shape, int(np.sum(got != want)), float(np.max(np.abs(got - want))))
        assert _same_bytes(got, e.strip_matvec(v, means, mm))
        e.strip_set_centering(means, mm)
        dev = e.strip_matvec_device(torch.from_numpy(v).to("cuda:%d" % e.device)).cpu().numpy()
        assert _same_bytes(got, dev)
        _still_serves(e, s)


@pytest.mark.parametrize("shape", STRIPS, ids=_id)
def test_the_rounded_matvec_is_the_ordered_twin_bit_for_bit(E, shape):
    _rounded_matvec(E, shape, False)


@pytest.mark.parametrize("shape", C.I64_ROUNDED_STRIPS, ids=_id)
def test_the_rounded_matvec_with_an_int64_part_is_the_ordered_twin_bit_for_bit(E, shape):
    _rounded_matvec(E, shape, True)


@pytest.mark.parametrize("shape", [(261, 196, 65), (1289, 8, 1281)], ids=_id)
def test_an_int32_partial_on_top_of_an_int64_part_is_added_in(E, shape):
    """load_gram of entries beyond int32 leaves the int32 matrix zero; one more variant carried by every sample puts a 1 into
    each of its entries, so the kernels' lo + hi has both parts non-zero."""
    n, col0, cols = shape
    s = C.strip_of(n, col0, cols, True)
    v, means, mm = C.exact_strip_inputs(n)
    rv, rmeans, rmm = C.rounded_strip_inputs(n)
    with _strip_engine(E, n, col0, s, True) as e:
        e.accumulate_callsets([list(range(n))])
        s1 = s + 1
        assert np.array_equal(e.gram(), s1)
        assert np.array_equal(e.strip_col_sums(), C.twin_strip_col_sums(s1))
        assert np.array_equal(e.strip_matvec(v, means, mm), C.int_strip_matvec(s1, col0, v, means, mm))
        assert np.array_equal(e.strip_matvec(rv, rmeans, rmm), C.twin_strip_matvec(s1, col0, rv, rmeans, rmm))


@pytest.mark.parametrize("a", [1, 64, 255])
def test_columns_of_a_strip_are_independent(E, a):
    """(c0, w) against (c0, a) + (c0 + a, w - a): the same bytes, column sums and rounded product"""
    n, c0, w = 1289, 7, 1025
    v, means, mm = C.rounded_strip_inputs(n)
    out = []
    for (p0, pw) in [(c0, w), (c0, a), (c0 + a, w - a)]:
        s = C.strip_of(n, p0, pw)
        with _strip_engine(E, n, p0, s, False) as e:
            out.append((e.strip_col_sums(), e.strip_matvec(v, means, mm)))
            _still_serves(e, s)
    for q in (0, 1):
        assert _same_bytes(out[0][q], np.concatenate([out[1][q], out[2][q]]))


# ---------------------------------------------------------------------------------------------------------------- pcoa_project
def _engines(E, co, ref_big=False, cross_big=False):
    ref = E.PcoaEngine(co.n_ref)
    ref.load_gram(co.reference(ref_big))
    cross = E.PcoaEngine(co.n_ref + co.cols, strip=(co.n_ref, co.cols))
    cross.load_gram(co.cross(cross_big))
    assert ref.timings()["gram_i64_live"] == (1 if ref_big else 0)
    assert cross.timings()["gram_i64_live"] == (1 if cross_big else 0)
    return ref, cross


def _exact_projection(E, shape, num_pc, cross_big):
    co = C.exact_project_cohort(*shape)
    want = C.int_project(co)[:, :num_pc]
    ref, cross = _engines(E, co, cross_big=cross_big)
    try:
        got = ref.project(cross, co.comps(num_pc), co.lam[:num_pc])
        assert got.shape == (co.cols, num_pc)
        assert np.array_equal(got, want), (shape, num_pc, np.argwhere(got != want)[:4].tolist())
        assert _same_bytes(got, ref.project(cross, co.comps(num_pc), co.lam[:num_pc]))
        _still_serves(cross, co.cross(cross_big))
        _still_serves(ref, co.r)
    finally:
        cross.close()
        ref.close()


@pytest.mark.parametrize("cross_big", [False, True], ids=["i32", "i64"])
@pytest.mark.parametrize("shape", PROJECTS, ids=_id)
def test_projection_of_an_exact_cohort_is_the_int64_arithmetic(E, shape, cross_big):
    _exact_projection(E, shape, C.num_pc_at(shape[0]), cross_big)


@pytest.mark.parametrize("cross_big", [False, True], ids=["i32", "i64"])
@pytest.mark.parametrize("num_pc", [k for k in C.NUM_PCS if k != C.MAX_PC])
@pytest.mark.parametrize("shape", [C.PROJECT_NARROW, C.PROJECT_WIDE], ids=_id)
def test_every_chunk_sequence_of_components_is_the_int64_arithmetic(E, shape, num_pc, cross_big):
    _exact_projection(E, shape, num_pc, cross_big)


def _rounded_projection(E, shape, ref_big=False, cross_big=False, one_by_one=True):
    co = C.rounded_project_cohort(*shape)
    mean, mm = C.reference_centring(co.reference(ref_big))
    want = C.twin_project(co.cross(cross_big), co.n_ref, mean, mm, co.u, co.lam)
    k = co.lam.size
    ref, cross = _engines(E, co, ref_big=ref_big, cross_big=cross_big)
    try:
        got = ref.project(cross, co.comps(), co.lam)
        assert np.array_equal(got, want), (shape, int(np.sum(got != want)), float(np.max(np.abs(got - want))))
        assert _same_bytes(got, ref.project(cross, co.comps(), co.lam))
        if one_by_one:    # a component's additions depend neither on its chunk's K nor on its place in it
            for c in range(k):
                one = ref.project(cross, co.comps()[:, c:c + 1], co.lam[c:c + 1])
                assert _same_bytes(np.ascontiguousarray(got[:, c:c + 1]), one), c
        _still_serves(cross, co.cross(cross_big))
        _still_serves(ref, co.reference(ref_big))
    finally:
        cross.close()
        ref.close()


@pytest.mark.parametrize("shape", PROJECTS, ids=_id)
def test_projection_of_a_rounded_cohort_is_the_ordered_twin_bit_for_bit(E, shape):
    _rounded_projection(E, shape)


@pytest.mark.parametrize("shape", C.I64_ROUNDED_PROJECT, ids=_id)
def test_rounded_projection_with_an_int64_part_in_the_cross_strip(E, shape):
    _rounded_projection(E, shape, cross_big=True)


def test_rounded_projection_with_an_int64_part_in_the_reference(E):
    """the reference's row sums then come from its int64 matrix; means near 3 * 2^31 round every t at 2^-20"""
    _rounded_projection(E, C.I64_REFERENCE_PROJECT, ref_big=True)


@pytest.mark.parametrize("a", [1, 64, 255])
def test_columns_of_a_cross_strip_are_independent(E, a):
    n_ref, w = 261, 257
    co = C.rounded_project_cohort(n_ref, w)
    ref = E.PcoaEngine(n_ref)
    ref.load_gram(co.r)
    out = []
    try:
        for (p0, pw) in [(0, w), (0, a), (a, w - a)]:
            s = np.ascontiguousarray(co.cross()[:n_ref + pw, p0:p0 + pw])     # rows [0, n_ref) + pw rows that are not read
            with _strip_engine(E, n_ref + pw, n_ref, s, False) as cross:
                out.append(ref.project(cross, co.comps(), co.lam))
    finally:
        ref.close()
    assert _same_bytes(out[0], np.concatenate([out[1], out[2]]))

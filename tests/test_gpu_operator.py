"""GPU tests of the implicit similarity operator (pcoa_create_operator): the products S v = X^T (X v) and the row sums are
exact integers wherever the inputs are, the centred product stays inside its summation bound, results are bit-identical run
to run and across call sizes, computePca over the operator gives the full engine's components, and what the operator cannot
serve says so and leaves the ctx usable.  The spec the products are held to is the numpy statement in test_operator_cpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, align_sign, golden_cases, int_gram, load_golden, load_oracle, load_pkg, planted_callsets, \
    write_golden_plink, write_golden_vcf
from test_operator_cpu import spec_centring, spec_matvec, spec_row_sums, unpack_bits

pytestmark = pytest.mark.gpu

SEGMENT_KNOB = "PCOA_OPERATOR_SEGMENT_ROWS"


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def ingest():
    return load_pkg("ingest")


def store_bytes(n, variants, segment_rows=None):
    """What pcoa_operator_info reports (include/pcoa.h): whole segments of ~256 MiB -- whole multiples of 2,048 rows where a
    segment holds that many -- of rows at a pitch of ceil(N / 32) words rounded up to 4."""
    pitch = ((n + 31) // 32 + 3) // 4 * 4
    rows = max(1, (256 << 20) // (pitch * 4))
    if rows >= 2048:
        rows -= rows % 2048
    if segment_rows:
        rows = segment_rows
    return -(-variants // rows) * rows * pitch * 4


def random_x(rng, n, v):
    """0/1 rows of mixed density with an all-zero row and a sample nobody carries in between."""
    x = (rng.random((v, n)) < rng.uniform(0.05, 0.6, size=(v, 1))).astype(np.float32)
    if v >= 3:
        x[v // 2] = 0
    if n >= 34:
        x[:, 33] = 0
    return x


def with_garbage(rng, bits, n, extra_words):
    """The same bitsets with random bits in the samples >= N of the last word and in `extra_words` more words per row."""
    w = bits.shape[1]
    out = rng.integers(0, 2 ** 32, size=(bits.shape[0], w + extra_words), dtype=np.uint64).astype(np.uint32)
    out[:, :w] = bits
    if n & 31:
        out[:, w - 1] |= rng.integers(0, 2 ** 32, size=bits.shape[0], dtype=np.uint64).astype(np.uint32) & np.uint32(
            (0xffffffff << (n & 31)) & 0xffffffff)
    return out


def feed(eng, bits, form, rng):
    """The four input forms: 0 host rows in one call, 1 host rows with garbage handed over in ragged calls with an empty call
    in between, 2 device rows with garbage in one call, 3 device rows in ragged calls."""
    import torch
    n, v = eng.n, bits.shape[0]
    if form in (1, 2):
        bits = with_garbage(rng, bits, n, 3 if form == 1 else 1)
    cuts = [0, v]
    if form in (1, 3) and v > 1:
        cuts = sorted(set([0, v] + [int(c) for c in rng.integers(1, v, size=min(3, v - 1))]))
    for a, b in zip(cuts[:-1], cuts[1:]):
        rows = np.ascontiguousarray(bits[a:b])
        if form >= 2:
            eng.accumulate_bits(torch.from_numpy(rows.view(np.int32)).cuda())
        else:
            eng.accumulate_bits(rows)
            eng.accumulate_bits(rows[:0])           # an empty call adds nothing
    eng.sync()


def product(eng, v, centred=False):
    import torch
    return eng.operator_matvec_device(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda(), centred).cpu().numpy()


# ---- exactness --------------------------------------------------------------------------------------------------------------
# N: the issue's list, then the kernels' constants minus one, exact, plus one: a wave's chunk of 64 word columns (2,048
# samples) and a pass-1 workgroup's group of 256 (8,192 samples).  V: the issue's list, then (at N = 2,504) a butterfly block of
# 32 rows, the 512 rows of a pass-1 workgroup and of a pass-2 range, and the 2,048 rows segments are whole multiples of, each
# minus one, exact, plus one.
SHAPES_N = [32, 33, 63, 64, 65, 2047, 2048, 2049, 2504, 4100, 8191, 8192, 8193]
SHAPES_V = [1, 31, 64, 65, 1000]
EXTRA_V = [32, 33, 511, 512, 513, 2047, 2048, 2049]


@pytest.mark.parametrize("n", SHAPES_N)
def test_integer_products_and_row_sums_are_exact_in_every_input_form(P, ingest, n):
    """v drawn from the integers in [-8, 8]: every partial sum of either pass is an integer far below 2^53, so y must equal
    int_gram(X) @ v bit for bit whatever the summation order; the row sums are int_gram(X).sum(1)."""
    rng = np.random.default_rng(1000 + n)
    vs = [65] if n > 4100 else SHAPES_V + (EXTRA_V if n == 2504 else [])
    with P.PcoaEngine(n, operator=True) as eng:
        assert eng.operator_info() == (0, 0)
        for nv in vs:
            x = random_x(rng, n, nv)
            s = int_gram(x)
            bits = ingest.pack_bits(x)
            v = rng.integers(-8, 9, size=n).astype(np.float64)
            want, want_rs = s.astype(np.float64) @ v, s.sum(axis=1)
            for form in range(4):
                eng.reset()
                feed(eng, bits, form, rng)
                assert eng.operator_info() == (nv, store_bytes(n, nv)), (nv, form)
                assert np.array_equal(product(eng, v), want), (nv, form)
                assert np.array_equal(eng.operator_row_sums(), want_rs), (nv, form)
        eng.reset()
        assert eng.operator_info()[0] == 0 and not product(eng, v).any()


def test_a_call_larger_than_the_staging_ring_row_cap(P):
    """V = 2^17 + 1 host rows at N = 2,504: one call, more rows than a slot of the host staging ring takes.  S v is stated
    through the spec's operator form here (int_gram of 131,073 rows is a 1.6-TFLOP fp64 product on the CPU); the two are the same
    exact integers, which test_operator_cpu.py asserts where S can be formed."""
    n, nv = 2504, (1 << 17) + 1
    rng = np.random.default_rng(17)
    w = (n + 31) // 32
    bits = (rng.integers(0, 2 ** 32, size=(nv, w), dtype=np.uint64) & rng.integers(0, 2 ** 32, size=(nv, w), dtype=np.uint64)).astype(np.uint32)
    x = unpack_bits(bits, n)                      # (the bits of samples >= N in the last word are garbage to the engine)
    v = rng.integers(-8, 9, size=n).astype(np.float64)
    with P.PcoaEngine(n, operator=True) as eng:
        eng.accumulate_bits(bits)
        assert eng.operator_info() == (nv, store_bytes(n, nv))
        assert np.array_equal(product(eng, v), spec_matvec(x, v, block=8192))
        assert np.array_equal(eng.operator_row_sums(), spec_row_sums(x))


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(tests)r)
from conftest import int_gram, load_pkg
import torch
P, ingest = load_pkg(), load_pkg("ingest")
rng = np.random.default_rng(96)
n, nv = 130, 1000
x = (rng.random((nv, n)) < 0.3).astype(np.float32)
s = int_gram(x)
bits = ingest.pack_bits(x)
v = rng.integers(-8, 9, size=n).astype(np.float64)
with P.PcoaEngine(n, operator=True) as eng:
    for r0 in range(0, nv, 250):
        eng.accumulate_bits(bits[r0:r0 + 250])
    assert eng.operator_info() == (nv, 11 * 96 * 8 * 4), eng.operator_info()      # 11 segments of 96 rows of 8 words
    y = eng.operator_matvec_device(torch.from_numpy(v).cuda(), False).cpu().numpy()
    assert np.array_equal(y, s.astype(np.float64) @ v)
    assert np.array_equal(eng.operator_row_sums(), s.sum(axis=1))
    comps, lam, nz = eng.compute(2)
    with P.PcoaEngine(n) as full:
        full.accumulate_bits(bits)
        cf, lf, nzf = full.compute(2)
    assert nz == nzf and np.max(np.abs(lam - lf) / np.abs(lf)) < 1e-6
    eng.reset()
    assert eng.operator_info() == (0, 96 * 8 * 4)
print("SEGMENTS-OK")
"""


def test_products_across_segment_boundaries():
    """1,000 rows in calls of 250 at N = 130 with segments of 96 rows (the knob is read once per process: a fresh child)."""
    env = dict(os.environ)
    env[SEGMENT_KNOB] = "96"
    res = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests")}], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0 and "SEGMENTS-OK" in res.stdout, res.stdout[-3000:]


def golden_bits(ingest, g):
    n = int(g["n_samples"])
    offs, idx = g["row_offsets"], g["sample_idx"]
    x = np.zeros((len(offs) - 1, n), dtype=np.float32)
    for k in range(len(offs) - 1):
        x[k, idx[offs[k]:offs[k + 1]]] = 1
    return n, x, ingest.pack_bits(x)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("name", golden_cases())
def test_plink_rows_give_the_products_of_the_goldens_bitsets(P, ingest, name, flip, tmp_path):
    import torch
    g = load_golden(name)
    n, x, bits = golden_bits(ingest, g)
    prefix = str(tmp_path / name)
    write_golden_plink(g, prefix, flip=flip)
    raw = np.fromfile(prefix + ".bed", dtype=np.uint8)[3:].reshape(-1, (n + 3) // 4)
    rng = np.random.default_rng(5)
    v = rng.integers(-8, 9, size=n).astype(np.float64)
    with P.PcoaEngine(n, operator=True) as ref:
        ref.accumulate_bits(bits)
        want = product(ref, v)
        want_rs = ref.operator_row_sums()
    assert np.array_equal(want, int_gram(x).astype(np.float64) @ v)
    pinned = torch.from_numpy(raw.copy()).pin_memory()
    for how in ("host", "device", "async"):
        with P.PcoaEngine(n, operator=True) as eng:
            if how == "host":
                eng.accumulate_plink_bed(raw, ref_is_a1=flip)
            elif how == "device":
                eng.accumulate_plink_bed(torch.from_numpy(raw.copy()).cuda(), ref_is_a1=flip)
            else:
                eng.accumulate_plink_bed(pinned, ref_is_a1=flip, asynchronous=True)
            eng.sync()
            assert eng.operator_info()[0] == raw.shape[0]
            assert np.array_equal(product(eng, v), want), how
            assert np.array_equal(eng.operator_row_sums(), want_rs), how


# ---- centring, determinism --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nv", [(65, 31), (2504, 3000), (4100, 513)])
def test_centred_product_stays_inside_its_summation_bound(P, ingest, n, nv):
    """centred = 1 against numpy's B @ v, B the oracle's centring of int_gram(X).  The terms the kernels add into y_i are
    sum_j S(i, j) v_j (N additions inside a row of pass 1, V across the rows of pass 2), m_i (1^T v), m^T v and mm (1^T v),
    with 1^T v and m^T v sums of N terms themselves: the worst-case summation bound over exactly those terms is
    (N + V + 8) 2^-52 ((|S| |v|)_i + |m_i| ||v||_1 + |m|^T |v| + |mm| ||v||_1), and |m_i| ||v||_1 + |m|^T |v| <=
    2 max|m| ||v||_1 (the 8 covers the roundings of m, mm and of the three combining operations; 2^-52 is twice the unit
    roundoff, which leaves the reference's own B @ v the same bound again)."""
    oracle = load_oracle()
    rng = np.random.default_rng(n)
    x = planted_callsets(rng, n, nv)
    s = int_gram(x)
    b = oracle.center_matrix(s)[0]
    m, mm = spec_centring(s.sum(axis=1))
    with P.PcoaEngine(n, operator=True) as eng:
        eng.accumulate_bits(ingest.pack_bits(x))
        for trial in range(3):
            v = rng.standard_normal(n) * (10.0 ** rng.integers(-3, 4))
            y = product(eng, v, centred=True)
            bound = (n + nv + 8) * 2.0 ** -52 * (np.abs(s) @ np.abs(v) + (2 * np.abs(m).max() + abs(mm)) * np.abs(v).sum())
            err = np.abs(y - b @ v)
            print("N=%d V=%d max err / bound = %.3g" % (n, nv, float((err / bound).max())))
            assert np.all(err <= bound)
            # the uncentred product of a real vector, against the spec, by the bound of its own terms
            y0 = product(eng, v)
            assert np.all(np.abs(y0 - spec_matvec(x, v)) <= (n + nv) * 2.0 ** -52 * (np.abs(s) @ np.abs(v)))


def test_products_are_bit_identical_run_to_run_and_across_call_sizes(P, ingest):
    rng = np.random.default_rng(31)
    n, nv = 2504, 5000                     # ten pass-2 ranges, two chunks of samples
    x = planted_callsets(rng, n, nv)
    bits = ingest.pack_bits(x)
    v = rng.standard_normal(n)
    with P.PcoaEngine(n, operator=True) as a, P.PcoaEngine(n, operator=True) as b:
        a.accumulate_bits(bits)
        for r0, r1 in ((0, 1), (1, 700), (700, 701), (701, 4097), (4097, nv)):
            b.accumulate_bits(bits[r0:r1])
        for centred in (False, True):
            y1, y2, y3 = product(a, v, centred), product(a, v, centred), product(b, v, centred)
            assert y1.tobytes() == y2.tobytes() == y3.tobytes()
        ca, cb = a.compute(2), b.compute(2)
        assert ca[0].tobytes() == cb[0].tobytes() and ca[1].tobytes() == cb[1].tobytes()


# ---- spectra ----------------------------------------------------------------------------------------------------------------
def check_spectrum(P, n, x, bits, eig=None, k=2):
    oracle = load_oracle()
    with P.PcoaEngine(n) as full:
        full.accumulate_bits(bits)
        comps_f, lam_f, nz_f = full.compute(k)
    with P.PcoaEngine(n, operator=True, eig=eig) as eng:
        eng.accumulate_bits(bits)
        comps, lam, nz = eng.compute(k)
        t = eng.timings()
    s = int_gram(x)
    assert nz == nz_f == int((s.sum(axis=1) > 0).sum())
    if n < 32:        # the temporary full engine: the full engine's result exactly
        assert comps.tobytes() == comps_f.tobytes() and lam.tobytes() == lam_f.tobytes()
        return
    assert t["operator_products"] > 0 and t["operator_store_bytes"] > 0 and t["eig_method"] == 1
    assert np.max(np.abs(lam - lam_f) / np.abs(lam_f)) < 1e-6
    assert np.abs(align_sign(comps, comps_f) - comps_f).max() < 1e-6
    b = oracle.center_matrix(s)[0]
    for c in range(k):
        assert abs(np.linalg.norm(comps[:, c]) - 1) < 1e-12
        assert np.linalg.norm(b @ comps[:, c] - lam[c] * comps[:, c]) <= 1e-9 * abs(lam[c])
    for c in range(k):
        for d in range(c):
            assert abs(comps[:, c] @ comps[:, d]) < 1e-10


@pytest.mark.parametrize("name", golden_cases())
def test_goldens_give_the_full_engines_components(P, ingest, name):
    n, x, bits = golden_bits(ingest, load_golden(name))
    check_spectrum(P, n, x, bits, k=min(2, n))


@pytest.mark.parametrize("n,eig", [(130, None), (260, None), (2504, None), (260, "band")])
def test_planted_cohorts_give_the_full_engines_components(P, ingest, n, eig):
    rng = np.random.default_rng(300 + n)
    x = planted_callsets(rng, n, 3000)
    x[:, 7] = 0                              # a sample nobody carries: a zero row of S
    check_spectrum(P, n, x, ingest.pack_bits(x), eig=eig)


def test_a_cohort_whose_similarity_matrix_would_not_fit(P):
    """N = 300,000: S would be 360 GB; 1,024 planted rows are 38 MB of bits.  The residual of the returned pairs is checked
    in numpy through the operator form on the packed bits: no N x N array exists anywhere."""
    E = load_pkg("engine")
    n, nv, k = 300000, 1024, 2
    rng = np.random.default_rng(3)
    pops = np.minimum((np.arange(n) * 3) // n, 2)
    which = rng.integers(0, 4, size=nv)
    thr = np.where(which[:, None] == pops[None, :], np.uint8(128), np.uint8(13))       # carrier probability 0.5 inside, 0.05 outside
    thr[which == 3] = 50
    x = (rng.integers(0, 256, size=(nv, n), dtype=np.uint8) < thr).astype(np.uint8)
    del thr
    bits = np.packbits(x, axis=1, bitorder="little").view("<u4")
    assert bits.shape == (nv, n // 32)
    free0 = E.device_memory(0)[0]
    with P.PcoaEngine(n, operator=True) as eng:
        eng.accumulate_bits(bits)
        comps, lam, nz = eng.compute(k)
        used = free0 - E.device_memory(0)[0]
        rs = eng.operator_row_sums()
    print("HBM in use beside the store's owner: %.2f GB" % (used / 1e9))
    assert used < 4e9
    want_rs = spec_row_sums(x, block=128)
    assert np.array_equal(rs, want_rs) and nz == int((want_rs > 0).sum())
    m, mm = spec_centring(want_rs)
    for c in range(k):
        u = comps[:, c]
        su = u.sum()
        bu = ((spec_matvec(x, u, block=64) - m * su) - m @ u) + mm * su
        assert abs(np.linalg.norm(u) - 1) < 1e-12
        assert np.linalg.norm(bu - lam[c] * u) <= 1e-9 * abs(lam[c])
    assert abs(comps[:, 0] @ comps[:, 1]) < 1e-10 and lam[0] > lam[1] > 0


# ---- state ------------------------------------------------------------------------------------------------------------------
def test_what_an_operator_cannot_serve_says_so_and_leaves_it_usable(P, ingest):
    import ctypes
    import torch
    L = load_pkg("_lib")
    rng = np.random.default_rng(9)
    n = 260
    x = planted_callsets(rng, n, 2000)
    bits = ingest.pack_bits(x)
    with P.PcoaEngine(n, operator=True) as eng, P.PcoaEngine(n) as full, P.PcoaEngine(n, strip=(0, n)) as strip:
        eng.accumulate_bits(bits)
        before = eng.compute(2)
        lib, ctx = eng._lib, eng._ctx
        buf = np.zeros((n, n), dtype=np.int64)
        dev = torch.zeros(n * n, dtype=torch.int64, device="cuda")
        p, dp = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(dev.data_ptr())
        f64 = np.zeros((n, n), dtype=np.float64)
        pf = ctypes.c_void_p(f64.ctypes.data)
        owners = (ctypes.c_void_p * 1)(ctx.value)
        refused = {
            "gram_read_i64": lambda: lib.pcoa_gram_read_i64(ctx, p),
            "gram_read_block_i64": lambda: lib.pcoa_gram_read_block_i64(ctx, 0, 0, 4, 4, p),
            "gram_load_i64": lambda: lib.pcoa_gram_load_i64(ctx, p),
            "gram_export": lambda: lib.pcoa_gram_export_device_i64(ctx, dp),
            "gram_import": lambda: lib.pcoa_gram_import_device_i64(ctx, dp),
            "reduce_from (dst)": lambda: lib.pcoa_gram_reduce_from(ctx, full._ctx),
            "allreduce": lambda: lib.pcoa_gram_allreduce_rccl(ctx, ctypes.c_void_p(1)),
            "center_read": lambda: lib.pcoa_center_read_f64(ctx, pf, None, None, None),
            "project (ref)": lambda: lib.pcoa_project(ctx, strip._ctx, 2, pf, pf, pf),
            "compute_strips": lambda: lib.pcoa_compute_strips(owners, 1, 2, pf, pf, None),
            "strip_col_sums": lambda: lib.pcoa_strip_col_sums(ctx, pf),
            "dense_f32": lambda: lib.pcoa_accumulate_dense_f32(ctx, pf, 1, n, 0),
            "dense_u8": lambda: lib.pcoa_accumulate_dense_u8(ctx, pf, 1, n, 0),
            "calls": lambda: lib.pcoa_accumulate_calls(ctx, p, p, 1),
        }
        for what, call in refused.items():
            lib.pcoa_accumulate_bits(ctx, None, -1, 0, 0)          # leaves another message behind: the next one must be the call's own
            assert call() == L.PCOA_ERR_STATE, what
            msg = lib.pcoa_last_error(ctx).decode()
            assert msg and "n_variants" not in msg, what
            if what in ("dense_f32", "dense_u8", "calls"):
                assert "pcoa_accumulate_bits" in msg             # names the bitset boundary
        # the other side of the two-engine calls: reported on the engine that was asked
        assert lib.pcoa_gram_reduce_from(full._ctx, ctx) == L.PCOA_ERR_STATE and lib.pcoa_last_error(full._ctx)
        full.accumulate_bits(bits)
        cf, lf, _ = full.compute(2)
        assert lib.pcoa_project(full._ctx, ctx, 2, pf, pf, pf) == L.PCOA_ERR_STATE and lib.pcoa_last_error(full._ctx)
        # an ordinary engine is not an operator
        assert full.operator_info() is None
        assert lib.pcoa_operator_row_sums(full._ctx, p) == L.PCOA_ERR_STATE
        assert lib.pcoa_operator_matvec_device(full._ctx, dp, dp, 0) == L.PCOA_ERR_STATE
        # finalize and sync work, and the ctx still computes the same components
        eng.finalize()
        eng.sync()
        after = eng.compute(2)
        assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes() and after[2] == before[2]
        assert np.abs(align_sign(after[0], cf) - cf).max() < 1e-6
        eng.reset()
        assert eng.operator_info()[0] == 0
        eng.reserve(0, 2)
        eng.accumulate_bits(bits[:1000])
        assert eng.operator_info()[0] == 1000
        assert np.array_equal(eng.operator_row_sums(), int_gram(x[:1000]).sum(axis=1))
    with pytest.raises(P.PcoaError) as ei:
        P.PcoaEngine(64, operator=True, eig="householder")
    assert ei.value.code == L.PCOA_ERR_INVALID_ARG
    with P.PcoaEngine(16, operator=True, eig="householder") as small:     # below the Lanczos path the dense solver is the only one
        small.accumulate_bits(ingest.pack_bits(x[:, :16]))
        assert small.compute(2)[0].shape == (16, 2)


# ---- hosts ------------------------------------------------------------------------------------------------------------------
def host_rows(res):
    assert res.returncode == 0, res.stderr[-2000:]
    rows = [ln.split("\t") for ln in res.stdout.splitlines() if ln.count("\t") == 3]
    return [(r[0], r[1]) for r in rows], np.array([[float(r[2]), float(r[3])] for r in rows])


@pytest.mark.parametrize("kind,name", [("vcf", "tile130"), ("plink", "tile260")])
def test_both_hosts_give_the_stored_forms_coordinates(kind, name, tmp_path):
    """--gram implicit against --gram stored of the same host: the same sample names, order and datasets, coordinates within
    1e-6 (not byte-identical: the additions differ)."""
    from test_operator_cpu import _run_driver, _run_python
    g = load_golden(name)
    if kind == "vcf":
        path = str(tmp_path / (name + ".vcf"))
        write_golden_vcf(g, path)
    else:
        write_golden_plink(g, str(tmp_path / name))
        path = str(tmp_path / name) + ".bed"
    for run in (_run_driver, _run_python):
        stored = run(["--input-path", path, "--gram", "stored"])
        implicit = run(["--input-path", path, "--gram", "implicit"])
        ids_s, xy_s = host_rows(stored)
        ids_i, xy_i = host_rows(implicit)
        assert len(ids_s) == int(g["n_samples"]) and ids_i == ids_s
        assert np.abs(xy_i - xy_s).max() < 1e-6
        assert "Implicit similarity operator" in implicit.stderr and "Implicit similarity operator" not in stored.stderr
        for line in ("Matrix size: %d." % int(g["n_samples"]), "Non zero rows in matrix:"):       # the milestone lines
            assert line in implicit.stdout and line in stored.stdout

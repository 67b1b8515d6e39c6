"""The staging ring of the host boundaries (StagingRing, csrc/pcoa_ctx.h; capi_accumulate.hip: staging_acquire) at the
smallest shapes that make a slot WRAP inside one call and GROW while it is marked used: two slots per ring, a slot is
rewritten or regrown only after the kernels that read it last, and a host input is consumed when its copy is done.  A ring
that frees or rewrites a slot early gives wrong counts here (a fault under PCOA_DEBUG_GUARD=1).  Counts are integers: every
comparison is exact."""
import numpy as np
import pytest

from conftest import int_gram, load_oracle, load_pkg

pytestmark = pytest.mark.gpu

SLOT_ROWS = 1 << 17     # rows of a bitset / .bed staging slot
CSR_ROWS = 1 << 20      # rows of a carrier-list chunk (one operand buffer)


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def O():
    return load_oracle()


def test_bitset_and_bed_rows_share_one_ring_that_wraps_and_regrows(P):
    """N = 70 (3 words per bitset row, 18 bytes per .bed row), on one engine: host bitsets at the dense stride in three
    chunks (slot 0 is reused inside the call), then .bed rows whose chunk of 2^17 x 18 B does not fit the 2^17 x 12 B the
    slots hold (both slots regrow while marked used), then bitsets at ld_words = 5 with garbage in the padding words (the 2-D
    copy).  Both reference-allele conventions, one engine each."""
    ingest = load_pkg("ingest")
    rng = np.random.default_rng(70)
    n, bpv = 70, 18
    x1 = rng.random((2 * SLOT_ROWS + 4097, n)) < 0.1
    x3 = rng.random((SLOT_ROWS + 1, n)) < 0.1
    # .bed codes: 2 = heterozygous (a carrier either way), 0 / 3 = homozygous A1 / A2 (a carrier when the OTHER allele is the
    # reference), 1 = missing; the two codes of padding in the last byte are anything
    codes = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), size=(SLOT_ROWS + 5, bpv * 4), p=[0.05, 0.85, 0.05, 0.05])
    quad = codes.reshape(-1, bpv, 4)
    raw = np.ascontiguousarray(quad[:, :, 0] | (quad[:, :, 1] << 2) | (quad[:, :, 2] << 4) | (quad[:, :, 3] << 6))
    b1 = ingest.pack_bits(x1)
    b3 = np.array(ingest.pack_bits(x3, pad_words=2))
    b3[:, 3:] = 0xa5a5a5a5
    assert b1.shape[1] == 3 and raw.shape[1] == bpv and b3.shape[1] == 5
    g13 = int_gram(x1) + int_gram(x3)
    for ref_a1 in (False, True):
        carrier = (codes[:, :n] == 2) | (codes[:, :n] == (3 if ref_a1 else 0))
        with P.PcoaEngine(n) as eng:
            eng.accumulate_bits(b1)
            eng.accumulate_plink_bed(raw, ref_is_a1=ref_a1)
            eng.accumulate_bits(b3)
            got = eng.gram()
        assert np.array_equal(got, g13 + int_gram(carrier))


def test_threshold_slots_regrow_while_marked_used(P, O):
    """pcoa_accumulate_synthetic, N = 260, 7 populations, calls of 100, 200, 20000, 30, 50000 variants: slot 0 holds 2^16 words
    after the first call and must grow at the third (140,000 words) and at the fifth (350,000), each time as a used slot."""
    synth = load_pkg("synth")
    n, n_pops, calls, seed = 260, 7, (100, 200, 20000, 30, 50000), 260
    offs = synth.pop_offsets(n, sizes=np.linspace(1.0, 2.0, n_pops))
    thr = synth.thresholds(seed, 0, sum(calls), n_pops=n_pops)
    want = O.similarity_from_dense(synth.genotypes(seed, 0, thr, offs), n)
    with P.PcoaEngine(n) as eng:
        v0 = 0
        for c in calls:
            eng.accumulate_synthetic(seed, offs, thr[v0:v0 + c], v0)
            v0 += c
        got = eng.gram()
        t = eng.timings()
    assert t["pack_launches"] == 0      # the thresholds went through the slots (no staging tile, no pre-pass)
    assert np.array_equal(got, want)


def test_carrier_list_slots_regrow_while_marked_used(P):
    """N = 64, pageable arrays, 2 * 2^20 + 300,000 variants in one call: the rows of the first two chunks carry one callset
    each, the rows of the third six distinct ones -- 1.8 M entries against the 1.18 M slot 0 holds from the first chunk, so
    the index buffer and its page-locked twin grow on a used slot.  Equal to the same arrays handed over as device tensors
    (no slot) and to the integer Gram."""
    import torch
    rng = np.random.default_rng(64)
    n, v_one, v_six = 64, 2 * CSR_ROWS, 300000
    one = rng.integers(0, n, size=v_one, dtype=np.int32)
    base = rng.integers(0, n, size=(v_six, 1))
    step = 2 * rng.integers(0, n // 2, size=(v_six, 1)) + 1      # odd: base + k * step are distinct mod 64 for k < 6
    six = ((base + np.arange(6) * step) % n).astype(np.int32)
    idx = np.concatenate([one, six.reshape(-1)])
    offs = np.concatenate([np.arange(v_one, dtype=np.int64), v_one + 6 * np.arange(v_six + 1, dtype=np.int64)])
    x6 = np.zeros((v_six, n), dtype=np.float32)
    np.put_along_axis(x6, six, 1.0, axis=1)
    assert int(x6.sum()) == 6 * v_six
    want = int_gram(x6) + np.diag(np.bincount(one, minlength=n)).astype(np.int64)
    with P.PcoaEngine(n) as eng:
        eng.accumulate_calls(idx, offs)
        got = eng.gram()
        t = eng.timings()
    assert t["csr_fast_chunks"] >= 3 and t["csr_redo_chunks"] == 0
    assert np.array_equal(got, want)
    with P.PcoaEngine(n) as eng:
        eng.accumulate_calls_tensors(torch.from_numpy(idx).cuda(), torch.from_numpy(offs).cuda())
        assert np.array_equal(eng.gram(), got)

"""Every launch form of the k-bits contraction held to an exact Gram, at the sample counts where the dispatch changes form.

fp4_setup / fp4_launch (operand.hip) pick the contraction's launch from the padded sample count: beside the next pre-pass
(co-resident pipeline) the 224-VGPR gram_kbits_kernel as an even split (mode 4), lock-step with split-K 8 / 4 / 2 / 1
(mode 2) or banded split-K (mode 0); alone on the chip (tail generation, finalize, serial bitsets) the one-wave-per-SIMD
kernel as an even split or banded.  On 256 CUs ("Launch bands"):

    N <= 1024                  no pipeline                   alone: even split
    1025 .. 11264 otherwise    beside: even split            alone: even split
    1537-1792 / 2305-2560 /    beside: lock-step, split-K    alone: even split
    3329-3840 / 4865-5632      8 / 4 / 2 / 1
    11265 .. 16384             beside: banded                alone: banded
    >= 16385                   no pipeline                   alone: banded

Each case takes V = 3 M + 777 variants with operand buffers of M variants (PCOA_DEBUG_MAX_LAUNCH): three generations
contracted beside the pre-pass of the next one, then a ragged tail generation contracted alone.  Inputs from a seed on the
device: fp32 tiles with a 16-byte row pitch (ring pre-pass, pipelined) and an odd one (ordinary pre-pass, serial), NaN in
the padding; a uint8 tile with 0xff padding; carrier bitsets with set bits beyond N; and an fp32 job whose second generation
alone holds carrier multiplicities (its FP4 contraction is skipped on the device, its chunks are redone on the int8 kernel).
Reference: X^T X in float64 on the device -- exact, every sum is an integer far below 2^53 -- held itself to int64 host
products on a few blocks.  S is compared in full (both triangles after finalize), and the launch counters must show the form
the band names: a threshold that moves fails here by name instead of dropping coverage.

The knobs are read once per process, so every environment runs in a child process of its own, which takes all sample
counts of that environment in turn (process start-up is most of a small case's time) and reports one JSON line per case.
"""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from conftest import load_pkg  # noqa: E402

pytestmark = pytest.mark.gpu

NUM_CU = 256
TJ = 256                      # sample tile of the contraction
M = 4608                      # variants per operand-buffer generation: 144 k-blocks, 36 stages of 128 variants
TAIL = 777                    # ragged tail generation (28 k-blocks, zero-padded to 48)
V = 3 * M + TAIL
CALL = M // 2                 # skip-flag job: two calls (= two pre-pass chunks) per generation

# N -> (band, mode beside the pre-pass (None: no pipeline), mode alone, lock-step split-K)
BANDS = {}
for _n in (1024,):
    BANDS[_n] = ("N <= 1024: no pipeline, even split alone", None, 4, None)
for _n in (1025, 1536, 1793, 2304, 2561, 3328, 3841, 4864, 5633, 11264):
    BANDS[_n] = ("1025-11264 outside the lock-step bands: even split beside the pre-pass", 4, 4, None)
for _n, _k in ((1537, 8), (1792, 8), (2305, 4), (2560, 4), (3329, 2), (3840, 2), (4865, 1), (5632, 1)):
    BANDS[_n] = ("lock-step split-K %d beside the pre-pass" % _k, 2, 4, _k)
for _n in (11265, 16383, 16384):
    BANDS[_n] = ("11265-16384: banded split-K beside the pre-pass", 0, 0, None)
for _n in (16385,):
    BANDS[_n] = ("N >= 16385: no pipeline, banded alone", None, 0, None)

HOST_BLOCK_N = 11265          # where the float64 reference is itself held to int64 host products
FOLD_THRESHOLD = 6000         # > M, < 2 M: an int32 -> int64 fold in front of the 2nd and 3rd generation

# environment -> (sample counts, inputs, knobs, child time limit in seconds: ~10x what an idle MI355X takes)
ENVS = {
    "default": (sorted(BANDS), ("f32", "f32_odd", "u8", "bits", "f32_mult"), {}, 180),
    "bits_pipeline": ((2305, 5633, 11265), ("bits",), {"PCOA_BITS_PIPELINE": "1"}, 60),
    "fold": ((11265, 16385), ("f32", "u8", "f32_mult"), {"PCOA_DEBUG_FOLD_THRESHOLD": str(FOLD_THRESHOLD)}, 60),
}


def ntri(n):
    t = (n + TJ - 1) // TJ
    return t * (t + 1) // 2


# --------------------------------------------------------------------------------------------------------- child process
def _genotypes(torch, n, v, seed):
    """Binary [v][n] uint8 on the device: per-variant carrier frequency p^2 (many rare variants, some common), the last
    sample a carrier of every third variant, and the first and last variant of every generation carried by everyone: a
    launch that drops or repeats a stage at a generation or k-segment edge moves every entry of S."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    p = torch.rand((v, 1), generator=g, device="cuda") ** 2
    x = (torch.rand((v, n), generator=g, device="cuda") < p).to(torch.uint8)
    x[::3, n - 1] = 1
    for r in sorted({0, M - 1, M, 2 * M - 1, 2 * M, 3 * M - 1, 3 * M, v - 1}):
        x[r] = 1
    x[7] = 0
    return x


def _gram64(torch, x):
    """X^T X as int64 through a float64 matmul (exact: integers below 2^53)."""
    xd = x.to(torch.float64)
    assert float(xd.max()) ** 2 * xd.shape[0] < 2.0 ** 53
    return (xd.t() @ xd).to(torch.int64)


def _compare(torch, eng, want):
    """S (exported on the device, both triangles) against the reference; the first mismatch with its 256 x 256 tile."""
    s = torch.empty_like(want)
    eng.export_device(s.data_ptr())
    eng.sync()
    torch.cuda.synchronize()
    bad = s != want
    nbad = int(bad.sum())
    if nbad == 0:
        return {"exact": True}
    n = want.shape[0]
    i, j = divmod(int(bad.view(-1).to(torch.uint8).argmax()), n)
    nt = (n + TJ - 1) // TJ
    per_tile = torch.nn.functional.pad(bad.to(torch.uint8), (0, nt * TJ - n, 0, nt * TJ - n)).view(nt, TJ, nt, TJ).any(3).any(1)
    tiles = per_tile.nonzero()[:12].tolist()
    return {"exact": False, "mismatches": nbad, "first": [i, j], "first_tile": [i // TJ, j // TJ],
            "got": int(s[i, j]), "want": int(want[i, j]), "tiles": tiles}


def _counters(eng):
    t = eng.timings()
    keys = ("gram_kernel_launches", "lockstep_launches", "evensplit_launches", "pipeline_launches", "pipeline_pre_pass_cus",
            "pipeline_contraction_cus", "fp4_fallbacks", "gram_variants", "gram_kernel_kind", "gram_i64_live")
    return dict((k, int(t[k])) for k in keys)


def _bits_of(torch, x, n):
    """Carrier bitsets [v][words + 1] (int32 words): bits of samples >= N set, and a whole padding word of ones."""
    v = x.shape[0]
    words = (n + 31) // 32
    bits = torch.full((v, words + 1), -1, dtype=torch.int32, device="cuda")
    shifts = torch.arange(32, device="cuda", dtype=torch.int32)
    for r0 in range(0, v, 4096):
        r1 = min(v, r0 + 4096)
        xb = torch.nn.functional.pad(x[r0:r1], (0, words * 32 - n), value=1).view(r1 - r0, words, 32)
        # int32 arithmetic wraps: bit 31 contributes -2^31, which is the two's-complement word wanted
        bits[r0:r1, :words] = (xb.to(torch.int32) << shifts).sum(dim=2, dtype=torch.int32)
    return bits


def _f32_tile(torch, x, ld):
    v, n = x.shape
    t = torch.full((v, ld), float("nan"), dtype=torch.float32, device="cuda")
    t[:, :n] = x
    return t[:, :n]


def _run_one(P, torch, np, n, kinds):
    x = _genotypes(torch, n, V, 7919 * n + 11)
    want = _gram64(torch, x)
    out = {"n": n}
    if n == HOST_BLOCK_N:
        # the float64 reference against int64 host products: diagonal blocks at both ends (the last one ragged), a block
        # straddling a tile edge, an off-diagonal block of the lower triangle
        xh = x.cpu().numpy().astype(np.int64)
        ok = True
        for r0, c0 in ((0, 0), (n - 64, n - 64), (TJ - 32, 5 * TJ - 32), (n - 64, 0)):
            blk = xh[:, r0:r0 + 64].T @ xh[:, c0:c0 + 64]
            ok = ok and bool(np.array_equal(blk, want[r0:r0 + 64, c0:c0 + 64].cpu().numpy()))
        out["host_blocks_exact"] = ok
        del xh
    ld4 = (n + 3) // 4 * 4 + 4                       # 16-byte rows: the ring pre-pass (pack_fp4_ring_ok)
    ld_odd = n + 3 if (n + 3) % 2 else n + 4          # odd pitch: the ordinary pre-pass, fp32 tiles stay serial
    for kind in kinds:
        if kind in ("f32", "f32_odd"):
            inp = _f32_tile(torch, x, ld4 if kind == "f32" else ld_odd)
        elif kind == "u8":
            ld8 = (n + 8) // 8 * 8                        # >= 1 byte of padding, 8-byte rows (pack_u8_ring_ok)
            buf = torch.full((V, ld8), 0xFF, dtype=torch.uint8, device="cuda")
            buf[:, :n] = x
            inp = buf[:, :n]
        elif kind == "bits":
            inp = _bits_of(torch, x, n)
        else:  # f32_mult: carrier multiplicities 2..127 in the second generation only
            g = torch.Generator(device="cuda")
            g.manual_seed(n)
            y = x[M:2 * M].to(torch.int32)
            hit = (torch.rand(y.shape, generator=g, device="cuda") < 1.0 / 64) & (y > 0)
            y = torch.where(hit, torch.randint(2, 128, y.shape, generator=g, device="cuda", dtype=torch.int32), y)
            xm = x.clone()
            xm[M:2 * M] = y.to(torch.uint8)
            want_m = _gram64(torch, xm)
            inp = _f32_tile(torch, xm, ld4)
            del y, hit
        torch.cuda.synchronize()
        with P.PcoaEngine(n) as eng:
            if kind == "f32_mult":
                for v0 in range(0, V, CALL):
                    eng.accumulate_dense(inp[v0:v0 + CALL])
            elif kind == "u8":
                eng.accumulate_dense_u8(inp)
            elif kind == "bits":
                eng.accumulate_bits(inp)
            else:
                eng.accumulate_dense(inp)
            res = _compare(torch, eng, want_m if kind == "f32_mult" else want)
            res.update(_counters(eng))
        out[kind] = res
        del inp
        if kind == "f32_mult":
            del want_m, xm
        torch.cuda.empty_cache()
    return out


def child_main(argv):
    import numpy as np
    import torch
    ns = [int(a) for a in argv[0].split(",")]
    kinds = argv[1].split(",")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != NUM_CU:
        print(json.dumps({"skip": "the launch bands are laid out for %d CUs; this device reports %d (a partitioned mode?)"
                                  % (NUM_CU, cus)}))
        return
    P = load_pkg()
    for n in ns:
        print(json.dumps(_run_one(P, torch, np, n, kinds)))
        sys.stdout.flush()


# --------------------------------------------------------------------------------------------------------- parent
_RUNS = {}
_FAULTED = []


def _run_env(name):
    """One child per environment, once per session, never retried.  After a child that died of a signal or ran out of time
    nothing more is started on the GPU from this module."""
    if name in _RUNS:
        return _RUNS[name]
    ns, kinds, knobs, limit = ENVS[name]
    if _FAULTED:
        pytest.fail("not started: an earlier child of this module ended abnormally (%s)" % _FAULTED[0])
    env = dict(os.environ, PCOA_DEBUG_MAX_LAUNCH=str(M), **knobs)
    cmd = [sys.executable, os.path.abspath(__file__), ",".join(str(n) for n in ns), ",".join(kinds)]
    try:
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env,
                             timeout=limit)
    except subprocess.TimeoutExpired as e:
        _FAULTED.append("%s: time limit %d s" % (name, limit))
        _RUNS[name] = {"error": "child exceeded its time limit of %d s; stdout so far:\n%s" % (limit, e.stdout)}
        return _RUNS[name]
    lines = [json.loads(s) for s in res.stdout.splitlines() if s.startswith("{")]
    run = {"cases": dict((d["n"], d) for d in lines if "n" in d)}
    if any("skip" in d for d in lines):
        run["skip"] = [d["skip"] for d in lines if "skip" in d][0]
    if res.returncode != 0:
        if res.returncode < 0 or res.returncode in (134, 139):
            _FAULTED.append("%s: exit status %d" % (name, res.returncode))
        run["error"] = "child exited with status %d\n%s" % (res.returncode, res.stderr[-4000:])
    _RUNS[name] = run
    return run


def _case(env_name, n):
    run = _run_env(env_name)
    if "skip" in run:
        pytest.skip(run["skip"])
    assert "error" not in run, run["error"]
    assert n in run["cases"], "no result for N = %d" % n
    return run["cases"][n]


def _check_exact(n, kind, r):
    assert r["exact"], "N = %d, %s: S differs from X^T X in %d entries; first (%d, %d) = %d, want %d, tile %s; tiles %s" % (
        n, kind, r["mismatches"], r["first"][0], r["first"][1], r["got"], r["want"], r["first_tile"], r["tiles"])


def _check_form(n, kind, r, side_launches, fp4_launches, int8_launches=0):
    """The launch counters of one input against the form its band names.  side_launches: contractions queued beside the
    next pre-pass (0 where the input or the band has no pipeline); fp4_launches: every FP4 contraction, skipped ones
    included; int8_launches: contractions on the int8 kernel (gram_kernel_launches counts both)."""
    band, side_mode, alone_mode, splitk = BANDS[n]
    where = "N = %d, %s, band '%s': %s" % (n, kind, band, r)
    side = side_launches if side_mode is not None else 0
    alone = fp4_launches - side
    assert r["pipeline_launches"] == side, where
    modes = [side_mode] * side + [alone_mode] * alone
    assert r["lockstep_launches"] == modes.count(2), where
    assert r["evensplit_launches"] == modes.count(4), where
    assert r["gram_kernel_launches"] == fp4_launches + int8_launches, where
    banded = r["gram_kernel_launches"] - int8_launches - r["lockstep_launches"] - r["evensplit_launches"]
    assert banded == modes.count(0), where
    if side_mode is None:
        assert r["pipeline_pre_pass_cus"] == 0, where
    else:   # co-resident: the ring pre-pass has waves on every CU, the contraction shares them
        assert r["pipeline_pre_pass_cus"] + r["pipeline_contraction_cus"] > NUM_CU, where
        if side_mode == 2:   # lock-step: one workgroup per (tile, k-segment)
            assert r["pipeline_contraction_cus"] == ntri(n) * splitk, where


GENS = 4    # three full generations and the tail


def _mult_launches(n):
    """(FP4, int8) contractions of the skip-flag job.  With two operand buffers (every band but the last) the flagged
    generation is resolved when its buffer is needed again, at the tail's pre-pass: its two chunks are redone on int8 and
    the tail stays on FP4.  With one buffer (N >= 16385: banded, no pipeline, no lock-step) it is resolved as soon as it
    is launched, at the first chunk of generation 3; the auto mode then keeps the next chunks -- the rest of generation 3
    and the tail -- on int8 as well (i8_streak), so generation 3 is contracted on FP4 with one chunk."""
    if BANDS[n][1] is None and BANDS[n][2] == 0:
        return GENS - 1, M // CALL + 2
    return GENS, M // CALL


@pytest.mark.parametrize("n", sorted(BANDS))
def test_every_launch_band_exact_on_fp32_uint8_and_bitset_tiles(n):
    c = _case("default", n)
    print("N = %d (%s):" % (n, BANDS[n][0]))
    for kind in ("f32", "f32_odd", "u8", "bits"):
        r = c[kind]
        _check_exact(n, kind, r)
        assert r["gram_variants"] == V and r["fp4_fallbacks"] == 0 and r["gram_kernel_kind"] == 3, (n, kind, r)
        # pipelined: the 16-byte-pitch fp32 tile and the uint8 tile; serial: an fp32 tile the ring cannot read, and
        # bitsets (unless PCOA_BITS_PIPELINE=1)
        _check_form(n, kind, r, GENS - 1 if kind in ("f32", "u8") else 0, GENS)
        print("  %-8s S exact; launches %d (lock-step %d, even split %d, beside the pre-pass %d)" % (
            kind, r["gram_kernel_launches"], r["lockstep_launches"], r["evensplit_launches"], r["pipeline_launches"]))
    if n == HOST_BLOCK_N:
        assert c["host_blocks_exact"], "the float64 reference differs from int64 host products"


@pytest.mark.parametrize("n", sorted(BANDS))
def test_skip_flag_of_a_generation_with_multiplicities_in_every_band(n):
    """Only the second generation holds multiplicities: its (pipelined, where the band has a pipeline) FP4 contraction is
    skipped by the device-side flag and its two pre-pass chunks are redone on the int8 kernel; every other generation stays
    on the FP4 kernel in the band's form."""
    r = _case("default", n)["f32_mult"]
    _check_exact(n, "f32_mult", r)
    assert r["fp4_fallbacks"] == M // CALL, (n, r)
    assert r["gram_variants"] == V, (n, r)
    _check_form(n, "f32_mult", r, GENS - 1, *_mult_launches(n))
    print("N = %d (%s): S exact; %d chunks redone on int8" % (n, BANDS[n][0], r["fp4_fallbacks"]))


@pytest.mark.parametrize("n", ENVS["bits_pipeline"][0])
def test_bitsets_through_the_co_resident_pipeline(n):
    """PCOA_BITS_PIPELINE=1: the bitset transpose beside the contraction, which takes the whole-chip form (even split or
    banded, never lock-step: fp4_launch side_kind 3)."""
    r = _case("bits_pipeline", n)["bits"]
    _check_exact(n, "bits", r)
    assert r["fp4_fallbacks"] == 0 and r["gram_variants"] == V, (n, r)
    mode = 0 if n >= 11265 else 4
    assert r["pipeline_launches"] == GENS - 1, (n, r)
    assert r["lockstep_launches"] == 0 and r["evensplit_launches"] == (GENS if mode == 4 else 0), (n, r)
    assert r["gram_kernel_launches"] == GENS, (n, r)
    print("N = %d: bitsets co-resident, S exact; even split %d, beside the pre-pass %d" % (
        n, r["evensplit_launches"], r["pipeline_launches"]))


@pytest.mark.parametrize("n", ENVS["fold"][0])
def test_int64_fold_between_generations(n):
    """PCOA_DEBUG_FOLD_THRESHOLD between one and two generations: the int32 partial is folded into int64 in front of the
    second and third contraction (waiting for the one beside the pre-pass), and S = int64 part + int32 partial."""
    c = _case("fold", n)
    for kind in ENVS["fold"][1]:
        r = c[kind]
        _check_exact(n, kind, r)
        assert r["gram_i64_live"] == 1, (n, kind, r)
        assert r["gram_variants"] == V, (n, kind, r)
        _check_form(n, kind, r, GENS - 1, *(_mult_launches(n) if kind == "f32_mult" else (GENS,)))
    assert c["f32_mult"]["fp4_fallbacks"] == M // CALL
    print("N = %d: S exact across int64 folds (%s)" % (n, ", ".join(ENVS["fold"][1])))


if __name__ == "__main__":
    child_main(sys.argv[1:])

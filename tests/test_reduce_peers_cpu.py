"""CPU tests of the peer reduction over k engines (pcoa_gram_reduce_peers, --reduce scatter): the entry point is declared,
exported, bound and refuses, before any device work, what it cannot take; the chunk partition tiles S in whole 16-byte quads;
the compiled host knows the fourth --reduce value; and the chunk kernel keeps its source table out of scratch."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import subset_cohort as C
from conftest import ROOT, load_golden, load_pkg, write_golden_vcf


def test_pcoa_gram_reduce_peers_is_declared_exported_and_bound():
    L = load_pkg("_lib")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcoa.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+pcoa_gram_reduce_peers\s*\(\s*pcoa_ctx\s*\*\s*const\s*\*\s*ctxs\s*,\s*int32_t\s+k\s*,"
                     r"\s*int32_t\s+root_only\s*\)\s*;", header)
    assert re.search(r"#define\s+PCOA_REDUCE_MAX_ENGINES\s+16\b", header) and L.PCOA_REDUCE_MAX_ENGINES == 16
    for name in ("pcoa_gram_reduce_peers", "pcoa_get_reduce_peers_stats", "pcoa_debug_reduce_chunk"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(L.load(), name)
    pkg = load_pkg()
    assert callable(pkg.reduce_peers) and pkg.reduce_peers is load_pkg("engine").reduce_peers
    # the three counters, in the order of the header's struct
    assert [f[0] for f in L.PcoaReducePeersStats._fields_] == ["reduce_peers_calls", "reduce_peers_seconds", "reduce_peers_bytes_in"]
    assert re.search(r"reduce_peers_calls;.*?reduce_peers_seconds;.*?reduce_peers_bytes_in;.*?}\s*pcoa_reduce_peers_stats\s*;",
                     header, flags=re.S)


def test_pcoa_gram_reduce_peers_refuses_bad_arguments_before_any_device_work():
    L = load_pkg("_lib")
    lib = L.load()
    nulls = (ctypes.c_void_p * 17)()
    for ctxs, k in ((None, 2), (nulls, 0), (nulls, -3), (nulls, 17), (nulls, 1), (nulls, 3)):
        lib.pcoa_create(None, 0, 0, 0)                               # leaves another message in the NULL ctx's slot
        assert b"pcoa_gram_reduce_peers" not in lib.pcoa_last_error(None)
        assert lib.pcoa_gram_reduce_peers(ctxs, k, 0) == L.PCOA_ERR_INVALID_ARG, k
        assert b"pcoa_gram_reduce_peers" in lib.pcoa_last_error(None), k
    assert lib.pcoa_gram_reduce_peers(nulls, 3, 1) == L.PCOA_ERR_INVALID_ARG
    assert b"ctxs[0] is NULL" in lib.pcoa_last_error(None)
    with pytest.raises(ValueError):
        load_pkg().reduce_peers([])


def _chunks(lib, n, k):
    out = []
    for g in range(k):
        first, count = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert lib.pcoa_debug_reduce_chunk(g, k, n, ctypes.byref(first), ctypes.byref(count)) == 0
        out.append((first.value, count.value))
    return out


@pytest.mark.parametrize("n", [1, 2, 5, 33, 130, 301])
@pytest.mark.parametrize("k", [1, 2, 3, 8, 16])
def test_the_chunks_tile_s_in_whole_quads(n, k):
    """The library's own reduce_chunk against the formula of pcoa.h: with Q = ceil(N^2 / 4), owner g takes the quads
    [g Q / k, (g + 1) Q / k); the last owner's chunk ends with the N^2 % 4 tail elements."""
    lib = load_pkg("_lib").load()
    nn = n * n
    q = (nn + 3) // 4
    got = _chunks(lib, n, k)
    want = [(4 * (g * q // k), min(4 * ((g + 1) * q // k), nn) - 4 * (g * q // k)) for g in range(k)]
    assert got == want
    pos = 0
    for first, count in got:                                         # they tile [0, N^2) exactly, in owner order
        assert first == pos and count >= 0 and first % 4 == 0
        pos += count
    assert pos == nn
    quads = [(c + 3) // 4 for _, c in got]
    assert max(quads) - min(quads) <= 1                              # at most one quad apart ...
    assert all(c % 4 == 0 for _, c in got[:-1]) and got[-1][1] % 4 == nn % 4   # ... and only the last owner holds the tail
    if q < k:
        assert any(c == 0 for _, c in got)                           # N = 5, k = 8: Q = 7 < k leaves an owner nothing


def test_the_partition_hook_refuses_what_lies_outside_it():
    L = load_pkg("_lib")
    lib = L.load()
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    for g, k, n in ((0, 0, 5), (0, 17, 5), (3, 3, 5), (-1, 3, 5), (0, 3, 0)):
        assert lib.pcoa_debug_reduce_chunk(g, k, n, ctypes.byref(a), ctypes.byref(b)) == L.PCOA_ERR_INVALID_ARG
    assert lib.pcoa_debug_reduce_chunk(0, 3, 5, None, ctypes.byref(b)) == L.PCOA_ERR_INVALID_ARG
    # 46,341^2 > 2^31: the arithmetic is 64-bit
    got = _chunks(lib, 100000, 8)
    assert sum(c for _, c in got) == 10 ** 10 and got[7][0] == 8750000000


@pytest.fixture(scope="module")
def kat5_vcf(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("reducecli") / "kat5.vcf")
    write_golden_vcf(load_golden("kat5"), path)
    return path


def test_driver_refuses_an_unknown_reduce_value_and_names_all_four(kat5_vcf):
    res = C.run_driver(["--input-path", kat5_vcf, "--reduce", "bogus"])
    assert res.returncode != 0 and "--reduce takes auto, rccl, peer or scatter" in res.stderr, res.stderr
    assert "Matrix size" not in res.stdout and "pcoa_create" not in res.stderr
    usage = subprocess.run([C.driver_exe(), "--help"], stdout=subprocess.PIPE, universal_newlines=True).stdout
    assert "--reduce auto|rccl|peer|scatter" in usage


@pytest.mark.parametrize("extra", [["--gpus", "1"], ["--gpus", "2", "--gpu-map", "0,0", "--layout", "strips"]])
def test_driver_accepts_reduce_scatter_in_the_argument_check(kat5_vcf, extra):
    """--parse-only: ingest and getCallsRdd without a GPU, behind the argument check.  With --layout strips there is no
    reduction step and the value is accepted and ignored, as peer is."""
    res = C.run_driver(["--input-path", kat5_vcf, "--reduce", "scatter", "--parse-only"] + extra)
    assert res.returncode == 0, res.stderr
    assert "--reduce takes" not in res.stderr
    peer = C.run_driver(["--input-path", kat5_vcf, "--reduce", "peer", "--parse-only"] + extra)
    assert "Matrix size" in res.stdout
    strip_times = lambda s: re.sub(r"[0-9.]+ s\b|(read|split|parse) [0-9.]+", "", s)      # noqa: E731  (wall times differ run to run)
    assert peer.returncode == 0 and strip_times(peer.stdout) == strip_times(res.stdout)


def test_reduce_chunk_kernels_do_not_spill_to_scratch():
    """reduce_peers.hip takes the table of up to 16 source matrices by value and indexes it by unrolled constants only; a
    run-time index would send it to scratch.  hipcc reports at compile time whether any of it went there."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"      # (what built the library; without it this test fails)
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                              "-I", csrc, "-c", os.path.join(csrc, "reduce_peers.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True)
    assert res.returncode == 0, res.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", res.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res.stdout)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", res.stdout)]
    # <int32_t, false>, <int64_t, true>, <int64_t, false>
    assert len(names) == len(scratch) == 3 and all("reduce_chunk_kernel" in nm for nm in names), names
    assert sorted(re.search(r"reduce_chunk_kernelI(\w)Lb(\d)E", nm).groups() for nm in names) == [("i", "0"), ("l", "0"), ("l", "1")]
    assert scratch == [0, 0, 0] and lds == [0, 0, 0]

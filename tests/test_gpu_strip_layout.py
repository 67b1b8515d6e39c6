"""GPU tests of the strip layout end to end in one process: `--layout strips` of the compiled host (owners sharing
device 0) on every golden and ingest road, pcoa_compute_strips against the torch-driven strips.compute_pca_over_strips
at N = 100,000, its argument checks, and the byte cap of the host-bitset staging at N = 250,000."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, align_sign, golden_cases, load_golden, load_oracle, load_pkg, write_golden_plink, write_golden_vcf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return load_pkg()


@pytest.fixture(scope="module")
def E():
    return load_pkg("engine")


def _exe():
    exe = os.path.join(ROOT, "spark-examples_amd", "variants_pca_driver")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "spark-examples_amd", "host")])
    return exe


def _run(args, n, tmp_path, tag):
    dump = str(tmp_path / ("s_%s.bin" % tag))
    out = str(tmp_path / ("o_%s" % tag))
    res = subprocess.run([_exe()] + args + ["--dump-similarity", dump, "--output-path", out], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert res.returncode == 0, (tag, res.stderr[-3000:])
    with open(out + "-pca.tsv", "rb") as f:
        tsv = f.read()
    return np.fromfile(dump, dtype="<i8").reshape(n, n), tsv, res


def _pcs(tsv):
    rows = [l.split(b"\t") for l in tsv.splitlines()]
    return [r[0] for r in rows], np.array([[float(r[1]), float(r[2])] for r in rows])


@pytest.mark.parametrize("name", golden_cases())
def test_goldens_through_the_strip_layout_match_the_reference_matrix_and_the_single_engine(name, tmp_path):
    g = load_golden(name)
    n = int(g["n_samples"])
    plink = str(tmp_path / "p")
    write_golden_plink(g, plink)
    vcf = str(tmp_path / "g.vcf")
    write_golden_vcf(g, vcf)
    s1, tsv1, r1 = _run(["--input-path", plink + ".bed"], n, tmp_path, "one")
    assert np.array_equal(s1, g["similarity"]) and "strip layout" not in r1.stderr     # auto = full here
    _, tsv1_vcf, _ = _run(["--input-path", vcf], n, tmp_path, "one_vcf")           # (the dataset column is the file's stem)
    nz1 = [l for l in r1.stdout.splitlines() if l.startswith("Non zero rows")]
    names1, pc1 = _pcs(tsv1)
    # the oracle-centred golden: is the top-2 eigen-gap wide enough to compare PCs entry by entry?
    b = load_oracle().center_matrix(g["similarity"])[0]
    lam = np.sort(np.linalg.eigvalsh(b))[::-1]
    scale = max(abs(lam[0]), 1e-300)
    separated = abs(lam[0] - lam[1]) >= 1e-6 * scale and (n < 3 or abs(lam[1] - lam[2]) >= 1e-6 * scale)
    roads = {
        "plink_device": ["--input-path", plink + ".bed", "--stream-rows", "7"],
        "plink_host": ["--input-path", plink + ".bed", "--stream-rows", "5", "--plink-decode", "host"],
        "vcf": ["--input-path", vcf],
        "no_stream": ["--input-path", plink + ".bed", "--no-stream"],
    }
    for k in (1, 2, 3):
        if k > n:
            continue
        for road, args in roads.items():
            tag = "%s_%d" % (road, k)
            s, tsv, res = _run(args + ["--layout", "strips", "--gpus", str(k), "--gpu-map", ",".join(["0"] * k)], n, tmp_path, tag)
            assert np.array_equal(s, g["similarity"]), tag
            assert "strip layout: %d owner(s)" % k in res.stderr, res.stderr
            assert [l for l in res.stdout.splitlines() if l.startswith("Non zero rows")] == nz1, tag
            if n < 32:
                assert tsv == (tsv1_vcf if road == "vcf" else tsv1), tag   # the temporary full engine: byte-identical
                continue
            names, pc = _pcs(tsv)
            assert names == names1, tag
            if separated:
                assert np.abs(align_sign(pc, pc1) - pc1).max() < 1e-9, tag
            # every PC against the oracle-centred matrix by its residual.  Rows are printed sorted by name; the name of
            # callset i is S%04d (write_golden_plink / write_golden_vcf), which maps a printed row back to callset order.
            where = np.array([int(nm[1:]) for nm in names])
            assert sorted(where.tolist()) == list(range(n))
            for c in range(2):
                v = np.zeros(n)
                v[where] = pc[:, c]
                mu = v @ b @ v
                assert np.linalg.norm(b @ v - mu * v) <= 1e-8 * scale, tag


def _planted_strips(P, n, v, ranges, seed):
    synth = load_pkg("synth")
    offs = synth.pop_offsets(n)
    owners = [P.PcoaEngine(n, strip=r) for r in ranges]
    chunk = 16384
    for v0 in range(0, v, chunk):
        thr = synth.thresholds(seed, v0, min(chunk, v - v0))
        for e in owners:
            e.accumulate_synthetic(seed, offs, thr, v0)
    return owners


def test_compute_strips_is_bit_identical_to_the_torch_driven_path_at_n_100000(P, E):
    """Three ragged, non-tile-aligned owners on one device, 2^16 planted variants: pcoa_compute_strips (built-in product,
    pieces written at y + col0) against strips.compute_pca_over_strips (torch device tensors) on the same owners."""
    strips = load_pkg("strips")
    n = 100000
    ranges = [(0, 33333), (33333, 40001), (73334, 26666)]
    owners = _planted_strips(P, n, 65536, ranges, 2026)
    try:
        comps, lam, nz = E.compute_strips(owners, 2)
        rs = np.concatenate([e.strip_col_sums() for e in owners])
        comps_t, lam_t, nz_t = strips.compute_pca_over_strips(owners, 2)
        assert np.array_equal(lam, lam_t) and np.array_equal(comps, comps_t)
        assert nz == nz_t == int((rs > 0).sum())
        assert lam[0] > lam[1] > 0 and abs(np.linalg.norm(comps[:, 0]) - 1) < 1e-12
        # a second call on the same owners gives the same bits (resident means replaced, not accumulated)
        comps2, lam2, _ = E.compute_strips(owners, 2)
        assert np.array_equal(lam2, lam) and np.array_equal(comps2, comps)
    finally:
        for e in owners:
            e.close()


def test_compute_strips_below_32_samples_is_the_single_engine(P, E):
    rng = np.random.default_rng(17)
    n = 20
    calls = [list(np.nonzero(rng.random(n) < 0.3)[0]) for _ in range(60)]
    with P.PcoaEngine(n) as full:
        full.accumulate_callsets(calls)
        want = full.compute(2)
    owners = [P.PcoaEngine(n, strip=r) for r in ((0, 7), (7, 6), (13, 7))]
    try:
        for e in owners:
            e.accumulate_callsets(calls)
        got = E.compute_strips(owners, 2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    finally:
        for e in owners:
            e.close()


def test_compute_strips_rejects_owners_that_do_not_tile(P, E):
    n = 300
    calls = [[1, 2, 250], [5, 299], [0, 100, 200]]
    made = []

    def mk(r, nn=n):
        e = P.PcoaEngine(nn, strip=r)
        e.accumulate_callsets([c for c in calls if max(c) < nn])
        made.append(e)
        return e

    try:
        a, b, c = mk((0, 100)), mk((100, 100)), mk((200, 100))
        assert E.compute_strips([a, b, c], 2)[2] > 0                      # the good tiling works
        gap = mk((210, 90))
        over = mk((90, 110))
        other_n = mk((200, 100), nn=400)
        full = P.PcoaEngine(n)
        made.append(full)
        for bad in ([a, b], [a, b, gap], [a, over, c], [b, a, c], [a, b, full], [a, b, other_n]):
            with pytest.raises(E.PcoaError) as ei:
                E.compute_strips(bad, 2)
            assert ei.value.code == -1, ei.value
    finally:
        for e in made:
            e.close()


def test_host_bitset_staging_is_capped_by_bytes_at_n_250000(P, E):
    """2^17 host bitset rows at N = 250,000 are 4.1 GB: the two staging slots of pcoa_accumulate_bits hold at most
    256 MiB each.  The owner's strip must still equal an independent owner's fed the same rows from device memory."""
    import torch
    n, cols, v = 250000, 31250, 1 << 17
    words = (n + 31) // 32
    rng = np.random.default_rng(250)
    block = rng.integers(0, 2 ** 32, size=(1024, words), dtype=np.uint32)
    block &= rng.integers(0, 2 ** 32, size=(1024, words), dtype=np.uint32)   # ~1/4 density
    block[:, -1] &= np.uint32((1 << (n - 32 * (words - 1))) - 1)            # no bits past sample N - 1
    bits = np.tile(block, (v // 1024, 1))
    a = P.PcoaEngine(n, strip=(0, cols))
    b = P.PcoaEngine(n, strip=(0, cols))
    try:
        dev = torch.from_numpy(bits.view(np.int32)).cuda()
        a.accumulate_bits(dev)        # operand buffers for this chunk size exist before the measured call
        b.accumulate_bits(dev)
        a.sync()
        b.sync()
        del dev
        a._keepalive.clear()
        b._keepalive.clear()
        torch.cuda.empty_cache()
        free0, _ = E.device_memory(0)
        a.accumulate_bits(bits)
        a.sync()
        free1, _ = E.device_memory(0)
        grew = free0 - free1
        # uncapped, the two slots alone are 2 x 4.1 GB; capped they are 2 x 256 MiB, and the call's other first-use device
        # buffers come on top (2.76 GB in all on an MI355X)
        assert grew < (4 << 30), grew
        for (r0, c0) in ((0, 0), (120000, 31000), (249900, 15000), (31000, 31100)):
            want = b.gram_block(r0, c0, 100, min(100, cols - c0))
            assert int(want.sum()) > 0
            assert np.array_equal(a.gram_block(r0, c0, 100, min(100, cols - c0)), 2 * want), (r0, c0)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("name", ["tile260", "pops40"])
def test_python_host_strip_layout_over_two_gloo_ranks_and_one_process(name, tmp_path):
    """variants_pca.py --layout strips: two real ranks sharing cuda:0 over gloo (rank r owns strip_ranges(N, 2)[r], reads
    every variant, the product's pieces travel as host vectors), and one process (pcoa_compute_strips).  Same S as the
    reference, same output as the single engine."""
    import socket
    g = load_golden(name)
    n = int(g["n_samples"])
    path = str(tmp_path / "golden.vcf")
    write_golden_vcf(g, path)
    script = os.path.join(ROOT, "spark-examples_amd", "variants_pca.py")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MASTER_PORT=str(port))
    outs = {}
    runs = (("one", []), ("strips_1", ["--layout", "strips"]),
            ("strips_2", ["--layout", "strips", "--gpus", "2", "--rank-devices", "0,0", "--dist-backend", "gloo"]))
    for tag, extra in runs:
        dump = str(tmp_path / (tag + ".bin"))
        res = subprocess.run([os.sys.executable, script, "--input-path", path, "--all-references", "--dump-similarity", dump] + extra,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env, timeout=600)
        assert res.returncode == 0, res.stderr[-3000:]
        assert np.array_equal(np.fromfile(dump, dtype="<i8").reshape(n, n), g["similarity"]), tag
        assert ("strip layout" in res.stderr) == (tag != "one"), res.stderr[-2000:]
        if tag == "strips_2":
            assert "strip layout: 2 owner(s)" in res.stderr and "Reduced over" not in res.stderr
        outs[tag] = [l for l in res.stdout.splitlines() if "\t" in l or l.startswith(("Matrix size", "Non zero rows"))]
    one = outs["one"]
    assert len(one) == n + 2
    a = np.array([[float(x) for x in l.split("\t")[2:4]] for l in one if "\t" in l])
    for tag in ("strips_1", "strips_2"):
        got = outs[tag]
        assert [l.split("\t")[:2] for l in got] == [l.split("\t")[:2] for l in one], tag   # names, datasets, the two lines
        b = np.array([[float(x) for x in l.split("\t")[2:4]] for l in got if "\t" in l])
        assert np.abs(align_sign(b, a) - a).max() < 1e-9, tag

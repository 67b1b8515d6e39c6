"""CPU tests of the pairwise-complete similarity (pcoa_set_call_companion, --missing-calls): the numpy rule against a plain
double loop, its closed forms, the fixtures the GPU tests rely on (tests/complete_cohort.py asserts their properties at every
shape test_gpu_complete.py uses), the numpy restatement of the pair decode, the CLI surface of both hosts with no engine
attempted, the call-rate file, the header and the binding, and the kernels' resource report."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import complete_cohort as C
from conftest import ROOT, int_gram, load_golden, load_pkg, write_golden_plink, write_golden_vcf


@pytest.fixture(scope="module")
def vp():
    return load_pkg("variants_pca")


# ---- the rule against a double loop ---------------------------------------------------------------------------------------------
def loop_rule(s, q, v):
    n = s.shape[0]
    c = [v - int(q[i, i]) for i in range(n)]
    k = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            m = c[i] + c[j] - v + int(q[i, j])
            k[i, j] = float(int(s[i, j])) / float(m) if m > 0 else 0.0
    return k


def small_cohorts():
    """(name, carriers, missing, V): random cohorts with one sample that has no call at all (index 2) and one called everywhere
    that carries nothing (the last), plus a pair of samples that are never called together (M = 0 off the diagonal)."""
    out = []
    for n, v, seed in ((7, 40, 1), (12, 90, 2), (23, 150, 3)):
        x, m, _ = C.populations_with_missing(n, v, seed=seed, all_missing=(2,), called_empty=(n - 1,))
        m[: v // 2, 0] = True      # sample 0 is called on the second half only, sample 1 on the first half only
        m[v // 2:, 0] = False
        m[: v // 2, 1] = False
        m[v // 2:, 1] = True
        x = x & ~m
        out.append(("pops%d" % n, x, m, v))
    return out


def test_the_rule_against_a_double_loop(vp):
    for name, x, m, v in small_cohorts():
        s, q = int_gram(x), int_gram(m)
        n = s.shape[0]
        k = vp.call_complete_measure(s, q, v)
        assert k.dtype == np.float64 and np.array_equal(k, loop_rule(s, q, v)), name
        assert np.array_equal(k, k.T) and np.abs(k).max() <= 1.0
        assert not k[2].any() and not k[:, 2].any()                               # no call at all: M = 0 against everybody, itself included
        assert not k[n - 1].any()                                                 # called everywhere, carries nothing
        assert k[0, 1] == 0.0 and k[0, 0] > 0 and k[1, 1] > 0                     # never called together: the M > 0 guard
        c = v - np.diagonal(q)
        assert c[2] == 0 and c[n - 1] == v
        b, r, mm, nz = vp.centred_measure(k)
        assert nz == n - 2
        assert np.array_equal(C.measure_longdouble(s, q, v).astype(np.float64), k)    # the long-double rule rounds to the same K
        ref_b = C.reference(s, q, v)[0]
        assert ref_b.dtype == np.longdouble and np.abs(ref_b.astype(np.float64) - b).max() <= C.entry_bound(n)
    with pytest.raises(ValueError):
        vp.call_complete_measure(np.zeros((3, 3)), np.zeros((3, 4)), 5)
    with pytest.raises(ValueError):
        vp.call_complete_measure(np.zeros((2, 2)), np.array([[4, 0], [0, 1]]), 3)     # V below a missing count
    assert vp.MISSING_CALLS == ("ignore", "pairwise")


def test_without_missing_calls_the_rule_is_s_over_v(vp):
    for name, x, m, v in small_cohorts():
        s = int_gram(x)
        k = vp.call_complete_measure(s, np.zeros_like(s), v)
        assert np.array_equal(k, s.astype(np.float64) / float(v)), name


# ---- the fixtures of the GPU tests ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(set(C.EXACT_TILE_N + C.EXACT_ROW_N)))
def test_the_exact_cohort_is_exact(n):
    for extra in C.EXTRAS:
        C.exact_case(n, extra)                                                    # asserts every closed form itself


@pytest.mark.parametrize("n", C.EIG_N + (C.HOST_N,))
def test_the_eigen_cohorts_have_their_gaps(n):
    x, m = C.eig_cohort(n)
    v = x.shape[0]
    lam, z, b, gaps = C.eig_reference(int_gram(x), int_gram(m), v)               # asserts positive leading eigenvalues and the gaps
    print("N = %d: lambda = %s, relative gaps %s" % (n, lam, ["%.3f" % g for g in gaps]))
    rate = m.mean(axis=0)
    assert rate.max() - rate.min() >= 0.2                                         # the call rates do differ


@pytest.mark.parametrize("n", C.ROUNDED_N)
def test_the_rounded_cohorts_keep_k_within_one(vp, n):
    x, m, rate = C.populations_with_missing(n, C.ROUNDED_V, all_missing=(1,), called_empty=(3,))
    s, q = int_gram(x), int_gram(m)
    k = C.measure_longdouble(s, q, C.ROUNDED_V)                                   # asserts s <= M itself
    assert float(np.abs(k).max()) <= 1.0
    assert vp.centred_measure(vp.call_complete_measure(s, q, C.ROUNDED_V))[3] == n - 2 == C.reference(s, q, C.ROUNDED_V)[3]


@pytest.mark.parametrize("n", C.I64_N)
def test_the_int64_cohorts_leave_int32_and_scale_exactly(vp, n):
    x, m, s, q, v = C.i64_cohort(n)                                               # asserts 2^22 S >= 2^31 itself
    k = vp.call_complete_measure(s, q, v)
    scaled = vp.call_complete_measure(s * C.I64_SCALE, q, v)
    assert np.array_equal(scaled, k * float(C.I64_SCALE))                         # a power of two changes no rounding
    b, bs = vp.centred_measure(k), vp.centred_measure(scaled)
    assert np.array_equal(bs[0], b[0] * float(C.I64_SCALE)) and np.array_equal(bs[1], b[1] * float(C.I64_SCALE))


def test_the_call_rate_artefact_the_rule_removes(vp):
    """The reason for the feature, at N = 260: a leading coordinate of the shared counts follows the per-sample missing rate,
    the pairwise-complete rule's does not."""
    n = 260
    x, m, rate = C.populations_with_missing(n, C.ROUNDED_V, seed=1000 + n)
    s, q = int_gram(x), int_gram(m)

    def worst(b):
        w, z = np.linalg.eigh(b)
        lead = z[:, np.argsort(-np.abs(w))[:2]]
        return max(abs(np.corrcoef(lead[:, c], rate)[0, 1]) for c in range(2))

    shared = worst(vp.centred_measure(s.astype(np.float64))[0])
    complete = worst(vp.centred_measure(vp.call_complete_measure(s, q, C.ROUNDED_V))[0])
    print("max |corr| with the missing rate: shared %.3f, pairwise-complete %.3f" % (shared, complete))
    assert complete < 0.1 < shared


# ---- the pair decode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref_is_a1", [False, True])
def test_decode_pair_over_all_four_codes(ref_is_a1):
    rows = np.array([[0b11100100]], dtype=np.uint8)                               # samples 0..3 hold codes 00, 01, 10, 11
    carriers, missing = C.decode_pair(rows, 4, ref_is_a1)
    assert missing.tolist() == [[False, True, False, False]]
    assert carriers.tolist() == [[False, False, True, True]] if ref_is_a1 else carriers.tolist() == [[True, False, True, False]]
    I = load_pkg("ingest")
    for n, v in ((5, 9), (63, 20), (65, 33)):
        rows = C.random_codes(n, v, seed=n)
        nb = (n + 3) // 4
        assert rows.shape == (v, nb)
        if n % 4:
            assert np.all((rows[:, -1] >> (2 * (n % 4))) == (0b01010101 >> (2 * (n % 4))))   # the padding pairs are 01
        carriers, missing = C.decode_pair(rows, n, ref_is_a1)
        assert not (carriers & missing).any()
        # the byte-wise statement: one sample at a time
        for s in (0, n // 2, n - 1):
            code = (rows[:, s // 4] >> (2 * (s % 4))) & 3
            assert np.array_equal(missing[:, s], code == 1)
            assert np.array_equal(carriers[:, s], (code == 2) | (code == (3 if ref_is_a1 else 0)))
        # a fixture built from (carriers, missing) decodes to them again
        again = C.bed_rows(carriers, missing, ref_is_a1=ref_is_a1, row_bytes=nb + 3)
        c2, m2 = C.decode_pair(again, n, ref_is_a1)
        assert np.array_equal(c2, carriers) and np.array_equal(m2, missing)
        assert I.pack_bits(missing).shape == (v, (n + 31) // 32)


def test_the_python_ingest_decodes_carriers_as_the_restatement(tmp_path):
    """ingest.load_plink's carrier bitsets (what --missing-calls ignore feeds) are decode_pair's carriers."""
    I = load_pkg("ingest")
    x, m = C.eig_cohort(C.HOST_N)
    names = [C.name_of(i) for i in range(C.HOST_N)]
    C.write_plink(str(tmp_path / "p" / "cohort"), x, m, names)
    raw = np.fromfile(str(tmp_path / "p" / "cohort.bed"), dtype=np.uint8)[3:].reshape(x.shape[0], -1)
    carriers, missing = C.decode_pair(raw, C.HOST_N)
    assert np.array_equal(carriers, x) and np.array_equal(missing, m)
    got = I.load_plink(str(tmp_path / "p" / "cohort.bed"), None, as_bits=True)
    bits = got[2][0][1]
    assert np.array_equal(bits, I.pack_bits(x))


# ---- the CLI surface of both hosts: no engine attempted -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("completecli")
    g = load_golden("kat5")
    write_golden_vcf(g, str(d / "kat5.vcf"))
    write_golden_plink(g, str(d / "kat5"))
    return {"vcf": str(d / "kat5.vcf"), "bed": str(d / "kat5.bed")}


_ON = ["--missing-calls", "pairwise"]
REFUSED = [
    ("@bed", _ON + ["--gram", "implicit"], "cannot take --gram implicit"),
    ("@bed", _ON + ["--layout", "strips"], "cannot take --layout strips"),
    ("@bed", _ON + ["--layout", "strips", "--gpus", "2"], "cannot take --layout strips"),
    ("@bed", _ON + ["--gpus", "2"], "cannot take --gpus 2"),
    ("@vcf", _ON + ["--project-input-path", "@vcf"], "cannot take --project-input-path"),
    ("@bed", _ON + ["--similarity-measure", "jaccard"], "cannot take --similarity-measure jaccard"),
    ("@bed", _ON + ["--similarity-measure", "cosine"], "cannot take --similarity-measure cosine"),
    ("@bed", _ON + ["--ld-window", "50"], "cannot take --ld-window"),
    ("@bed", _ON + ["--loadings-output-path", "@out"], "cannot take --loadings-output-path"),
    ("@vcf", _ON, "must name a single .bed / .bim / .fam"),
    ("@bed", ["--missing-calls", "drop"], "takes ignore or pairwise"),
    ("@bed", ["--missing-calls", "Pairwise"], "takes ignore or pairwise"),
    ("@bed", ["--missing-calls", ""], "takes ignore or pairwise"),
    ("@bed", ["--call-rate-output-path", "@out"], "--call-rate-output-path needs --missing-calls pairwise"),
    ("@bed", ["--missing-calls", "ignore", "--call-rate-output-path", "@out"], "--call-rate-output-path needs --missing-calls pairwise"),
]


def _args(inputs, path, extra, tmp):
    sub = {"@vcf": inputs["vcf"], "@bed": inputs["bed"], "@out": os.path.join(tmp, "never.tsv")}
    return ["--input-path", sub[path]] + [sub.get(a, a) for a in extra]


@pytest.mark.parametrize("path,extra,what", REFUSED)
def test_driver_refuses_what_the_rule_cannot_serve(inputs, path, extra, what, tmp_path):
    res = C.run_driver(_args(inputs, path, extra, str(tmp_path)))
    assert res.returncode != 0 and "--missing-calls" in res.stderr and what in res.stderr, res.stderr
    assert "Matrix size" not in res.stdout and "pcoa_create" not in res.stderr       # no file was read, no engine attempted
    assert not os.path.exists(str(tmp_path / "never.tsv"))


@pytest.mark.parametrize("path,extra,what", REFUSED)
def test_python_host_refuses_what_the_rule_cannot_serve(vp, inputs, path, extra, what, capsys, tmp_path):
    """(In process: the refusals come from check_missing_conf, which main runs before it reads a file.)"""
    with pytest.raises(SystemExit) as ei:
        vp.main(_args(inputs, path, extra, str(tmp_path)))
    assert "--missing-calls" in str(ei.value) and what in str(ei.value), str(ei.value)
    assert "Matrix size" not in capsys.readouterr().out
    assert not os.path.exists(str(tmp_path / "never.tsv"))


def test_both_hosts_say_the_same_refusal(vp, inputs, tmp_path):
    for path, extra, _ in REFUSED:
        args = _args(inputs, path, extra, str(tmp_path))
        res = C.run_driver(args)
        with pytest.raises(SystemExit) as ei:
            vp.main(args)
        assert res.stderr.strip() == str(ei.value), (res.stderr, str(ei.value))


def test_the_compiled_host_keeps_the_streamed_device_decode(inputs):
    for extra, what in ((["--no-stream"], "cannot take --no-stream"), (["--parse-only"], "cannot take --parse-only"),
                        (["--plink-decode", "host"], "cannot take --plink-decode host")):
        res = C.run_driver(["--input-path", inputs["bed"]] + _ON + extra)
        assert res.returncode != 0 and "--missing-calls pairwise" in res.stderr and what in res.stderr, res.stderr
        assert "pcoa_create" not in res.stderr


def test_ignore_is_the_default_and_refuses_nothing(vp):
    conf = vp.PcaConf([])
    assert conf.missing_calls == "ignore" and conf.call_rate_output_path is None
    vp.check_missing_conf(conf)
    vp.check_missing_conf(vp.PcaConf(["--missing-calls", "ignore", "--gram", "implicit", "--similarity-measure", "jaccard"]))
    conf = vp.PcaConf(["--input-path", "x.bed", "--missing-calls", "pairwise", "--outlier-iterations", "2", "--related-min-jaccard", "0.4",
                       "--remove-related", "--call-rate-output-path", "r.tsv"])
    vp.check_missing_conf(conf)                                                   # composes with the subset features
    vp.check_outlier_conf(conf)
    vp.check_related_conf(conf)
    for other in ("x.bim", "x.fam"):
        vp.check_missing_conf(vp.PcaConf(["--input-path", other, "--missing-calls", "pairwise"]))
    with pytest.raises(SystemExit):
        vp.check_missing_conf(vp.PcaConf(["--input-path", "a.bed", "b.bed", "--missing-calls", "pairwise"]))
    with pytest.raises(SystemExit):
        vp.check_missing_conf(vp.PcaConf(["--input-path", "a.bed", "--min-allele-frequency", "0.1", "--missing-calls", "pairwise"]))


def test_usage_strings(vp, capsys):
    usage = subprocess.run([C.driver_exe(), "--help"], stdout=subprocess.PIPE, universal_newlines=True).stdout
    assert "--missing-calls ignore|pairwise [--call-rate-output-path FILE]" in usage
    assert "--similarity-measure shared|jaccard|cosine" in usage                  # (the measure's line is what it was)
    with pytest.raises(SystemExit) as ei:
        vp.PcaConf(["--help"])
    out = capsys.readouterr().out
    assert ei.value.code == 0 and "--missing-calls" in out and "--call-rate-output-path" in out and "ignore|pairwise" in out


# ---- the call-rate file ---------------------------------------------------------------------------------------------------------
def test_call_rate_file_format(vp, tmp_path):
    names = ["A", "B b", "C"]
    path = str(tmp_path / "rates.tsv")
    vp.write_call_rates(path, names, np.array([7, 0, 3]), 7)
    assert open(path).read() == "A\t7\t7\t1.000000\nB b\t0\t7\t0.000000\nC\t3\t7\t0.428571\n"
    vp.write_call_rates(path, names[:1], np.array([0]), 0)
    assert open(path).read() == "A\t0\t0\t0.000000\n"
    missing = np.array([[0, 1, 0], [0, 1, 1], [0, 1, 1], [0, 1, 0], [0, 1, 1], [0, 1, 1], [0, 1, 0]], dtype=bool)
    vp.write_call_rates(path, names, 7 - missing.sum(axis=0), 7)
    assert open(path).read().splitlines() == C.call_rate_lines(names, missing)


# ---- header and binding ---------------------------------------------------------------------------------------------------------
def test_the_calls_are_declared_exported_and_bound():
    L = load_pkg("_lib")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcoa.h")).read(), flags=re.S)
    ws = r"\s*"
    protos = {
        "pcoa_set_call_companion": r"\bint\s+pcoa_set_call_companion\s*\(\s*pcoa_ctx\s*\*\s*ctx\s*,\s*pcoa_ctx\s*\*\s*missing\s*,\s*int64_t\s+n_variants\s*\)\s*;",
        "pcoa_get_call_companion": r"\bint\s+pcoa_get_call_companion\s*\(\s*const\s+pcoa_ctx\s*\*\s*ctx\s*,\s*pcoa_ctx\s*\*\s*\*\s*missing_out\s*,\s*int64_t\s*\*\s*n_variants_out\s*\)\s*;",
        "pcoa_accumulate_plink_bed_calls": r"\bint\s+pcoa_accumulate_plink_bed_calls\s*\(\s*pcoa_ctx\s*\*\s*ctx\s*,\s*pcoa_ctx\s*\*\s*missing\s*,\s*const\s+uint8_t\s*\*\s*bed_rows\s*,\s*"
                                           r"int64_t\s+n_variants\s*,\s*int64_t\s+row_bytes\s*,\s*int\s+ref_is_a1\s*,\s*int\s+is_device_ptr\s*\)\s*;",
    }
    assert ws
    lib = L.load()
    sig = dict((s[0], s) for s in L._SIGNATURES)
    for name, proto in protos.items():
        assert re.search(proto, header), name
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    vp_, i64 = ctypes.c_void_p, ctypes.c_int64
    assert sig["pcoa_set_call_companion"][2] == [vp_, vp_, i64]
    assert sig["pcoa_get_call_companion"][2] == [vp_, ctypes.POINTER(vp_), ctypes.POINTER(i64)]
    assert sig["pcoa_accumulate_plink_bed_calls"][2] == [vp_, vp_, vp_, i64, i64, ctypes.c_int, ctypes.c_int]
    E = load_pkg().PcoaEngine
    for method in ("set_call_companion", "get_call_companion", "accumulate_plink_bed_calls"):
        assert hasattr(E, method)
    full = open(os.path.join(ROOT, "include", "pcoa.h")).read()
    doc = full[full.index("the pairwise-complete similarity: S normalised"):full.index("int pcoa_set_call_companion")]
    assert "Extends:" in doc and "VariantsPca.scala:56-60" in doc and "VariantsPca.scala:198-231" in doc
    assert "NOT positive semi-definite" in doc and "|lambda|" in doc
    # the similarity binding keeps exactly three kinds
    assert not re.search(r"#define\s+PCOA_SIMILARITY_\w+\s+3\b", header)


def test_the_null_ctx_is_refused_without_a_device():
    L = load_pkg("_lib")
    lib = L.load()
    assert lib.pcoa_set_call_companion(None, None, 0) == L.PCOA_ERR_INVALID_ARG
    assert b"pcoa_set_call_companion" in lib.pcoa_last_error(None)
    out, v = ctypes.c_void_p(5), ctypes.c_int64(7)
    assert lib.pcoa_get_call_companion(None, ctypes.byref(out), ctypes.byref(v)) == L.PCOA_ERR_INVALID_ARG
    assert out.value == 5 and v.value == 7 and b"pcoa_get_call_companion" in lib.pcoa_last_error(None)


# ---- the kernels: no scratch, resources recorded --------------------------------------------------------------------------------
KERNELS = (("plink_bed_to_bits_pair_kernel", 1), ("complete_diag_kernel", 1), ("complete_fill_kernel", 1),
           ("complete_symv_rows_kernel", 4), ("complete_symv_sym_tiles_kernel", 2), ("complete_center_kernel", 1))
RECORD = os.path.join(ROOT, "profiles", "r15a_complete_kernel_resources.txt")
FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", r"ScratchSize \[bytes/lane\]", r"Occupancy \[waves/SIMD\]", r"LDS Size \[bytes/block\]")


@pytest.fixture(scope="module")
def resource_report():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"      # (what built the library; without it these tests fail)
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                              "-I", csrc, "-c", os.path.join(csrc, "complete.hip"), "-o", os.path.join(td, "x.o"),
                              "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True)
    assert res.returncode == 0, res.stdout[-2000:]
    return res.stdout


def _resources(text):
    """{kernel: {field: value}} from the compiler's remarks or from the record (the same lines without the remark's prefix)."""
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        for f in FIELDS:
            m = re.search(f + r": (\d+)", line)
            if m and name:
                out[name][f] = int(m.group(1))
    return out


def test_complete_kernels_do_not_spill_to_scratch(resource_report):
    """complete.hip keeps a lane's eight c_j, the column sums and two rows of EACH matrix in registers; hipcc reports at compile
    time whether any of it went to scratch."""
    names = re.findall(r"Function Name: (\S+)", resource_report)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", resource_report)]
    # decode, diagonal, fill, dense centring; the row form x (int64 part or not) x (centred or not); the tile form x (centred or not)
    assert len(names) == len(scratch) == 10
    for kernel, count in KERNELS:
        assert sum(kernel in nm for nm in names) == count, names
    assert scratch == [0] * 10


def test_the_resource_record_is_current(resource_report):
    now = _resources(resource_report)
    recorded = _resources(open(RECORD).read())
    assert len(now) == 10 and all(len(v) == len(FIELDS) for v in now.values())
    assert recorded == now, "profiles/r15a_complete_kernel_resources.txt is not what hipcc reports for complete.hip today"


def test_measure_unit_and_the_similarity_kinds_are_what_they_were():
    """The new kernels live in a unit of their own: measure.hip has no kernel of this family, and the kinds stay three."""
    csrc = os.path.join(ROOT, "spark-examples_amd", "csrc")
    measure = open(os.path.join(csrc, "measure.hip")).read()
    assert "complete_" not in measure and "comp_q32" not in measure
    assert load_pkg().PcoaEngine.SIMILARITY_KINDS == {"shared": 0, "jaccard": 1, "cosine": 2}

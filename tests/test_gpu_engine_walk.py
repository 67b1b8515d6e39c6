"""GPU walks over a carrier-count engine: an engine is taken through the scripts of tests/engine_walk.py --
appends in every input form, resets, loads within and beyond int32, exports and imports, reductions, subsets, measures,
companions -- and at every observer it is held to three things.
(a) A TWIN: a fresh engine with the walk's create flags, brought to the model's state by load_gram, set_similarity and, where
bound, a fresh companion loaded with Q and bound with V.  Everything a full engine returns is documented to be a function of
exactly that and the call's arguments, so walk and twin must agree byte for byte; no tolerance.
(b) The REPRESENTATION: gram_i64_live of walk and twin are equal, and 1 exactly when the model's S has an entry beyond int32
(the walks without a debug knob).
(c) The MODEL: integers exactly, floating point inside the bounds the section tests already state for the same quantity.
A failure prints the seed, the step and the script up to it as Python literals: run_script replays them."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import complete_cohort as C
import engine_walk as W
from conftest import ROOT, align_sign, load_pkg
from loadings_cohort import pack_rows

pytestmark = pytest.mark.gpu

MAX_ENGINES = 6
FLOATS = ("b", "rs", "mm", "y", "components", "eigenvalues", "w")     # the floating-point outputs, by name


@pytest.fixture(scope="module")
def P():
    return load_pkg()


def new_engine(P, model):
    return P.PcoaEngine(model.n, gram_kernel=model.kernel, operand=model.operand)


def bits_of(x, garbage=False):
    """carrier bitsets of x != 0 with one padding word; garbage: the padding word holds 0xa5a5a5a5"""
    bits = load_pkg("ingest").pack_bits(np.asarray(x) != 0, pad_words=1)
    if garbage:
        bits[:, -1] = 0xa5a5a5a5
    return bits


def csr_of(x):
    rows = [np.flatnonzero(r).astype(np.int32) for r in x]
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([r.size for r in rows])
    idx = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int32)
    return np.ascontiguousarray(idx, dtype=np.int32), offs


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def feed(eng, comp, a, n):
    """One append in the script's form.  Under a binding the companion takes the missing rows: from the same read of the .bed
    rows (bed_calls), else as bitsets."""
    import torch
    x, missing = W.rows_of(a, n)
    form, k = a["form"], a["k"]
    if form == "empty":
        eng.accumulate_dense_u8(np.zeros((0, n), dtype=np.uint8))
    elif form == "f32_host":
        eng.accumulate_dense(x.astype(np.float32))
    elif form == "f32_dev":
        buf = torch.full((k, n + 5), float("nan"), dtype=torch.float32, device="cuda")
        buf[:, :n] = torch.from_numpy(x.astype(np.float32)).cuda()
        eng.accumulate_dense(buf)
    elif form == "u8_host":
        eng.accumulate_dense_u8(x)
    elif form == "u8_dev":
        buf = torch.full((k, n + 3), 255, dtype=torch.uint8, device="cuda")
        buf[:, :n] = torch.from_numpy(x).cuda()
        eng.accumulate_dense_u8(buf)
    elif form == "bits_host":
        eng.accumulate_bits(bits_of(x, garbage=True))
    elif form == "bits_dev":
        eng.accumulate_bits(torch.from_numpy(bits_of(x, garbage=True).view(np.int32)).cuda())
    elif form == "csr_host":
        eng.accumulate_calls(*csr_of(x))
    elif form == "csr_pinned":
        idx, offs = csr_of(x)
        eng.accumulate_calls_tensors(torch.from_numpy(idx).pin_memory(), torch.from_numpy(offs).pin_memory(), asynchronous=True)
    elif form == "csr_dev":
        idx, offs = csr_of(x)
        eng.accumulate_calls_tensors(torch.from_numpy(idx).cuda(), torch.from_numpy(offs).cuda())
    elif form in W.BED_FORMS:
        rows = C.bed_rows(x != 0, missing, ref_is_a1=a["ref_is_a1"], seed=a["seed"], row_bytes=(n + 3) // 4 + 3)
        if form == "bed_host":
            eng.accumulate_plink_bed(rows, ref_is_a1=a["ref_is_a1"])
        elif form == "bed_dev":
            eng.accumulate_plink_bed(torch.from_numpy(rows).cuda(), ref_is_a1=a["ref_is_a1"])
        else:
            eng.accumulate_plink_bed_calls(rows, comp, ref_is_a1=a["ref_is_a1"])
    elif form == "ld_prune":
        # two chunks through one pruner, the first from the host, the second from the device; the masks are the rule's
        cut, keep = W.ld_chunks(a, x)
        with eng.ld_pruner(a["window"], a["r2"], accumulate=True) as ld:
            first = ld.bits(bits_of(x[:cut], garbage=True))
            if a["reset_between"]:
                eng.reset()                                           # drops the carried rows with S: the window starts over
            second = ld.bits(torch.from_numpy(bits_of(x[cut:], garbage=True).view(np.int32)).cuda())
        assert np.array_equal(np.concatenate([first, second]), keep), ("the pruner's keep mask", a)
    elif form == "ragged":
        rng = np.random.default_rng(a["seed"] + 1)
        bits = bits_of(x)
        cuts = sorted(set([0, k] + [int(c) for c in rng.integers(1, k, size=3)]))
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate_bits(np.ascontiguousarray(bits[lo:hi]))
            eng.accumulate_bits(bits[:0])
    else:
        raise ValueError(form)
    if comp is not None and form != "bed_calls" and k:
        comp.accumulate_bits(bits_of(missing))
        comp.sync()
    eng.sync()


class Walked(object):
    """the engine a walk is on and its companion, beside the model"""

    def __init__(self, P, index):
        self.P, self.model = P, W.new_model(index)
        self.eng, self.comp, self.owned, self.tstream = new_engine(P, self.model), None, False, None

    def close(self):
        if self.eng is not None:
            if self.comp is not None and not self.owned:
                self.eng.set_call_companion(None)
            self.eng.close()
        if self.comp is not None and not self.owned:
            self.comp.close()
        self.eng = self.comp = None

    def engines(self):
        return 1 + (self.comp is not None)

    def drop_companion(self):
        self.eng.set_call_companion(None)                   # (an owned companion goes with the binding)
        if self.comp is not None and not self.owned:
            self.comp.close()
        self.comp, self.owned = None, False

    def mutate(self, op, a):
        import torch
        P, eng, n = self.P, self.eng, self.eng.n
        after = W.apply(self.model.copy(), op, a)
        if op == "append":
            feed(eng, self.comp, a, n)
            if self.comp is not None:
                eng.set_call_companion(self.comp, after.comp.v)                   # the caller binds again when V changes
        elif op == "reset":
            eng.reset()
        elif op == "load":
            eng.load_gram(W.load_of(a, n))
        elif op == "export_import":
            buf = torch.zeros((n, n), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            eng.export_device(buf.data_ptr())
            eng.sync()
            eng.import_device(buf.data_ptr())
            eng.sync()
        elif op in ("reduce_from", "reduce_peers"):
            partners = []
            try:
                for g in range(1 if op == "reduce_from" else 2):
                    p = new_engine(P, self.model)
                    partners.append(p)
                    if a.get("near"):
                        p.load_gram(W.near_gram(a["seed"], n))
                    else:
                        p.accumulate_dense_u8(W.partner_rows(a["seed"] + g, n, a["k"]))
                assert self.engines() + len(partners) + 2 <= MAX_ENGINES
                if op == "reduce_from":
                    eng.reduce_from(partners[0])
                elif a["position"] == 0:
                    P.reduce_peers([eng] + partners, root_only=bool(a["root_only"]))
                else:
                    P.reduce_peers([partners[0], eng, partners[1]], root_only=True)   # the walk comes back empty
            finally:
                for p in partners:
                    p.close()
        elif op == "subset":
            sub = eng.subset(W.keep_of(a, n))
            if self.comp is not None and not self.owned:
                eng.set_call_companion(None)
                self.comp.close()
            eng.close()                                                           # the walk goes on on the subset
            self.eng, self.tstream = sub, None
            self.comp, self.owned = (sub.get_call_companion()[0], True) if after.comp is not None else (None, False)
        elif op == "set_similarity":
            eng.set_similarity(a["kind"])
        elif op == "bind":
            if a["v"] is None:
                self.drop_companion()
            elif a["fresh"]:
                self.comp, self.owned = P.PcoaEngine(n), False
                eng.set_call_companion(self.comp, a["v"])
            else:
                eng.set_call_companion(self.comp, a["v"])
        elif op == "companion_append":
            self.comp.accumulate_bits(bits_of(W.missing_rows(a, n)))
            self.comp.sync()
            eng.set_call_companion(self.comp, after.comp.v)
        elif op == "companion_reset":
            self.comp.reset()
        elif op == "reserve":
            eng.reserve(a["variants"], a["num_pc"])
        elif op == "set_stream":
            if a["to"] == "torch":
                self.tstream = torch.cuda.Stream()
                eng.set_stream(self.tstream.cuda_stream)
            else:
                eng.set_stream(0)
                self.tstream = None
        else:
            raise ValueError(op)
        self.model = after

    def refuse(self, kind):
        """refusals found on the host or rolled back: each returns its documented code and leaves the ctx as it was"""
        P, L, eng, n, m = self.P, self.P._lib, self.eng, self.eng.n, self.model
        code = L.PCOA_ERR_INVALID_ARG
        if kind == "bind_low_v":
            # a V below a sample's missing count is accepted by the binding and answered by the next centring, on walk and twin
            low = int(np.diagonal(m.comp.q).max()) - 1
            twin, tc = twin_of(P, m)
            try:
                for e, c in ((eng, self.comp), (twin, tc)):
                    e.set_call_companion(c, low)
                    with pytest.raises(P.PcoaError) as ei:
                        e.center()
                    assert ei.value.code == L.PCOA_ERR_INVALID_ARG, ei.value
                    e.set_call_companion(c, m.comp.v)
            finally:
                close_twin(twin, tc)
            return
        with pytest.raises(P.PcoaError) as ei:
            if kind == "index_n":
                eng.accumulate_calls(np.array([0, n], dtype=np.int32), np.array([0, 2], dtype=np.int64))
                code = L.PCOA_ERR_INDEX_RANGE
            elif kind == "block_outside":
                eng.gram_block(n - 1, 0, 2, 1)
            elif kind == "compute_0":
                eng.compute(0)
            elif kind == "compute_n1":
                eng.compute(n + 1)
            elif kind == "keep_repeat":
                keep = list(range(n))
                keep[2] = keep[1]
                eng.subset(keep)
            elif kind == "min_jaccard_0":
                eng.similar_pairs(0.0, 0)
            elif kind == "similarity_unknown":
                eng.set_similarity(7)
            elif kind == "jaccard_on_bound":
                code = L.PCOA_ERR_STATE
                eng.set_similarity("jaccard")
            elif kind == "bind_on_measured":
                code = L.PCOA_ERR_STATE
                other = P.PcoaEngine(n)
                try:
                    eng.set_call_companion(other, 5)
                finally:
                    other.close()
            elif kind == "bind_self":
                eng.set_call_companion(eng, 1)
            else:
                raise ValueError(kind)
        if kind == "index_n":
            code = L.PCOA_ERR_INDEX_RANGE
            assert isinstance(ei.value, P.IndexRangeError)
        assert ei.value.code == code, (kind, ei.value)


def twin_of(P, model):
    """A fresh engine brought straight to the model's state, and its companion (or None)."""
    eng = new_engine(P, model)
    eng.load_gram(model.s)
    eng.set_similarity(model.measure)
    comp = None
    if model.comp is not None:
        comp = P.PcoaEngine(model.n)
        comp.load_gram(model.comp.q)
        eng.set_call_companion(comp, model.comp.v)
    return eng, comp


def close_twin(twin, comp):
    if comp is not None:
        twin.set_call_companion(None)
    twin.close()
    if comp is not None:
        comp.close()


def observe(P, eng, op, a):
    """What observer `op` returns on `eng`: ("ok", {name: numpy array}, gram_i64_live) or ("error", code, message)."""
    import torch
    n = eng.n
    try:
        if op == "gram":
            out = {"s": eng.gram()}
        elif op == "gram_block":
            out = {"s": eng.gram_block(*a["rect"])}
        elif op == "export":
            buf = torch.zeros((n, n), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            eng.export_device(buf.data_ptr())
            eng.sync()
            out = {"s": buf.cpu().numpy()}
        elif op == "pairs":
            pairs, found, diag = eng.similar_pairs(a["min_jaccard"], a["capacity"])
            out = {"found": np.array([found], dtype=np.int64), "i": pairs["i"].copy(), "j": pairs["j"].copy(),
                   "shared": pairs["shared"].copy(), "diag": diag}
        elif op == "center":
            b, rs, nz, mm = eng.center()
            out = {"b": b, "rs": rs, "mm": np.array([mm]), "nz": np.array([nz], dtype=np.int64)}
        elif op == "matvec":
            out = {"y": eng.debug_centred_matvec(W.vector_of(a["seed"], n), a["form"])}
        elif op == "compute":
            comps, lam, nz = eng.compute(a["k"])
            out = {"components": comps, "eigenvalues": lam, "nz": np.array([nz], dtype=np.int64)}
        elif op == "loadings":
            x, u, lam = W.loadings_of(a, n)
            with eng.loadings(u, lam) as ld:
                out = {"w": ld.bits(pack_rows(x, n, pad_words=1, garbage=True))}
        elif op == "getters":
            comp, v = eng.get_call_companion()
            out = {"similarity": np.array([eng.SIMILARITY_KINDS[eng.get_similarity()]], dtype=np.int64),
                   "companion": np.array([0 if comp is None else 1, v], dtype=np.int64)}
        else:
            raise ValueError(op)
        return "ok", out, int(eng.timings()["gram_i64_live"])
    except P.PcoaError as e:
        return "error", e.code, str(e)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_twin(got, want, floats_too):
    """(a): no tolerance.  floats_too False: walk and twin hold S differently (a debug knob), the floating-point outputs are left
    to the model's bounds"""
    assert got[0] == want[0], ("walk and twin differ in kind", got[:2], want[:2])
    if got[0] == "error":
        assert got[1] == want[1], ("walk and twin differ in the error code", got, want)
        return
    assert sorted(got[1]) == sorted(want[1])
    for name in sorted(got[1]):
        if name in FLOATS and not floats_too:
            continue
        a, b = got[1][name], want[1][name]
        if not same_bytes(a, b):
            where = np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:5] if a.shape == b.shape else None
            raise AssertionError("walk and twin differ in %r: shapes %s / %s, first entries %s: %s / %s" % (
                name, a.shape, b.shape, where, None if where is None else a.reshape(-1)[where], None if where is None else b.reshape(-1)[where]))


def check_model(got, exp, op):
    """(c): an engine's output against the model"""
    assert exp.error is None and got[0] == "ok", got
    out = got[1]
    for name, want in exp.exact.items():
        assert np.array_equal(out[name], want), (op, name, out[name], want)
    for name, (want, bound) in exp.close.items():
        assert out[name].shape == np.shape(want), (op, name, out[name].shape, np.shape(want))
        err = np.abs((out[name].astype(np.longdouble) - np.asarray(want, dtype=np.longdouble)).astype(np.float64))
        assert np.all(err <= bound), (op, name, float(err.max()), float(np.max(bound)))
    if op == "compute":
        lam = exp.note["eigenvalues"]
        if not lam.any():
            assert np.allclose(out["eigenvalues"], 0) and np.isfinite(out["components"]).all()   # S = 0 (tests/test_gpu_parity.py)
        else:
            assert np.allclose(out["eigenvalues"], lam, rtol=1e-6, atol=0), (out["eigenvalues"], lam)
        if exp.note["vectors"] is not None:
            want = exp.note["vectors"]
            assert np.abs(align_sign(out["components"], want) - want).max() < 1e-6


# ---- a walk -----------------------------------------------------------------------------------------------------------------
def run_script(P, index, script, knobs=False):
    """Walks an engine with the flags of WALKS[index] through `script`; returns (observer steps, floating-point observers held
    byte for byte, those left to the bounds, seconds).  Any failure names the step and prints what replays it."""
    t0 = time.time()
    walked = Walked(P, index)
    observers = by_bytes = by_bound = 0
    at = -1
    try:
        for at, (op, a) in enumerate(script):
            if op in W.MUTATORS:
                walked.mutate(op, a)
            elif op == "refuse":
                walked.refuse(a["kind"])
            else:
                model = walked.model
                got = observe(P, walked.eng, op, a)
                twin, tc = twin_of(P, model)
                try:
                    assert walked.engines() + 1 + (tc is not None) <= MAX_ENGINES
                    want = observe(P, twin, op, a)
                finally:
                    close_twin(twin, tc)
                same_form = got[0] == "ok" and want[0] == "ok" and got[2] == want[2]
                if not knobs:                                                  # (b)
                    assert got[0] == "ok" and want[0] == "ok", (got, want)
                    assert got[2] == want[2] == model.i64_live(), ("gram_i64_live of walk, twin, model", got[2], want[2], model.i64_live())
                check_twin(got, want, same_form)
                exp = model.expect(op, a)
                check_model(want, exp, op)
                if any(name in FLOATS for name in want[1]):
                    by_bytes, by_bound = by_bytes + same_form, by_bound + (not same_form)
                if not same_form:
                    check_model(got, exp, op)
                observers += 1
    except BaseException as e:
        sys.stdout.write("\nengine walk failed: walk %d %r, op %d of %d: %s: %s\nreplay with run_script(P, %d, %r, knobs=%r)\n" % (
            index, W.WALKS[index], at, len(script), type(e).__name__, e, index, list(script[:at + 1]), knobs))
        raise
    finally:
        walked.close()
    return observers, by_bytes, by_bound, time.time() - t0


IN_PROCESS = [w for w in range(len(W.WALKS)) if W.WALKS[w][4] is None]
CHILDREN = [w for w in range(len(W.WALKS)) if W.WALKS[w][4] is not None]


@pytest.mark.parametrize("walk", IN_PROCESS)
def test_a_walked_engine_equals_its_twin_and_the_model_at_every_observer(P, walk):
    observers, by_bytes, by_bound, seconds = run_script(P, walk, W.script(walk))
    assert observers == len(W.steps_of(W.script(walk)))
    print("walk %d %r: %d steps in %.2f s; floating-point observers byte for byte %d, inside the bounds only %d" % (
        walk, W.WALKS[walk], observers, seconds, by_bytes, by_bound))
    assert by_bound == 0          # no knob: the representation cannot differ, so no floating-point observer may fall back


def test_a_reset_leaves_no_int64_part_behind(P):
    """The fixed case beside the walks.  A companion whose S went beyond int32, was reset and then fed a few
    rows must be accepted by the next centring (a companion with an int64 part is refused); an engine with the same history
    keeps the upper-triangle mat-vec form; and reset leaves the cumulative counters alone (include/pcoa.h).  The int64 part is
    reached by a load beyond int32: without a debug knob no fold happens at this size.  The same case by a real fold runs in
    child A (fold_reset_feed), where the threshold is 200 variants."""
    n = 64
    a = {"k": 40, "seed": 77, "missing": True}
    x, missing = W.rows_of(a, n)
    with P.PcoaEngine(n) as eng, P.PcoaEngine(n) as comp, P.PcoaEngine(n) as twin, P.PcoaEngine(n) as tc:
        for e in (eng, comp):
            e.load_gram(W.big_gram(5, n))
            assert e.timings()["gram_i64_live"] == 1
            e.reset()
            assert e.timings()["gram_i64_live"] == 0 and not e.gram().any()
        eng.accumulate_dense_u8(x)
        comp.accumulate_bits(bits_of(missing))
        eng.finalize()                                                # (a deferred chunk is counted when it is contracted)
        t = eng.timings()
        assert t["gram_i64_live"] == 0 and t["gram_variants"] == 40 and comp.timings()["gram_i64_live"] == 0
        eng.set_call_companion(comp, 40)
        twin.load_gram(eng.gram())
        tc.load_gram(comp.gram())
        twin.set_call_companion(tc, 40)
        got, want = eng.center(), twin.center()                       # refused with PCOA_ERR_STATE while reset kept the int64 part
        assert same_bytes(got[0], want[0]) and same_bytes(got[1], want[1]) and got[2:] == want[2:]
        xv = W.vector_of(1, n)
        assert same_bytes(eng.debug_centred_matvec(xv, 1), twin.debug_centred_matvec(xv, 1))
        eng.set_call_companion(None)
        twin.set_call_companion(None)
        eng.reset()
        assert eng.timings()["gram_variants"] == 40                   # cumulative since create / reset_timings, not a statement about S


def fold_reset_feed(P, n=64):
    """Child A only (PCOA_DEBUG_FOLD_THRESHOLD=200): a companion that FOLDED, was reset and fed fewer rows than the threshold
    has no int64 part, and the next centring accepts it and returns the twin's bits."""
    big = {"k": 400, "seed": 78, "missing": True}
    small = {"k": 40, "seed": 79, "missing": True}
    x, missing = W.rows_of(small, n)
    with P.PcoaEngine(n) as eng, P.PcoaEngine(n) as comp, P.PcoaEngine(n) as twin, P.PcoaEngine(n) as tc:
        for e in (eng, comp):
            e.accumulate_bits(bits_of(W.rows_of(big, n)[1]))
            e.finalize()
            assert e.timings()["gram_i64_live"] == 1, "no fold happened: is the threshold set?"
            e.reset()
            assert e.timings()["gram_i64_live"] == 0
        eng.accumulate_dense_u8(x)
        comp.accumulate_bits(bits_of(missing))
        eng.set_call_companion(comp, 40)
        twin.load_gram(eng.gram())
        tc.load_gram(comp.gram())
        assert comp.timings()["gram_i64_live"] == 0 and tc.timings()["gram_i64_live"] == 0
        twin.set_call_companion(tc, 40)
        got, want = eng.center(), twin.center()
        assert same_bytes(got[0], want[0]) and same_bytes(got[1], want[1]) and got[2:] == want[2:]
        eng.set_call_companion(None)
        twin.set_call_companion(None)


CHILD = r"""
import sys
sys.path.insert(0, %(tests)r)
import engine_walk as W
import test_gpu_engine_walk as T
from conftest import load_pkg
observers, by_bytes, by_bound, seconds = T.run_script(load_pkg(), %(walk)d, W.script(%(walk)d), knobs=True)
assert observers == len(W.steps_of(W.script(%(walk)d)))
print("walk %(walk)d %%r: %%d steps in %%.2f s; floating-point observers byte for byte %%d, inside the bounds only %%d" %% (
    W.WALKS[%(walk)d], observers, seconds, by_bytes, by_bound))
if W.WALKS[%(walk)d][4] == "A":
    T.fold_reset_feed(load_pkg())
    print("fold -> reset -> feed: accepted")
print("WALK-OK")
"""
CHILD_LIMIT = {"A": 30, "B": 30}      # seconds: about ten times the wall of the child on an idle MI355X
_FAULTED = []


@pytest.mark.parametrize("walk", CHILDREN)
def test_a_walk_under_debug_knobs(walk):
    """Child A: folds, spare re-use, several launches and several pack chunks inside nearly every append.  Child B: no narrowing,
    so the int64 kernels serve the observers.  The knobs are read once per process: one fresh child each, one after the other,
    under its own time limit, never retried; after a child that died of a signal or ran out of time the other is not started."""
    name = W.WALKS[walk][4]
    if _FAULTED:
        pytest.fail("not started: an earlier child of this module ended abnormally (%s)" % _FAULTED[0])
    env = dict(os.environ, **W.CHILD_ENV[name])
    try:
        res = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests"), "walk": walk}], env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=CHILD_LIMIT[name])
    except subprocess.TimeoutExpired as e:
        _FAULTED.append("child %s: time limit %d s" % (name, CHILD_LIMIT[name]))
        pytest.fail("child %s exceeded its time limit of %d s; output so far:\n%s" % (name, CHILD_LIMIT[name], e.stdout))
    if res.returncode < 0 or res.returncode in (134, 139):
        _FAULTED.append("child %s: exit status %d" % (name, res.returncode))
    print(res.stdout[-400:] if res.returncode == 0 else res.stdout[-6000:])
    assert res.returncode == 0 and "WALK-OK" in res.stdout, res.stdout[-6000:]

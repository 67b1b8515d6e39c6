"""GPU walks over a GRM ctx: an engine is taken through the scripts of tests/grm_walk.py -- appends across the
sizes at which its buffers regrow, resets, min_maf changes, prunes, subsets -- and at every observer it is held to two things.
(a) A TWIN: a fresh engine created with the model's N, fed the model's rows in one call, given min_maf and the model's prune.
Everything a GRM ctx returns is documented to be a function of exactly that and the call's arguments, so walk and twin must
agree byte for byte; no tolerance.  This is the check that sees a stale flag or a buffer that regrew under resident state.
(b) The MODEL: counts, rows, masks, n(i, j), called and M' exactly, the floating-point outputs inside the bounds the GRM tests
already state.  A failure prints the seed, the step and the script up to it as Python literals: run_script replays them."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import grm_walk as W
from conftest import ROOT, align_sign, load_pkg
from grm_subset_cohort import pack_rows
from test_grm_cpu import pack_bed

pytestmark = pytest.mark.gpu

MAX_ENGINES = 4


@pytest.fixture(scope="module")
def P():
    return load_pkg()


def device_vector(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def feed(eng, a, n):
    """One append in the script's form: host rows; host rows with garbage in the padding slots and three extra row bytes, in ragged
    calls with an empty one between them; a device tensor; an empty call."""
    codes = W.rows_of(a, n)
    if a["form"] == "empty":
        eng.accumulate_plink_bed(np.zeros((0, (n + 3) // 4), dtype=np.uint8), ref_is_a1=a["ref_is_a1"])
    elif a["form"] == "host":
        eng.accumulate_plink_bed(pack_bed(codes), ref_is_a1=a["ref_is_a1"])
    elif a["form"] == "device":
        import torch
        eng.accumulate_plink_bed(torch.from_numpy(pack_bed(codes)).cuda(), ref_is_a1=a["ref_is_a1"])
    else:
        rng = np.random.default_rng(a["seed"] + 1)
        rows = pack_bed(codes, 3, rng)
        k = rows.shape[0]
        cuts = sorted(set([0, k] + [int(c) for c in rng.integers(1, k, size=min(3, k - 1))])) if k > 1 else [0, k]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.accumulate_plink_bed(np.ascontiguousarray(rows[lo:hi]), ref_is_a1=a["ref_is_a1"])
            eng.accumulate_plink_bed(rows[:0], ref_is_a1=a["ref_is_a1"])
    eng.sync()


class Walked(object):
    """the engine a walk is on and its study store, beside the model of both"""

    def __init__(self, P, n):
        self.P, self.state = P, W.State(n)
        self.eng, self.study = P.PcoaEngine(n, grm=True), None

    def close(self):
        for e in (self.eng, self.study):
            if e is not None:
                e.close()
        self.eng = self.study = None

    def mutate(self, op, a):
        eng = self.eng
        if op == "append":
            feed(eng, a, eng.n)
        elif op == "reset":
            eng.reset()
        elif op in ("min_maf_new", "min_maf_same"):
            eng.grm_set_min_maf(a["maf"])
        elif op == "ld_prune":
            got = eng.grm_ld_prune(a["window"], a["r2"], a["breaks"])
        elif op == "ld_clear":
            eng.grm_ld_clear()
        elif op == "subset_panel":
            self.eng = eng.grm_subset(W.keep_of(a, eng.n))
            eng.close()                                                   # the walk goes on on the subset
        elif op == "subset_study":
            if self.study is not None:
                self.study.close()
            self.study = eng.grm_subset(W.keep_of(a, eng.n), study=True)
        self.state.apply(op, a)
        if op == "ld_prune":
            keep = self.state.panel.mask()
            cand = int(W.LD.candidates(np.array([0, -1, 1, 2], dtype=np.int8)[self.state.panel.codes], self.state.panel.min_maf).sum())
            assert got == (cand, int(keep.sum())), (got, cand, int(keep.sum()))

    def refuse(self, kind):
        """host-side refusals, found before any device work: each returns its documented code and leaves the ctx as it was"""
        L, eng = self.P._lib, self.eng
        with pytest.raises(self.P.PcoaError) as ei:
            if kind == "rect_outside":
                eng.grm_block(eng.n - 1, 2, 0, 1)
            elif kind == "band_63":
                eng.grm_pairs(0.1, band_rows=63, capacity=0)
            elif kind == "keep_not_increasing":
                keep = list(range(eng.n))
                keep[2] = keep[1]                                         # every index inside [0, N), one of them twice
                eng.grm_subset(keep)
            elif kind == "min_maf_half":
                eng.grm_set_min_maf(0.5)
            else:
                assert self.study is not None and self.state.study.v != self.state.panel.v
                comps, lam = W.vectors_of(1, eng.n, 1)
                eng.grm_project(self.study, comps, lam)
        assert ei.value.code == (L.PCOA_ERR_STATE if kind == "project_other_v" else L.PCOA_ERR_INVALID_ARG), (kind, ei.value.code)


def twin_of(P, model):
    """A fresh engine brought straight to the model's state."""
    eng = P.PcoaEngine(model.n, grm=not model.study, grm_study=model.study)
    if model.v:
        eng.accumulate_plink_bed(pack_rows(model.codes), ref_is_a1=True)
    if not model.study:
        eng.grm_set_min_maf(model.min_maf)
        if model.prune is not None:
            eng.grm_ld_prune(*model.prune)
    return eng


def observe(P, eng, study, op, a):
    """What observer `op` returns on `eng`: ("ok", {name: numpy array}) or ("error", code, message)."""
    try:
        if op == "info":
            return "ok", {"info": np.array(eng.grm_info()[:2], dtype=np.int64), "counts": eng.grm_counts(a["first"], a["n"])}
        if op == "rows":
            return "ok", {"rows": eng.grm_rows(a["first"], a["n"])}
        if op == "ld_mask":
            return "ok", {"mask": eng.grm_ld_mask(a["first"], a["n"])}
        if op == "matvec":
            return "ok", {"y": eng.grm_matvec_device(device_vector(W.vectors_of(a["seed"], eng.n, 1)[0][:, 0])).cpu().numpy()}
        if op == "block":
            r0, r, c0, c = a["rect"]
            got = eng.grm_block(r0, r, c0, c, a["divisor"], pairs=a["pairs"], device=a["device"])
            got = got if a["pairs"] else (got,)
            got = [g.cpu().numpy() if a["device"] else g for g in got]
            return "ok", dict(zip(("k", "n"), got))
        if op == "pairs":
            pairs, found = eng.grm_pairs(a["cutoff"], a["divisor"], band_rows=a["band_rows"], capacity=W.capacity_of(a["capacity"], eng.n))
            return "ok", {"found": np.array([found], dtype=np.int64), "i": pairs["i"].copy(), "j": pairs["j"].copy(),
                          "n": pairs["n"].copy(), "k": pairs["k"].copy()}
        if op == "weights":
            comps, lam = W.vectors_of(a["seed"], eng.n, a["num_pc"])
            return "ok", {"w": eng.grm_weights(comps, lam, scaled=a["scaled"], first_variant=a["first"], n_variants=a["n"])}
        if op == "project":
            comps, lam = W.vectors_of(a["seed"], eng.n, a["num_pc"])
            xy, called = eng.grm_project(eng if a["study"] == "self" else study, comps, lam)
            return "ok", {"coords": xy, "called": called}
        if op == "compute":
            comps, lam, nz = eng.compute(a["num_pc"])
            return "ok", {"components": comps, "eigenvalues": lam, "nonzero": np.array([nz], dtype=np.int64)}
    except P.PcoaError as e:
        return "error", e.code, str(e)
    raise ValueError(op)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_twin(got, want):
    """(a): no tolerance"""
    assert got[0] == want[0], ("walk and twin differ in kind", got[:2], want[:2])
    if got[0] == "error":
        assert got[1] == want[1], ("walk and twin differ in the error code", got, want)
        return
    assert sorted(got[1]) == sorted(want[1])
    for name in sorted(got[1]):
        a, b = got[1][name], want[1][name]
        if not same_bytes(a, b):
            where = np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:5] if a.shape == b.shape else None
            raise AssertionError("walk and twin differ in %r: shapes %s / %s, first entries %s: %s / %s" % (
                name, a.shape, b.shape, where, None if where is None else a.reshape(-1)[where], None if where is None else b.reshape(-1)[where]))


def check_model(P, twin, got, exp, op, a):
    """(b): the twin's output (the walk's, after (a)) against the model"""
    if exp.error is not None:
        assert got[0] == "error" and got[1] == getattr(P._lib, exp.error[0]) and exp.error[1] in got[2], (got, exp.error)
        return
    assert got[0] == "ok", got
    out = got[1]
    for name, want in exp.exact.items():
        assert np.array_equal(out[name], want), (name, out[name].shape, np.asarray(want).shape)
    for name, (want, bound) in exp.close.items():
        assert out[name].shape == want.shape, (name, out[name].shape, want.shape)
        err = np.abs(out[name] - want)
        assert np.all(err <= bound), (name, float((err - bound).max()), float(err.max()))
    if op == "pairs":
        # the list is the rule applied to the bits pcoa_grm_block returns on the same ctx (include/pcoa.h)
        vp = load_pkg("variants_pca")
        k = twin.grm_dense(a["divisor"])
        cnt = twin.grm_pairs_block(0, twin.n, 0, twin.n) if a["divisor"] == "pairwise" else twin.grm_info()[1]
        want = vp.grm_pairs_rule(k, a["cutoff"], cnt)
        assert out["found"][0] == want.size
        listed = want[:out["i"].size]
        assert np.array_equal(out["i"], listed["i"]) and np.array_equal(out["j"], listed["j"]) and np.array_equal(out["n"], listed["n"])
        assert same_bytes(out["k"], np.ascontiguousarray(listed["k"]))
    if op == "compute":
        lam = exp.note["eigenvalues"]
        assert np.allclose(out["eigenvalues"], lam, rtol=1e-6, atol=0), (out["eigenvalues"], lam)
        if exp.note["vectors"] is not None:
            want = exp.note["vectors"]
            assert np.abs(align_sign(out["components"], want) - want).max() < 1e-6


# ---- a walk -----------------------------------------------------------------------------------------------------------------
def run_script(P, n0, script, seed=None):
    """Walks an engine of n0 samples through `script`; returns (observer steps, seconds).  Any failure names the step and prints
    what replays it."""
    t0 = time.time()
    walked = Walked(P, n0)
    observers = 0
    at = -1
    try:
        for at, (op, a) in enumerate(script):
            if op in W.MUTATORS:
                walked.mutate(op, a)
            elif op == "refuse":
                walked.refuse(a["kind"])
            else:
                panel, study = walked.state.panel, walked.state.study
                got = observe(P, walked.eng, walked.study, op, a)
                twin = twin_of(P, panel)
                twin_study = twin_of(P, study) if op == "project" and a["study"] == "study" else None
                try:
                    assert 2 + (walked.study is not None) + (twin_study is not None) <= MAX_ENGINES
                    want = observe(P, twin, twin_study, op, a)
                    check_twin(got, want)
                    check_model(P, twin, want, panel.expect(op, a, study), op, a)
                finally:
                    twin.close()
                    if twin_study is not None:
                        twin_study.close()
                observers += 1
    except BaseException as e:
        sys.stdout.write("\nGRM walk failed: seed %r, N = %d, op %d of %d: %s: %s\nreplay with run_script(P, %d, %r)\n" % (
            seed, n0, at, len(script), type(e).__name__, e, n0, list(script[:at + 1])))
        raise
    finally:
        walked.close()
    return observers, time.time() - t0


IN_PROCESS = [w for w in range(len(W.WALKS)) if W.WALKS[w][2] is None]


@pytest.mark.parametrize("walk", IN_PROCESS)
def test_a_walked_engine_equals_its_twin_and_the_model_at_every_observer(P, walk):
    seed, n0, _, _ = W.WALKS[walk]
    observers, seconds = run_script(P, n0, W.script(walk), seed)
    assert observers == len(W.steps_of(W.script(walk)))
    print("walk %d (seed %d, N = %d): %d steps in %.2f s" % (walk, seed, n0, observers, seconds))


CHILD = r"""
import sys
sys.path.insert(0, %(tests)r)
import grm_walk as W
import test_gpu_grm_walk as T
from conftest import load_pkg
seed, n0, segment, _ = W.WALKS[%(walk)d]
observers, seconds = T.run_script(load_pkg(), n0, W.script(%(walk)d), seed)
assert observers == len(W.steps_of(W.script(%(walk)d)))
print("walk %(walk)d (seed %%d, N = %%d, segments of %%d rows): %%d steps in %%.2f s" %% (seed, n0, segment, observers, seconds))
print("WALK-OK")
"""


def test_a_walk_over_segments_of_96_rows():
    """Both stores of the walk and every twin in segments of 96 rows, so that the appends and the subset gathers cut at segment
    boundaries of source and result (the knob is read once per process: a fresh child)."""
    walk = [w for w in range(len(W.WALKS)) if W.WALKS[w][2] is not None][0]
    env = dict(os.environ)
    env["PCOA_GRM_SEGMENT_ROWS"] = str(W.WALKS[walk][2])
    res = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests"), "walk": walk}], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(res.stdout[-400:] if res.returncode == 0 else res.stdout[-6000:])
    assert res.returncode == 0 and "WALK-OK" in res.stdout, res.stdout[-6000:]

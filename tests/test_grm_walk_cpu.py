"""CPU tests of the walks over a GRM ctx (tests/grm_walk.py): the model against an independent dense statement
with numpy.linalg, and what the committed scripts cover, asserted from the script data alone -- tests/test_gpu_grm_walk.py runs
the same scripts on an engine, so a pair, a threshold or a drop that is missing here is missing there."""
import numpy as np
import pytest

import grm_ld_cohort as LD
import grm_walk as W
from conftest import align_sign
from grm_subset_cohort import pack_rows


# ---- the model against a dense statement ------------------------------------------------------------------------------------
def dense_statement(model):
    """(kept-and-used rows' indices, A [rows][N], d [rows], c [rows][N]) written out directly: the store's coding is 00 g = 0, 01
    missing, 10 g = 1, 11 g = 2; a row is used iff it is called somewhere, polymorphic, at or above min_maf and kept."""
    codes = model.codes.astype(np.int64)
    c = (codes != 1).astype(np.float64)
    g = np.where(codes == 2, 1.0, np.where(codes == 3, 2.0, 0.0))
    n_v, a_v = c.sum(axis=1), g.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = np.where(n_v > 0, a_v / n_v, 0.0)
        used = (n_v > 0) & (a_v > 0) & (a_v < 2 * n_v) & (np.minimum(a_v, 2 * n_v - a_v) >= model.min_maf * 2 * n_v)
    if model.prune is not None:
        w, t, breaks = model.prune
        gi = np.where(codes == 1, -1, g.astype(np.int64)).astype(np.int8)
        keep = LD.rule(gi, w, t, breaks, model.min_maf)[0]                 # the V x V form of the rule; the model uses the band form
        assert np.array_equal(keep, model.mask())
        used &= keep
    idx = np.flatnonzero(used)
    a = (g[idx] - mu[idx, None]) * c[idx]
    d = 1.0 / (mu[idx] * (1.0 - 0.5 * mu[idx]))
    return idx, a, d, c[idx]


SHORT = [   # (N, script): every observer once per script, with a mask installed, after a drop, on a subset
    (49, [("append", {"k": 90, "seed": 1, "edge": True, "form": "host", "ref_is_a1": False}),
          ("append", {"k": 40, "seed": 2, "edge": False, "form": "host", "ref_is_a1": True}),
          ("ld_prune", {"window": 7, "r2": 0.02, "breaks": [50]})]),
    (65, [("append", {"k": 120, "seed": 3, "edge": True, "form": "host", "ref_is_a1": True}),
          ("ld_prune", {"window": 64, "r2": 0.01, "breaks": []}),
          ("min_maf_new", {"maf": 0.05})]),
    (70, [("append", {"k": 150, "seed": 4, "edge": False, "form": "host", "ref_is_a1": False}),
          ("ld_prune", {"window": 20, "r2": 0.05, "breaks": []}),
          ("subset_study", {"size": 17, "seed": 5}),
          ("subset_panel", {"size": 33, "seed": 6}),
          ("min_maf_same", {"maf": 0.0}),
          ("ld_prune", {"window": 1, "r2": 0.005, "breaks": [3, 77]})]),
]


@pytest.mark.parametrize("case", range(len(SHORT)))
def test_the_model_equals_a_dense_statement_with_numpy_linalg(case):
    n0, script = SHORT[case]
    st = W.State(n0)
    for op, a in script:
        st.apply(op, a)
    p, study = st.panel, st.study
    n, v = p.n, p.v
    idx, a, d, c = dense_statement(p)
    m = idx.size
    assert 0 < m < v and p.used() == m
    k = (a.T * d) @ a / m
    cnt = (c.T @ c).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        kp = np.where(cnt > 0, (a.T * d) @ a / cnt, 0.0)
    tol = 1e-12

    e = p.expect("info", {"first": 3, "n": v - 5})
    assert e.exact["info"].tolist() == [v, m]
    codes = p.codes[3:v - 2]
    assert np.array_equal(e.exact["counts"], np.stack([(codes != 1).sum(1), (codes == 2).sum(1), (codes == 3).sum(1)], axis=1))
    assert np.array_equal(p.expect("rows", {"first": 0, "n": v}).exact["rows"], pack_rows(p.codes))
    e = p.expect("ld_mask", {"first": 0, "n": v})
    if p.prune is None:
        assert e.error == ("PCOA_ERR_STATE", "no keep mask")
    else:
        assert np.array_equal(e.exact["mask"][idx], np.ones(m, dtype=bool)) and e.exact["mask"].sum() == m
    e = p.expect("matvec", {"seed": 9})
    x = W.vectors_of(9, n, 1)[0][:, 0]
    assert np.abs(e.close["y"][0] - k @ x).max() <= tol and np.all(e.close["y"][1] >= 0) and e.close["y"][1].max() < 1e-9
    for divisor, want in (("used", k), ("pairwise", kp)):
        rect = (5, 20, 2, 30)
        e = p.expect("block", {"rect": rect, "divisor": divisor, "pairs": True, "device": False})
        assert np.abs(e.close["k"][0] - want[5:25, 2:32]).max() <= tol and np.array_equal(e.exact["n"], cnt[5:25, 2:32])
        assert e.close["k"][1].shape == (20, 30) and e.close["k"][1].max() < 1e-9
        iu = np.triu_indices(n, 1)
        cutoff = W.gap_cutoff(want[iu], 0.05)
        e = p.expect("pairs", {"cutoff": cutoff, "divisor": divisor, "band_rows": 0, "capacity": "all"})
        hit = want[iu] >= cutoff
        assert e.exact["found"][0] == hit.sum() > 0
        assert np.array_equal(e.exact["i"], iu[0][hit]) and np.array_equal(e.exact["j"], iu[1][hit])
        assert np.array_equal(e.exact["n"], cnt[iu][hit] if divisor == "pairwise" else np.full(hit.sum(), m))
        assert p.expect("pairs", {"cutoff": cutoff, "divisor": divisor, "band_rows": 64, "capacity": 1}).exact["i"].size == 1
    comps, lam = W.vectors_of(21, n, 3)
    t = np.zeros((v, 3))
    t[idx] = d[:, None] * (a @ comps)
    e = p.expect("weights", {"scaled": False, "first": 0, "n": v, "num_pc": 3, "seed": 21})
    assert np.abs(e.close["w"][0] - t).max() <= 1e-11
    e = p.expect("weights", {"scaled": True, "first": 2, "n": v - 2, "num_pc": 3, "seed": 21})
    wv = np.zeros((v, 3))
    wv[idx] = np.sqrt(d)[:, None] * (a @ comps) / np.sqrt(m * lam)[None, :]
    assert np.abs(e.close["w"][0] - wv[2:]).max() <= 1e-11 and np.all(e.close["w"][1] >= 0)
    for target, other in (("self", p), ("study", study)):
        if other is None:
            continue
        oc = other.codes[idx].astype(np.int64)
        og = np.where(oc == 2, 1.0, np.where(oc == 3, 2.0, 0.0))
        called = (oc != 1).astype(np.float64)
        mu = (np.where(p.codes[idx] == 2, 1.0, np.where(p.codes[idx] == 3, 2.0, 0.0)).sum(1)) / (p.codes[idx] != 1).sum(1)
        want = ((og - mu[:, None] * called).T @ t[idx]) / m / lam[None, :]
        e = p.expect("project", {"study": target, "num_pc": 3, "seed": 21}, study)
        assert np.abs(e.close["coords"][0] - want).max() <= 1e-11 and np.array_equal(e.exact["called"], called.sum(axis=0))
    e = p.expect("compute", {"num_pc": 2})
    ev, vec = np.linalg.eigh(k)
    assert np.allclose(e.note["eigenvalues"], ev[::-1][:2], rtol=1e-10, atol=0)
    assert e.exact["nonzero"][0] == (c.sum(axis=0) > 0).sum()
    if e.note["vectors"] is not None:
        want = vec[:, ::-1][:, :2]
        assert np.abs(align_sign(e.note["vectors"], want) - want).max() < 1e-8


def test_the_degenerate_answers_are_the_headers():
    p = W.Model(40)
    for op, a, err in (("block", {"rect": (0, 1, 0, 1), "divisor": "used", "pairs": False, "device": False}, "PCOA_ERR_STATE"),
                       ("pairs", {"cutoff": 0.1, "divisor": "used", "band_rows": 0, "capacity": 0}, "PCOA_ERR_STATE"),
                       ("weights", {"scaled": True, "first": 0, "n": 0, "num_pc": 1, "seed": 1}, "PCOA_ERR_INVALID_ARG"),
                       ("project", {"study": "self", "num_pc": 1, "seed": 1}, "PCOA_ERR_INVALID_ARG"),
                       ("compute", {"num_pc": 2}, "PCOA_ERR_STATE"), ("ld_mask", {"first": 0, "n": 0}, "PCOA_ERR_STATE")):
        assert p.expect(op, a).error[0] == err, op
    y, bound = p.expect("matvec", {"seed": 1}).close["y"]
    assert not y.any() and not bound.any() and y.shape == (40,)
    assert p.expect("info", {"first": 0, "n": 0}).exact["info"].tolist() == [0, 0]
    p.append(np.full((3, 40), 3, dtype=np.uint8), True)          # three monomorphic rows: V = 3, M' = 0
    assert p.expect("info", {"first": 0, "n": 3}).exact["info"].tolist() == [3, 0] and p.degenerate("matvec", {"seed": 1}) is False
    assert p.expect("block", {"rect": (0, 1, 0, 1), "divisor": "used", "pairs": False, "device": False}).error[0] == "PCOA_ERR_STATE"
    other = W.Model(5, study=True)
    assert p.expect("project", {"study": "study", "num_pc": 1, "seed": 1}, other).error == ("PCOA_ERR_STATE", "same variants")


# ---- what the committed scripts cover ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trace():
    """per walk, per step: what the script data and the model say about it"""
    out = []
    for w, (seed, n0, segment, masked) in enumerate(W.WALKS):
        st, steps = W.State(n0), []
        for m, ma, kind, o, oa in W.steps_of(W.script(w)):
            before = {"v": st.panel.v, "mask": st.panel.prune is not None, "n": st.panel.n}
            st.apply(m, ma)
            p = st.panel
            exp = p.expect(o, oa, st.study)
            steps.append({"m": m, "ma": ma, "refuse": kind, "o": o, "oa": oa, "before": before, "v": p.v, "n": p.n, "used": p.used(),
                          "mask": p.prune is not None, "degenerate": p.degenerate(o, oa, st.study), "error": exp.error,
                          "study_v": None if st.study is None else st.study.v})
            if o == "pairs" and exp.error is None:
                iu = np.triu_indices(p.n, 1)
                margin = np.abs(p.dense(oa["divisor"])[0][iu] - oa["cutoff"]) - p.dense_bound(oa["divisor"])[iu]
                steps[-1]["pairs"] = (float(margin.min()), int(exp.exact["found"][0]), iu[0].size)
        out.append(steps)
    return out


def test_the_scripts_are_plain_data_and_the_same_every_time():
    import ast
    assert len(W.WALKS) == 7 and sorted(set(w[1] for w in W.WALKS)) == [49, 65, 130, 260]
    assert [w[2] for w in W.WALKS].count(96) == 1 and W.WALKS[-1][1:3] == (130, 96)
    for w in range(len(W.WALKS)):
        assert ast.literal_eval(repr(list(W.script(w)))) == list(W.script(w))
        assert tuple(W.Planner(w).run()) == W.script(w)
        assert 36 <= len(W.steps_of(W.script(w))) <= W.STEPS_CAP


def test_every_mutator_observer_pair_occurs(trace):
    seen = set((s["m"], s["o"]) for steps in trace for s in steps)
    missing = [(m, o) for m in W.MUTATORS for o in W.OBSERVERS if (m, o) not in seen]
    assert not missing, missing


def test_every_observer_sees_a_mask_and_each_way_of_dropping_one(trace):
    masked = set(s["o"] for steps in trace for s in steps if s["mask"])
    assert masked == set(W.OBSERVERS), set(W.OBSERVERS) - masked
    for dropper in W.DROPPERS:
        real = lambda s: s["m"] == dropper and s["before"]["mask"] and not s["mask"]
        after = set(s["o"] for steps in trace for s in steps if real(s))
        assert after == set(W.OBSERVERS), (dropper, set(W.OBSERVERS) - after)
    # and the calls that must keep one do: the same min_maf, a subset taken of the engine, an empty call
    for keeper in ("min_maf_same", "subset_study"):
        assert any(s["m"] == keeper and s["before"]["mask"] and s["mask"] for steps in trace for s in steps), keeper
    assert any(s["m"] == "append" and s["ma"]["k"] == 0 and s["before"]["mask"] and s["mask"] for steps in trace for s in steps)


def test_every_walk_leaves_the_weights_alone_stale_and_prunes_over_a_mask(trace):
    """Two transitions in which one flag carries the whole change, each followed by an observer that reads the weights: a new
    min_maf with no mask to drop, and a prune over an installed mask (the twin's first prune has none to prune over)."""
    for w, steps in enumerate(trace):
        pairs = list(zip(steps[:-1], steps[1:]))
        reads = lambda s: s["o"] in W.RESIDENT_AFTER and not s["degenerate"]
        assert any(a["o"] in W.RESIDENT_AFTER and a["used"] > 0 and b["m"] == "min_maf_new" and not b["before"]["mask"] and reads(b)
                   for a, b in pairs), w
        assert any(b["m"] == "ld_prune" and b["before"]["mask"] and reads(b) for a, b in pairs), w


def test_every_walk_crosses_every_regrow_threshold_with_resident_state_in_front(trace):
    with_mask = set()
    for w, steps in enumerate(trace):
        for t in W.THRESHOLDS:
            hits = [i for i, s in enumerate(steps) if s["m"] == "append" and W.crosses(s["before"]["v"], s["v"], t)]
            resident = [i for i in hits if i > 0 and steps[i - 1]["o"] in W.RESIDENT_AFTER and steps[i - 1]["used"] > 0]
            assert resident, (w, t, hits)
            with_mask |= set((t, w) for i in resident if steps[i]["before"]["mask"])
    for t in W.THRESHOLDS:
        assert any(tw[0] == t for tw in with_mask), t
    assert any(all((t, w) in with_mask for t in W.THRESHOLDS) for w in range(len(trace)))
    assert max(s["v"] for steps in trace for s in steps) > 1024 and min(s["v"] for steps in trace for s in steps) == 0


def test_the_shared_buffers_change_hands_between_calls_of_other_sizes(trace):
    """grm_blk: a block then the bands of a pair screen, and the other way round, with another size; grm_mw: the weights then a
    projection, and the other way round"""
    found = set()
    for steps in trace:
        for a, b in zip(steps[:-1], steps[1:]):
            if a["degenerate"] or b["degenerate"]:
                continue
            size = {"block": lambda s: W.block_doubles(s["oa"]), "pairs": lambda s: W.pairs_doubles(s["oa"], s["n"])}
            if (a["o"], b["o"]) in (("block", "pairs"), ("pairs", "block")) and size[a["o"]](a) != size[b["o"]](b):
                found.add((a["o"], b["o"], size[a["o"]](a) > size[b["o"]](b)))
            if (a["o"], b["o"]) in (("weights", "project"), ("project", "weights")):
                found.add((a["o"], b["o"]))
    assert ("weights", "project") in found and ("project", "weights") in found, found
    assert any(f[:2] == ("block", "pairs") for f in found) and any(f[:2] == ("pairs", "block") for f in found), found
    assert ("block", "pairs", True) in found and ("pairs", "block", True) in found, found      # the later call gets the smaller share


def test_a_subset_of_a_pruned_engine_is_observed_and_later_pruned_itself(trace):
    ok = False
    for steps in trace:
        for i, s in enumerate(steps):
            if s["m"] == "subset_panel" and s["before"]["mask"] and not s["degenerate"] and s["n"] < s["before"]["n"]:
                ok |= any(x["m"] == "ld_prune" for x in steps[i + 1:])
    assert ok
    sizes = set(s["n"] for steps in trace for s in steps)
    assert set((97, 64, 33)) <= sizes, sizes
    assert any(s["m"] == "subset_study" for steps in trace for s in steps)
    assert any(s["o"] == "project" and s["oa"]["study"] == "study" and not s["degenerate"] for steps in trace for s in steps)


def test_degenerate_steps_are_few_and_expect_what_the_header_says(trace):
    for w, steps in enumerate(trace):
        bad = [i for i, s in enumerate(steps) if s["degenerate"]]
        assert 10 * len(bad) <= len(steps), (w, bad)
        for i in bad:
            assert steps[i]["v"] == 0 or steps[i]["error"] is not None
        assert all(s["degenerate"] or s["error"] is None for s in steps)
    # the walks do visit them: an empty store, and a missing mask
    assert any(s["v"] == 0 for steps in trace for s in steps)
    assert any(s["o"] == "ld_mask" and not s["mask"] for steps in trace for s in steps)


def test_refused_calls_are_few_and_of_every_kind(trace):
    kinds = set()
    for w, steps in enumerate(trace):
        refused = [s for s in steps if s["refuse"]]
        assert 10 * len(refused) <= len(steps), w
        kinds |= set(s["refuse"] for s in refused)
        for s in refused:
            assert s["refuse"] != "project_other_v" or (s["study_v"] is not None and s["study_v"] != s["v"])
    assert kinds == set(W.REFUSALS), set(W.REFUSALS) - kinds


def test_every_input_form_and_both_codings_feed_every_walk(trace):
    for w, steps in enumerate(trace):
        appends = [s["ma"] for s in steps if s["m"] == "append"]
        assert set(a["form"] for a in appends) == set(W.FORMS), w
        assert set(a["ref_is_a1"] for a in appends if a["k"]) == set((False, True)), w
        assert any(a["edge"] for a in appends), w


def test_no_entry_of_the_models_k_lies_within_its_bound_of_a_cutoff(trace):
    """so the pair list of pure numpy is the list the device must return; and every screen finds some pairs and not all"""
    checked = 0
    for steps in trace:
        for s in steps:
            if "pairs" in s:
                margin, found, total = s["pairs"]
                assert margin > 0 and 0 < found < total, (s["oa"], s["pairs"])
                checked += 1
    assert checked >= 14

"""CPU tests of the walks over a carrier-count engine (tests/engine_walk.py): the model against brute-force
numpy, and what the committed scripts cover, asserted from the script data and the model alone -- tests/test_gpu_engine_walk.py
runs the same scripts on an engine, so a pair, a form or a regrowth that is missing here is missing there."""
import ast

import numpy as np
import pytest

import engine_walk as W


# ---- the model against brute force ------------------------------------------------------------------------------------------
def brute_gram(x):
    x = np.asarray(x, dtype=np.int64)
    return np.array([[int((x[:, i] * x[:, j]).sum()) for j in range(x.shape[1])] for i in range(x.shape[1])], dtype=np.int64)


def brute_centre(k):
    n = k.shape[0]
    r = np.array([sum(k[i, j] for j in range(n)) for i in range(n)])
    mm = sum(r) / n / n
    b = np.array([[((k[i, j] - r[i] / n) - r[j] / n) + mm for j in range(n)] for i in range(n)])
    return b, r, mm


def test_the_model_equals_brute_force_numpy_on_a_small_script():
    n = 12
    m = W.Model(n)
    a1 = {"k": 40, "seed": 5, "mult": True}
    a2 = {"k": 30, "seed": 6, "missing": True}
    m = W.apply(m, "append", a1)
    s = brute_gram(W.rows_of(a1, n)[0])
    assert W.rows_of(a1, n)[0].max() > 1 and np.array_equal(m.s, s)
    e = m.expect("center", {})
    b, r, mm = brute_centre(s.astype(np.float64))
    assert np.array_equal(e.exact["b"], b) and np.array_equal(e.exact["rs"], r) and e.exact["mm"][0] == mm     # integers: exact in any order
    assert np.array_equal(m.expect("gram_block", {"rect": (3, 1, 4, 9)}).exact["s"], s[3:7, 1:10])
    # a measure
    m = W.apply(m, "set_similarity", {"kind": "jaccard"})
    d = np.diagonal(s)
    k = np.array([[s[i, j] / (d[i] + d[j] - s[i, j]) if d[i] + d[j] - s[i, j] > 0 else 0.0 for j in range(n)] for i in range(n)])
    b, r, mm = brute_centre(k)
    e = m.expect("center", {})
    assert np.abs(np.asarray(e.close["b"][0], dtype=np.float64) - b).max() < 1e-14 and e.close["b"][1] == W.M.entry_bound(n)
    x = W.vector_of(3, n)
    e = m.expect("matvec", {"seed": 3, "form": 0})
    assert np.abs(np.asarray(e.close["y"][0], dtype=np.float64) - b @ x).max() < 1e-13 and np.all(e.close["y"][1] > 0)
    e = m.expect("compute", {"k": 2})
    w = np.linalg.eigvalsh(b)
    assert np.allclose(e.note["eigenvalues"], w[np.argsort(-np.abs(w))][:2], rtol=1e-10)
    # pairs: the rule written out
    e = m.expect("pairs", {"min_jaccard": 0.3, "capacity": 5})
    want = [(i, j) for i in range(n) for j in range(i + 1, n) if d[i] + d[j] - s[i, j] > 0 and float(s[i, j]) >= 0.3 * float(d[i] + d[j] - s[i, j])]
    assert e.exact["found"][0] == len(want) and list(zip(e.exact["i"], e.exact["j"])) == want[:5] and np.array_equal(e.exact["diag"], d)
    # reset keeps the measure; a binding; a paired append; a subset
    m = W.apply(m, "reset", {})
    assert not m.s.any() and m.measure == "jaccard"
    m = W.apply(m, "set_similarity", {"kind": "shared"})
    m = W.apply(m, "load", {"kind": "gram", "seed": 9})
    m = W.apply(m, "bind", {"v": int(m.s.max()) + 2, "fresh": True})
    v0, s0 = m.comp.v, m.s.copy()
    m = W.apply(m, "append", a2)
    x2, miss = W.rows_of(a2, n)
    assert not (x2 * miss).any() and np.array_equal(m.s, s0 + brute_gram(x2)) and np.array_equal(m.comp.q, brute_gram(miss))
    assert m.comp.v == v0 + 30 and m.consistent()
    q, v = m.comp.q, m.comp.v
    c = v - np.diagonal(q)
    k = np.array([[m.s[i, j] / (c[i] + c[j] - v + q[i, j]) if c[i] + c[j] - v + q[i, j] > 0 else 0.0 for j in range(n)] for i in range(n)])
    b, r, mm = brute_centre(k)
    e = m.expect("center", {})
    assert np.abs(np.asarray(e.close["b"][0], dtype=np.float64) - b).max() < 1e-14
    assert m.expect("getters", {}).exact["companion"].tolist() == [1, v]
    keep = W.keep_of({"size": 7, "seed": 4}, n)
    sub = W.apply(m, "subset", {"size": 7, "seed": 4})
    assert sub.n == 7 and np.array_equal(sub.s, m.s[keep][:, keep]) and np.array_equal(sub.comp.q, q[keep][:, keep])
    assert sub.comp.v == v and sub.comp.owned and sub.measure == "shared"
    # the scaled load leaves int32, and only it
    assert m.i64_live() == 0
    big = W.apply(W.Model(n), "load", {"kind": "big", "seed": 9})
    assert big.i64_live() == 1 and W.apply(big, "reset", {}).i64_live() == 0
    lo = W.apply(W.Model(n), "append", a1)
    lo = W.apply(lo, "reduce_peers", {"seed": 70, "k": 20, "root_only": 1, "position": 0})
    assert np.array_equal(lo.s, s + brute_gram(W.partner_rows(70, n, 20)) + brute_gram(W.partner_rows(71, n, 20)))
    assert not W.apply(lo, "reduce_peers", {"seed": 70, "k": 20, "root_only": 1, "position": 1}).s.any()


# ---- what the committed scripts cover ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trace():
    """per walk, per step: what the script data and the model say about it"""
    out = []
    for w in range(len(W.WALKS)):
        model, steps, max_call, caps = W.new_model(w), [], 0, {}
        for m, ma, kind, o, oa in W.steps_of(W.script(w)):
            before = {"n": model.n, "measure": model.measure, "bound": model.comp is not None, "max_call": max_call,
                      "s": model.s, "q": None if model.comp is None else model.comp.q.copy(), "zero": not model.s.any(),
                      "i64": model.i64_live()}
            regrown = {}
            if m == "append":
                for buf, need in W.buffer_needs(ma, model.n, W.rows_of(ma, model.n)[0]).items():
                    if need > caps.get(buf, 0):
                        regrown[buf] = (caps.get(buf, 0), need)           # (capacity it had, elements asked for)
                        caps[buf] = max(need, 1024)
            model = W.apply(model.copy(), m, ma)
            if m == "append":
                max_call = max(max_call, ma["k"])
            if m == "subset":
                max_call, caps = 0, {}                                     # a new ctx
            step = {"m": m, "ma": ma, "c": W.CLASS_OF[m], "refuse": kind, "o": o, "oa": oa, "before": before, "n": model.n,
                    "measure": model.measure, "bound": model.comp is not None, "degenerate": model.degenerate(), "model": model,
                    "i64": model.i64_live(), "consistent": model.consistent(), "regrown": regrown}
            if o == "compute":
                step["gaps"] = model.gaps_ok(oa["k"])
            steps.append(step)
        out.append(steps)
    return out


def flat(trace):
    return [s for steps in trace for s in steps]


def test_the_scripts_are_plain_data_and_the_same_every_time():
    assert len(W.WALKS) == 8 and sorted(set(w[1] for w in W.WALKS)) == [49, 65, 130, 260]
    assert set(w[2] for w in W.WALKS) == set(("auto", "fp4", "i8", "f32")) and set(w[3] for w in W.WALKS) == set(("bits", "fp4"))
    assert [w[4] for w in W.WALKS] == [None] * 6 + ["A", "B"]
    for w in range(len(W.WALKS)):
        assert ast.literal_eval(repr(list(W.script(w)))) == list(W.script(w))
        assert tuple(W.Planner(w).run()) == W.script(w)
        assert 36 <= len(W.steps_of(W.script(w))) <= W.STEPS_CAP + 2


def test_every_mutator_class_observer_pair_occurs(trace):
    seen = set((s["c"], s["o"]) for s in flat(trace))
    missing = [(c, o) for c in W.CLASSES for o in W.OBSERVERS if (c, o) not in seen]
    assert not missing, missing
    assert set(s["m"] for s in flat(trace)) == set(W.MUTATORS)


def test_every_observer_runs_under_each_measure_and_under_a_binding(trace):
    for kind in W.MEASURES:
        seen = set(s["o"] for s in flat(trace) if s["measure"] == kind and not s["bound"])
        assert seen == set(W.OBSERVERS), (kind, set(W.OBSERVERS) - seen)
    seen = set(s["o"] for s in flat(trace) if s["bound"])
    assert seen == set(W.OBSERVERS), set(W.OBSERVERS) - seen
    # a binding is inherited by a subset (an owned companion), and observed there
    assert any(s["bound"] and s["model"].comp.owned for s in flat(trace))
    assert all(s["consistent"] for s in flat(trace))
    # the mat-vec forms, form 1 only where it exists
    forms = set(s["oa"]["form"] for s in flat(trace) if s["o"] == "matvec")
    assert forms == set((0, 1, 2))
    assert all(s["n"] % 4 == 0 and not s["i64"] for s in flat(trace) if s["o"] == "matvec" and s["oa"]["form"] == 1)
    assert set(s["oa"]["k"] for s in flat(trace) if s["o"] == "compute") == set((1, 2, 5))


def test_every_input_form_is_read_by_every_reader_with_no_reader_between(trace):
    """a step is mutator, observer: the observer is the first call after the append, which is where a missing flush shows"""
    seen = set((s["ma"]["form"], s["o"]) for s in flat(trace) if s["m"] == "append" and s["ma"]["k"] > 0)
    missing = [(f, o) for f in W.READ_FORMS for o in W.READERS if (f, o) not in seen]
    assert not missing, missing
    assert any(s["m"] == "append" and s["ma"]["form"] == "empty" for s in flat(trace))
    assert set(s["ma"]["ref_is_a1"] for s in flat(trace) if s["m"] == "append" and s["ma"]["form"] in W.BED_FORMS) == set((False, True))
    assert all(s["before"]["bound"] for s in flat(trace) if s["m"] == "append" and s["ma"]["form"] == "bed_calls")
    for steps in trace:
        assert sum(s["ma"]["k"] for s in steps if s["m"] == "append") <= 3000
        assert max(s["ma"]["k"] for s in steps if s["m"] == "append") <= 400


def test_multiplicities_are_fed_where_the_kernel_takes_them_and_in_front_of_reset_load_and_subset(trace):
    for w, steps in enumerate(trace):
        appends = [s for s in steps if s["m"] == "append"]
        mult = [s for s in appends if s["ma"]["mult"]]
        capable = W.WALKS[w][2] in ("auto", "i8", "f32")
        assert bool(mult) == capable, w
        assert all(s["ma"]["form"] in W.MULT_FORMS and not s["before"]["bound"] for s in mult)
        # one append in six: every sixth append of an unbound engine (but the scripted empty call and the planned sequences)
        sixth = [s for i, s in enumerate(appends) if (i + 1) % 6 == 0 and not s["before"]["bound"] and s["ma"]["form"] != "empty"]
        if capable:
            assert sixth and sum(s["ma"]["mult"] for s in sixth) >= len(sixth) - 1, (w, [s["ma"] for s in sixth])
            assert 6 * len(mult) >= len([s for s in appends if not s["before"]["bound"]]) - 5, w
    # the redo in flight: multiplicities, then an observer that reads no S (a reader would flush through finalize_impl), then
    # the mutator -- in a walk whose kernel defers the contraction (auto: provisional FP4 chunks redone on int8; i8)
    after = set()
    for w, steps in enumerate(trace):
        if W.WALKS[w][2] not in ("auto", "i8"):
            continue
        for a, b in zip(steps[:-1], steps[1:]):
            if a["m"] == "append" and a["ma"]["mult"] and a["o"] in W.NON_READERS:
                after.add(b["c"])
    assert set(("reset", "load", "subset")) <= after, after


def test_the_pruner_road_is_walked_and_a_reset_falls_between_two_of_its_chunks(trace):
    """LdPruner(accumulate=True): the kept rows by ld_cohort.ld_rule; with the reset between the chunks the second chunk starts
    a window of its own (ld_drop_tail) and is all S holds"""
    import ld_cohort as LD
    lds = [s for s in flat(trace) if s["m"] == "append" and s["ma"]["form"] == "ld_prune"]
    assert set(s["o"] for s in lds) >= set(W.READERS)
    assert all(not s["before"]["bound"] and 0 < s["ma"]["cut"] < s["ma"]["k"] for s in lds)
    drops = [s for w, steps in enumerate(trace) for s in steps if s in lds and s["ma"]["reset_between"] and W.WALKS[w][4] is None]
    assert drops and any(s["ma"]["reset_between"] for s in lds if s not in drops)       # without a knob, and in a child
    removed = 0
    for s in lds:
        a, n = s["ma"], s["before"]["n"]
        x = W.rows_of(a, n)[0]
        cut, keep = W.ld_chunks(a, x)
        removed += int((~keep).sum())
        if a["reset_between"]:
            assert s["before"]["s"].any()                                               # there was an S to drop
            second = LD.ld_rule_banded(x[cut:], a["window"], a["r2"])                   # the band form of the rule, on the chunk alone
            assert np.array_equal(keep[cut:], second) and np.array_equal(s["model"].s, W.int_gram(x[cut:][second]))
            assert not np.array_equal(keep, LD.ld_rule(x, a["window"], a["r2"]))        # the carried rows would have mattered
        else:
            assert np.array_equal(keep, LD.ld_rule_banded(x, a["window"], a["r2"]))
            assert np.array_equal(s["model"].s, s["before"]["s"] + W.int_gram(x[keep]))
    assert removed > 100


def test_a_call_larger_than_any_before_arrives_with_a_measure_set_and_with_a_binding(trace):
    """the operand, tile and staging buffers of a ctx are sized by the largest call it has seen (floor 1,024): a call larger
    than every earlier one of the same ctx regrows them, here with the lazily allocated measure and companion buffers live"""
    # the buffers whose sizes are read off capi_accumulate.hip: `tile` leaves its floor of 1,024 elements and later its own
    # capacity with each measure set and under a binding; `csr_idx` does under a measure or a binding
    tiles = [s for s in flat(trace) if "tile" in s["regrown"] and s["regrown"]["tile"][0] >= 1024]
    assert set(s["before"]["measure"] for s in tiles if not s["before"]["bound"]) == set(W.MEASURES), tiles
    assert any(s["before"]["bound"] for s in tiles)
    assert any(s["regrown"]["tile"][0] == 0 and s["regrown"]["tile"][1] > 1024 for s in flat(trace) if "tile" in s["regrown"])
    idx = [s for s in flat(trace) if "csr_idx" in s["regrown"] and s["regrown"]["csr_idx"][1] > 1024]
    assert any(s["before"]["bound"] or s["before"]["measure"] != "shared" for s in idx), idx      # (past its floor, at least)
    grows = [s for s in flat(trace) if s["m"] == "append" and 0 < s["before"]["max_call"] < s["ma"]["k"]]
    assert set(s["before"]["measure"] for s in grows if not s["before"]["bound"]) == set(W.MEASURES)
    assert any(s["before"]["bound"] for s in grows)
    assert max(s["ma"]["k"] for s in grows) == 400
    for w, steps in enumerate(trace):
        assert any(s in grows for s in steps), w


def test_the_int64_part_comes_and_goes(trace):
    """S leaves int32 by a scaled load and comes back by a reset, a load and a subset; appends and reductions land on top of it"""
    fl = flat(trace)
    assert any(s["i64"] for s in fl) and any(s["m"] == "load" and s["ma"]["kind"] == "big" for s in fl)
    left = set(s["c"] for s in fl if s["before"]["i64"] and not s["i64"])
    assert set(("reset", "load")) <= left, left
    on_top = set(s["c"] for s in fl if s["before"]["i64"] and s["i64"])
    assert set(("append", "import")) <= on_top, on_top
    # load(beyond int32) -> reset -> append -> observer, in a walk without a knob: where gram_i64_live is asserted
    plain = [steps for w, steps in enumerate(trace) if W.WALKS[w][4] is None]
    assert any(a["i64"] and b["m"] == "reset" and c["m"] == "append" for steps in plain for a, b, c in zip(steps[:-2], steps[1:-1], steps[2:]))
    # two reductions of partials near 0.45 * 2^31 in a row: the first stays in int32, the second leaves it
    near = [(a, b) for steps in plain for a, b in zip(steps[:-1], steps[1:]) if a["m"] == b["m"] == "reduce_from" and a["ma"].get("near")]
    assert near and all(not a["i64"] and b["i64"] and b["ma"].get("near") for a, b in near)
    for s in fl:
        if s["m"] == "load" and s["ma"]["kind"] == "big":
            assert s["model"].s.max() > 2 ** 31 and s["model"].s.max() < 2 ** 53 // s["n"]


def test_degenerate_states_are_visited_and_few(trace):
    for w, steps in enumerate(trace):
        bad = [i for i, s in enumerate(steps) if s["degenerate"]]
        assert 10 * len(bad) <= len(steps), (w, bad)
    fl = flat(trace)
    assert any(not s["model"].s.any() for s in fl)
    assert any(s["model"].s.any() and (np.diagonal(s["model"].s) == 0).any() for s in fl)
    assert any(s["n"] == 32 for s in fl)
    assert set((97, 64, 33, 32)) <= set(s["n"] for s in fl)
    assert any(s["m"] == "load" and s["ma"]["kind"] == "zero" for s in fl)
    assert any(s["m"] == "reduce_peers" and s["ma"]["root_only"] and s["ma"]["position"] == 1 for s in fl)
    assert any(s["m"] == "reduce_peers" and s["ma"]["root_only"] and s["ma"]["position"] == 0 for s in fl)
    assert any(s["m"] == "reduce_peers" and not s["ma"]["root_only"] for s in fl)


def test_spectra_without_the_gap_are_few(trace):
    computes = [s for s in flat(trace) if s["o"] == "compute"]
    without = [s for s in computes if not s["gaps"]]
    assert len(computes) >= 30 and 10 * len(without) <= len(computes), (len(without), len(computes))


def test_refused_calls_are_few_of_every_kind_and_their_preconditions_hold(trace):
    kinds = set()
    for w, steps in enumerate(trace):
        refused = [s for s in steps if s["refuse"]]
        assert 10 * len(refused) <= len(steps), w
        for s in refused:
            kinds.add(s["refuse"])
            m = s["model"]
            if s["refuse"] == "jaccard_on_bound":
                assert m.comp is not None
            if s["refuse"] == "bind_on_measured":
                assert m.comp is None and m.measure != "shared"
            if s["refuse"] == "bind_low_v":
                assert m.comp is not None and np.diagonal(m.comp.q).max() >= 1
    assert kinds == set(W.REFUSALS), set(W.REFUSALS) - kinds


def test_every_screen_has_pairs_on_both_sides_of_its_cut(trace):
    """the rule is exact on both sides (integers and one product): no tie-break is needed, only pairs to find and to leave"""
    checked = 0
    caps = set()
    for s in flat(trace):
        if s["o"] != "pairs":
            continue
        m, cut = s["model"], s["oa"]["min_jaccard"]
        assert 0 < cut <= 1
        found = int(m.expect("pairs", s["oa"]).exact["found"][0])
        caps.add("none" if s["oa"]["capacity"] == 0 else "less" if s["oa"]["capacity"] < found else "all")
        if not m.s.any():
            continue
        d = np.diagonal(m.s)
        u = (d[:, None] + d[None, :] - m.s)[np.triu_indices(m.n, 1)]
        assert 0 < found < int((u > 0).sum()), (s["oa"], found)
        checked += 1
    assert checked >= 20 and caps == set(("none", "less", "all")), (checked, caps)


def test_the_neutral_calls_and_the_companion_calls_occur(trace):
    fl = flat(trace)
    assert set(s["ma"]["to"] for s in fl if s["m"] == "set_stream") == set(("torch", "null"))
    assert any(s["m"] == "reserve" and s["ma"]["variants"] and s["ma"]["num_pc"] for s in fl)
    binds = [s for s in fl if s["m"] == "bind"]
    assert any(s["ma"]["fresh"] for s in binds) and any(s["ma"]["v"] is None for s in binds)
    assert any(not s["ma"]["fresh"] and s["ma"]["v"] is not None and s["before"]["bound"] for s in binds)
    kinds = set(s["ma"]["kind"] for s in fl if s["m"] == "set_similarity")
    assert kinds == set(W.MEASURES)
    assert any(s["m"] == "set_similarity" and s["ma"]["kind"] == s["before"]["measure"] for s in fl)
    # reset keeps the measure and the binding: both are observed directly behind one
    assert any(s["m"] == "reset" and s["measure"] != "shared" for s in fl) and any(s["m"] == "reset" and s["bound"] for s in fl)

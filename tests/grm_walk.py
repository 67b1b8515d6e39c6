"""What the walks over a GRM ctx share (no test here, no GPU): a numpy model of the state of a GRM ctx, the
seeded generator of the walks -- long random sequences of calls as plain data -- and the summation bound of an entry of K.

Everything a GRM ctx returns is documented to be a function of the store's rows, min_maf, the installed keep mask and the
call's arguments alone (include/pcoa.h).  The model holds exactly that and answers through the numpy
twins the GRM tests already have; tests/test_grm_walk_cpu.py holds the model and the scripts, tests/test_gpu_grm_walk.py walks
an engine through a script and compares it, at every observer, with a fresh engine brought straight to the model's state.

A script is a list of (op, arguments): a step is one mutator, at most one ("refuse", ...) and one observer, in that order."""
import functools

import numpy as np

import grm_ld_cohort as LD
from conftest import load_pkg
from grm_subset_cohort import SWAP, pack_rows, spec_grm_subset_rows, unpack_rows
from test_gpu_grm_pairs import gap_cutoff
from test_gpu_grm_project import FOUR_ROUNDINGS, t_bound
from test_grm_cpu import dense_k, dosage, edge_rows, random_codes, spec_grm_bound, spec_grm_called_samples, spec_grm_counts, \
    spec_grm_matvec, spec_grm_weights
from test_grm_project_cpu import scale_weights, spec_grm_project, spec_grm_project_bound, spec_grm_t

MUTATORS = ("append", "reset", "min_maf_new", "min_maf_same", "ld_prune", "ld_clear", "subset_panel", "subset_study")
OBSERVERS = ("info", "rows", "ld_mask", "matvec", "block", "pairs", "weights", "project", "compute")
REFUSALS = ("rect_outside", "band_63", "keep_not_increasing", "min_maf_half", "project_other_v")
DROPPERS = ("append", "reset", "min_maf_new", "ld_clear")          # what drops an installed mask (include/pcoa.h, "Lifetime")
RESIDENT_AFTER = ("info", "matvec", "block", "pairs", "weights", "project", "compute")   # observers that leave counts and weights resident
FORMS = ("host", "ragged", "device", "empty")
THRESHOLDS = (256, 512, 1024)      # V at which grm_cnt (4 V > 1,024), grm_par (1 + 2 V > 1,024) and grm_keep (V > 1,024) regrow
MAFS = (0.0, 0.02, 0.05, 0.1)
MIN_GAP = 0.01                     # the relative gaps test_grm_cpu.py asks of a cohort whose eigenvectors are compared

# (seed, the first N, PCOA_GRM_SEGMENT_ROWS or None, every threshold crossed with a mask installed)
WALKS = [(11, 130, None, True), (12, 65, None, False), (13, 49, None, False), (14, 260, None, True), (15, 130, None, False),
         (16, 260, None, False), (17, 130, 96, False)]
PANEL_SIZES = (97, 64, 33, 32)              # subset_panel takes N down through these,
SEGMENT_PANEL_SIZES = (65, 33, 32)          # and through these in the walk over short segments
STUDY_SIZES = (1, 15, 17, 33)
DECK_SEED = 2024
STEPS = 40                                  # steps of a walk, more where its share of the deck needs them
STEPS_CAP = 56
DEGENERATE_BUDGET = 3                       # of a walk's observer steps (at most 10 %: tests/test_grm_walk_cpu.py)
SEQUENCES = [[("block", "pairs")], [("pairs", "block")], [("weights", "project")], [("project", "weights")], [("block", "pairs")],
             [("weights", "project")], [("pairs", "block"), ("project", "weights")]]


def entry_bound(codes, ref_is_a1, min_maf, n_pairs, divisor):
    """(V + 16) 2^-52 (|A|^T diag(d) |A|)_ij / divisor_ij: the standard bound of a sum of V products, each rounded after the
    scaling by d, the 16 covering the roundings of mu, d and the division, doubled to cover numpy's own error."""
    g, c = dosage(codes, ref_is_a1)
    mu, d, used, m = spec_grm_weights(spec_grm_counts(codes, ref_is_a1), min_maf)
    a = np.abs(np.where(c == 1, g.astype(np.float64) - mu[:, None], 0.0))
    w = (a.T * d) @ a
    with np.errstate(divide="ignore", invalid="ignore"):
        w = w / float(m) if divisor == "used" else np.where(n_pairs > 0, w / n_pairs.astype(np.float64), 0.0)
    return (codes.shape[0] + 16) * 2.0 ** -52 * w


# ---- the model ------------------------------------------------------------------------------------------------------------------
class Expected(object):
    """What one observer must return.  error: (the name of the PCOA_ERR_* code, a word of its message) or None; exact: name ->
    array that must be equal; close: name -> (array, bound per entry); note: what only the caller can check."""

    def __init__(self, error=None, exact=None, close=None, note=None):
        self.error, self.exact, self.close, self.note = error, exact or {}, close or {}, note or {}


class Model(object):
    """A GRM ctx as the header defines its answers: the code matrix [V][N] in the store's coding (a .bed row with ref_is_a1 = 1),
    min_maf, the installed prune (window, r2, breaks) or None, and the kind (panel, or a study store without weights)."""

    def __init__(self, n, study=False, codes=None, min_maf=0.0):
        self.n, self.study, self.min_maf, self.prune = int(n), bool(study), float(min_maf), None
        self.codes = np.zeros((0, self.n), dtype=np.uint8) if codes is None else np.ascontiguousarray(codes, dtype=np.uint8)
        self._memo = {}

    @property
    def v(self):
        return self.codes.shape[0]

    # -- mutators
    def append(self, codes, ref_is_a1):
        """rows as they are fed; the store keeps them with 11 the homozygous non-reference code.  An empty call changes nothing."""
        if codes.shape[0] == 0:
            return
        self.codes = np.concatenate([self.codes, codes if ref_is_a1 else SWAP[codes]], axis=0)
        self.prune, self._memo = None, {}

    def reset(self):
        self.codes, self.prune, self._memo = np.zeros((0, self.n), dtype=np.uint8), None, {}

    def set_min_maf(self, maf):
        if float(maf) != self.min_maf:
            self.min_maf, self.prune, self._memo = float(maf), None, {}

    def ld_prune(self, window, r2, breaks=()):
        self.prune, self._memo = (int(window), float(r2), tuple(int(b) for b in breaks)), {}

    def ld_clear(self):
        self.prune, self._memo = None, {}

    def subset(self, keep, study):
        """pcoa_create_grm_subset: the rows of the kept samples by spec_grm_subset_rows, the source's min_maf, no mask."""
        keep = np.asarray(keep, dtype=np.int64)
        rows = spec_grm_subset_rows(pack_rows(self.codes), self.n, keep)
        return Model(keep.size, study, unpack_rows(rows, keep.size), self.min_maf)

    # -- the state behind the answers
    def _once(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def mask(self):
        """The keep mask of the installed prune (grm_ld_cohort's rule, its band form), or None."""
        if self.prune is None:
            return None

        def make():
            w, t, breaks = self.prune
            g = np.array([0, -1, 1, 2], dtype=np.int8)[self.codes]
            return LD.greedy_band(LD.exceeds_band(g, w, t), LD.candidates(g, self.min_maf), w, breaks)
        return self._once("mask", make)

    def effective(self):
        """The rows as the consumers see them: the mask enters used_v, so a removed row counts like a row nobody
        is called at -- unused, d = 0, no share in any n(i, j) -- while V, and with it every summation bound, stays the store's."""
        def make():
            keep = self.mask()
            if keep is None:
                return self.codes
            eff = self.codes.copy()
            eff[~keep] = 1
            return eff
        return self._once("effective", make)

    def weights(self):
        return self._once("weights", lambda: spec_grm_weights(spec_grm_counts(self.effective(), True), self.min_maf))

    def used(self):
        return 0 if self.study else self.weights()[3]

    def dense(self, divisor):
        """(K, n) of variants_pca.grm_dense_rule, None where M' = 0."""
        rule = load_pkg("variants_pca").grm_dense_rule
        return self._once(("dense", divisor), lambda: rule(self.effective(), True, self.min_maf, divisor) if self.used() else None)

    def dense_bound(self, divisor):
        return self._once(("bound", divisor), lambda: entry_bound(self.effective(), True, self.min_maf, self.dense(divisor)[1], divisor))

    def spectrum(self):
        return self._once("spectrum", lambda: np.linalg.eigh(dense_k(self.effective(), True, self.min_maf)))

    # -- the observers
    def expect(self, op, a, study=None):
        """Expected of observer `op` with arguments `a` (study: the Model of the walk's study store, where there is one)."""
        v, m = self.v, self.used()
        if op == "info":
            return Expected(exact={"info": np.array([v, m], dtype=np.int64),
                                   "counts": spec_grm_counts(self.codes, True)[a["first"]:a["first"] + a["n"]]})
        if op == "rows":
            return Expected(exact={"rows": pack_rows(self.codes)[a["first"]:a["first"] + a["n"]]})
        if op == "ld_mask":
            if self.prune is None:
                return Expected(error=("PCOA_ERR_STATE", "no keep mask"))
            return Expected(exact={"mask": self.mask()[a["first"]:a["first"] + a["n"]]})
        if op == "matvec":
            x = vectors_of(a["seed"], self.n, 1)[0][:, 0]
            eff = self.effective()
            return Expected(close={"y": (spec_grm_matvec(eff, True, x, self.min_maf), spec_grm_bound(eff, True, x, self.min_maf))})
        if op == "block":
            if m == 0:
                return Expected(error=("PCOA_ERR_STATE", "none of the"))
            r0, r, c0, c = a["rect"]
            k, cnt = self.dense(a["divisor"])
            out = Expected(close={"k": (k[r0:r0 + r, c0:c0 + c], self.dense_bound(a["divisor"])[r0:r0 + r, c0:c0 + c])})
            if a["pairs"]:
                out.exact["n"] = cnt[r0:r0 + r, c0:c0 + c].astype(np.int32)
            return out
        if op == "pairs":
            if m == 0:
                return Expected(error=("PCOA_ERR_STATE", "none of the"))
            k, cnt = self.dense(a["divisor"])
            want = load_pkg("variants_pca").grm_pairs_rule(k, a["cutoff"], cnt if a["divisor"] == "pairwise" else m)
            cap = capacity_of(a["capacity"], self.n)
            listed = want[:min(want.size, cap)]
            bound = self.dense_bound(a["divisor"])
            return Expected(exact={"found": np.array([want.size], dtype=np.int64), "i": listed["i"], "j": listed["j"], "n": listed["n"]},
                            close={"k": (listed["k"], bound[listed["i"], listed["j"]])})
        if op == "weights":
            if m == 0:
                return Expected(error=("PCOA_ERR_INVALID_ARG", "M' = 0"))
            comps, lam = vectors_of(a["seed"], self.n, a["num_pc"])
            eff = self.effective()
            sl = slice(a["first"], a["first"] + a["n"])
            t, tb = spec_grm_t(eff, True, comps, self.min_maf), t_bound(eff, True, comps, self.min_maf)
            if not a["scaled"]:
                return Expected(close={"w": (t[sl], tb[sl])})
            # w = used ? t / s : 0 with s = sqrt(d ((double)M' lambda)): t carries t_bound, s its three roundings and the quotient a
            # fourth, so |w - twin| <= t_bound / s + FOUR_ROUNDINGS |twin| -- the two bounds of tests/test_gpu_grm_project.py, added
            mu, d, used, _ = self.weights()
            w = scale_weights(t, d, used, m, lam)
            with np.errstate(divide="ignore", invalid="ignore"):
                wb = np.where(used[:, None], tb / np.sqrt(d[:, None] * (float(m) * lam[None, :])), 0.0) + FOUR_ROUNDINGS * np.abs(w)
            return Expected(close={"w": (w[sl], wb[sl])})
        if op == "project":
            other = self if a["study"] == "self" else study
            if other.v != v:
                return Expected(error=("PCOA_ERR_STATE", "same variants"))
            if m == 0:
                return Expected(error=("PCOA_ERR_INVALID_ARG", "M' = 0"))
            comps, lam = vectors_of(a["seed"], self.n, a["num_pc"])
            eff = self.effective()
            xy, called = spec_grm_project(eff, True, other.codes, True, comps, lam, self.min_maf)
            return Expected(exact={"called": called},
                            close={"coords": (xy, spec_grm_project_bound(eff, True, other.codes, True, comps, lam, self.min_maf))})
        if op == "compute":
            if m == 0:
                return Expected(error=("PCOA_ERR_STATE", "K is undefined"))
            lam, vec = self.spectrum()
            k = a["num_pc"]
            top = lam[::-1]
            gaps = all((top[c] - top[c + 1]) / top[0] >= MIN_GAP for c in range(k))
            return Expected(exact={"nonzero": np.array([spec_grm_called_samples(self.effective(), True, self.min_maf)], dtype=np.int64)},
                            note={"eigenvalues": top[:k].copy(), "vectors": np.ascontiguousarray(vec[:, ::-1][:, :k]) if gaps else None})
        raise ValueError("no observer %r" % (op,))

    def degenerate(self, op, a, study=None):
        """A step that only checks what the header documents for an empty or unusable state."""
        return self.v == 0 or self.expect(op, a, study).error is not None


class State(object):
    """The panel a walk is on and its study store (None until a subset_study)."""

    def __init__(self, n):
        self.panel, self.study = Model(n), None

    def apply(self, op, a):
        p = self.panel
        if op == "append":
            p.append(rows_of(a, p.n), a["ref_is_a1"])
        elif op == "reset":
            p.reset()
        elif op in ("min_maf_new", "min_maf_same"):
            p.set_min_maf(a["maf"])
        elif op == "ld_prune":
            p.ld_prune(a["window"], a["r2"], a["breaks"])
        elif op == "ld_clear":
            p.ld_clear()
        elif op == "subset_panel":
            self.panel = p.subset(keep_of(a, p.n), False)
        elif op == "subset_study":
            self.study = p.subset(keep_of(a, p.n), True)
        else:
            raise ValueError("no mutator %r" % (op,))


# ---- what a script's arguments stand for ------------------------------------------------------------------------------------
def rows_of(a, n):
    """[k][n] codes of an append as they are fed (random_codes with 5 % missing; edge: test_grm_cpu.edge_rows on top)."""
    rng = np.random.default_rng(a["seed"])
    codes = random_codes(rng, a["k"], n, missing=0.05)
    return edge_rows(codes) if a["edge"] and a["k"] > 0 else codes


def keep_of(a, n):
    if a["size"] == n:
        return np.arange(n, dtype=np.int32)
    return np.sort(np.random.default_rng(a["seed"]).choice(n, size=a["size"], replace=False)).astype(np.int32)


def vectors_of(seed, n, k):
    """(components [n][k], eigenvalues [k]) of a weights / project step and the x of a product: any vectors will do."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, k)), rng.uniform(0.5, 3.0, size=k)


def capacity_of(kind, n):
    return n * n if kind == "all" else int(kind)


def block_doubles(a):
    return a["rect"][1] * a["rect"][3]


def pairs_doubles(a, n):
    """the band of pcoa_grm_pairs in the ctx's block buffer: band_rows x 64 ceil(N / 64) (include/pcoa.h, "memory")"""
    return (a["band_rows"] or 1024) * 64 * (-(-n // 64))


def steps_of(script):
    """[(mutator, its arguments, refusal kind or None, observer, its arguments)]"""
    out, i = [], 0
    while i < len(script):
        (m, ma), i = script[i], i + 1
        assert m in MUTATORS, m
        kind = None
        if script[i][0] == "refuse":
            kind, i = script[i][1]["kind"], i + 1
        (o, oa), i = script[i], i + 1
        assert o in OBSERVERS, o
        out.append((m, ma, kind, o, oa))
    return out


def crosses(v0, v1, t):
    """an append from v0 to v1 rows takes the store over threshold t: landed short of it, then at least one row past it"""
    return v0 < t < v1


# ---- the generator --------------------------------------------------------------------------------------------------------------
def inherently_degenerate(m, o):
    """pairs whose observer can only see an empty store or a missing mask"""
    return m == "reset" or (o == "ld_mask" and m in ("append", "min_maf_new", "ld_clear", "subset_panel"))


@functools.lru_cache(maxsize=None)
def hands():
    """The deck of all (mutator, observer) pairs, shuffled and dealt to the walks; the degenerate pairs go round first, so no walk
    holds more than two of them."""
    rng = np.random.default_rng(DECK_SEED)
    deck = [(m, o) for m in MUTATORS for o in OBSERVERS]
    deck = [deck[i] for i in rng.permutation(len(deck))]
    deck = [p for p in deck if inherently_degenerate(*p)] + [p for p in deck if not inherently_degenerate(*p)]
    out = [[] for _ in WALKS]
    for i, p in enumerate(deck):
        out[i % len(WALKS)].append(p)
    return tuple(tuple(out[w][i] for i in rng.permutation(len(out[w]))) for w in range(len(WALKS)))


class Planner(object):
    """Writes the script of one walk.  It runs the model alongside, so every step is chosen for the state it meets: its hand of
    the deck first, where the state lets the pair mean something (a dropper with a mask to drop, ld_mask with a mask to read);
    appends paced so that V lands a few rows short of each threshold behind an observer that leaves the weights resident and
    crosses it in the next step; the pairs of observers that hand a shared buffer over; fill otherwise."""

    def __init__(self, index):
        seed, n0, segment, masked = WALKS[index]
        self.sizes = SEGMENT_PANEL_SIZES if segment else PANEL_SIZES
        self.rng = np.random.default_rng(seed)
        self.seed, self.masked = seed, masked
        self.state = State(n0)
        self.wanted = list(hands()[index])
        self.sequences = list(SEQUENCES[index])
        self.script, self.queue = [], []
        self.nsteps = self.degenerate = self.appends = 0
        self.refusals = index
        self.since_append, self.prev_obs, self.next_seed = 99, None, 1000 * seed
        self.refused, self.extras = set(), ["plain_maf", "reprune"]

    # -- small draws
    def draw_seed(self):
        self.next_seed += 1
        return self.next_seed

    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    @property
    def panel(self):
        return self.state.panel

    def has_mask(self):
        return self.panel.prune is not None

    def next_threshold(self):
        return next((t for t in THRESHOLDS if self.panel.v < t - 2), None)

    def room_to_append(self):
        """a few rows fit without coming within three rows of the next threshold: crossings are planned, never met"""
        t = self.next_threshold()
        return t is None or t - 3 - self.panel.v >= 1

    def fill_observer(self, resident=False):
        pool = [o for o in (RESIDENT_AFTER if resident else OBSERVERS) if o != "ld_mask" or self.has_mask()]
        return self.pick(pool)

    def take_wanted(self, mutator, resident=False):
        """an observer the deck still wants after `mutator`, where the state allows the pair"""
        for p in self.wanted:
            if p[0] == mutator and self.feasible(p) and (not resident or p[1] in RESIDENT_AFTER):
                self.wanted.remove(p)
                return p[1]
        return self.fill_observer(resident)

    def feasible(self, p):
        m, o = p
        room = self.degenerate < DEGENERATE_BUDGET
        if m != "append" and self.panel.v == 0:
            return False
        if m == "reset":
            return self.has_mask() and room and self.nsteps >= 4
        if m == "append" and not self.room_to_append():
            return False
        if m in ("append", "min_maf_new", "ld_clear", "subset_panel"):   # the deck's copy of a dropper runs with a mask to drop
            return self.has_mask() and (o != "ld_mask" or room)
        if m in ("min_maf_same", "subset_study"):
            return o != "ld_mask" or self.has_mask()
        return self.panel.v >= 8                                         # ld_prune

    # -- one step
    def choose(self):
        v, t = self.panel.v, self.next_threshold()
        if v == 0 and self.rng.random() < 0.5:                           # a short store first: the states below the first threshold
            return "append", self.fill_observer(True), {"k": int(self.rng.integers(40, 200))}
        if t is None and self.since_append >= 3 and 1024 < v < 1300:      # past the last threshold: on to about 1,300 rows
            return "append", self.take_wanted("append"), {"k": int(self.rng.integers(60, 140))}
        if v == 0 or (t is not None and self.since_append >= 2):
            land = t - int(self.rng.integers(3, 9)) - v
            self.queue = [("append", None, {"cross": t})]                # land short of the threshold, then cross it
            if self.masked:
                self.queue.insert(0, ("ld_prune", None, {"resident": True}))
            if land >= 1:
                return "append", self.take_wanted("append", resident=True) if v else self.fill_observer(True), {"k": land}
            return self.pick(("min_maf_same", "subset_study")), self.fill_observer(True), {}   # (already short of it)
        if self.extras and self.nsteps >= 8 and self.prev_obs in RESIDENT_AFTER and self.panel.used() > 0:
            # once a walk: min_maf changes under resident weights with no mask to drop (the weights alone go stale), and a prune
            # runs over an installed mask (the candidates are judged without it, the weights must not keep either state)
            for extra, m, ok in (("plain_maf", "min_maf_new", not self.has_mask()), ("reprune", "ld_prune", self.has_mask())):
                if extra in self.extras and ok:
                    self.extras.remove(extra)
                    return m, self.fill_observer(True), {}
        if self.sequences and self.nsteps >= 6 and self.panel.used() > 0:
            first, second = self.sequences.pop(0)
            self.queue = [("append", second, {"empty": True, "after": first})]
            return self.pick(("min_maf_same", "subset_study", "ld_prune")), first, {"before": second}
        for p in self.wanted:
            if self.feasible(p):
                self.wanted.remove(p)
                return p[0], p[1], {}
        if self.wanted and not self.has_mask() and v >= 8:                # what is left of the hand needs a mask to drop
            return "ld_prune", self.fill_observer(), {}
        m = self.pick(("append", "append", "ld_prune", "ld_prune", "min_maf_new", "min_maf_same", "ld_clear", "subset_study"))
        if m == "append" and not self.room_to_append():
            m = "ld_prune"
        if m == "ld_prune" and v < 8:
            m = "min_maf_same"
        return m, self.fill_observer(), {}

    def mutator_args(self, m, hint):
        p, rng = self.panel, self.rng
        if m == "append":
            if hint.get("empty"):
                return {"k": 0, "seed": 0, "edge": False, "form": "empty", "ref_is_a1": False}
            v = p.v
            if "cross" in hint:
                k = hint["cross"] + int(rng.integers(1, 10)) - v
            elif "k" in hint:
                k = hint["k"]
            else:
                t = self.next_threshold()
                if t is not None:
                    k = max(1, min(int(rng.integers(1, 13)), t - 3 - v))
                else:
                    k = int(rng.integers(1, 13)) if v < 1300 else 1
            self.appends += 1
            return {"k": int(k), "seed": self.draw_seed(), "edge": bool(k >= 5 and rng.random() < 0.4),
                    "form": FORMS[(self.appends - 1) % 3], "ref_is_a1": bool(rng.random() < 0.5)}
        if m == "reset" or m == "ld_clear":
            return {}
        if m == "min_maf_new":
            return {"maf": self.pick([x for x in MAFS if x != p.min_maf])}
        if m == "min_maf_same":
            return {"maf": p.min_maf}
        if m == "ld_prune":
            v = p.v
            window = self.pick((1, 7, 20) if v > 400 else (1, 7, 64, 65))
            nb = int(rng.integers(0, 4)) if v > 8 else 0
            breaks = sorted(set(int(b) for b in rng.integers(1, v, size=nb))) if nb else []
            return {"window": int(window), "r2": float(self.pick((0.005, 0.01, 0.02, 0.05))), "breaks": breaks}
        if m == "subset_panel":
            size = next((s for s in self.sizes if s < p.n), p.n)
            return {"size": int(size), "seed": self.draw_seed()}
        if m == "subset_study":
            return {"size": int(min(self.pick(STUDY_SIZES), p.n)), "seed": self.draw_seed()}
        raise ValueError(m)

    def window(self):
        v = self.panel.v
        if v == 0:
            return 0, 0
        if self.rng.random() < 0.3:
            return 0, v
        first = int(self.rng.integers(0, v))
        return first, int(self.rng.integers(1, min(v - first, 300) + 1))

    def observer_args(self, o, hint):
        p, rng, n = self.panel, self.rng, self.panel.n
        if o in ("info", "rows", "ld_mask"):
            first, cnt = self.window()
            return {"first": first, "n": cnt}
        if o == "matvec":
            return {"seed": self.draw_seed()}
        if o == "block":
            if hint.get("before") == "pairs":
                rect = (0, n, 0, n)                                       # the largest block, in front of a band of 64 rows
            elif hint.get("after") == "pairs" or rng.random() < 0.6:
                r0, c0 = int(rng.integers(0, n)), int(rng.integers(0, n))
                rect = (r0, int(rng.integers(1, min(n - r0, 40) + 1)), c0, int(rng.integers(1, min(n - c0, 40) + 1)))
            else:
                rect = (0, n, 0, n)
            return {"rect": rect, "divisor": self.pick(("used", "pairwise")), "pairs": bool(rng.random() < 0.6 or "before" in hint),
                    "device": bool(rng.random() < 0.5)}
        if o == "pairs":
            divisor = self.pick(("used", "pairwise"))
            band = 64 if hint.get("after") == "block" else 0 if hint.get("before") == "block" else self.pick((0, 64, 128))
            cutoff = 0.05
            if p.used() > 0:
                upper = p.dense(divisor)[0][np.triu_indices(n, 1)]          # a target in the upper tail of this K, then the widest gap near it
                near = float(np.quantile(upper, self.pick((0.9, 0.99, 0.999))))
                cutoff = gap_cutoff(upper, near if near > 0 else 0.02)
            return {"cutoff": float(cutoff), "divisor": divisor, "band_rows": int(band), "capacity": self.pick((0, 1, "all", "all"))}
        if o == "weights":
            first, cnt = self.window()
            return {"scaled": bool(rng.random() < 0.5), "first": first, "n": cnt, "num_pc": int(rng.integers(1, 4)), "seed": self.draw_seed()}
        if o == "project":
            s = self.state.study
            own = s is None or s.v != p.v or rng.random() < 0.25
            return {"study": "self" if own else "study", "num_pc": int(rng.integers(1, 4)), "seed": self.draw_seed()}
        if o == "compute":
            return {"num_pc": 2}
        raise ValueError(o)

    def refusal(self):
        """every eleventh step refuses a call in front of its observer: host-side refusals, nothing a kernel would see"""
        if self.nsteps % 11 != 6 or self.panel.v == 0:
            return None
        s = self.state.study
        if s is not None and s.v != self.panel.v and "project_other_v" not in self.refused:
            kind = "project_other_v"
        else:
            kind = REFUSALS[self.refusals % 4]
            self.refusals += 1
        self.refused.add(kind)
        return kind

    def step(self):
        m, o, hint = self.queue.pop(0) if self.queue else self.choose()
        if m == "ld_prune" and hint.get("resident"):
            o = self.take_wanted("ld_prune", resident=True)
        if o is None:
            o = self.take_wanted(m)
        if (m, o) in self.wanted and self.feasible((m, o)):
            self.wanted.remove((m, o))
        v0 = self.panel.v
        ma = self.mutator_args(m, hint)
        self.state.apply(m, ma)
        self.script.append((m, ma))
        self.since_append = 0 if m == "append" and ma["k"] > 0 else self.since_append + 1
        kind = self.refusal()
        if kind:
            self.script.append(("refuse", {"kind": kind}))
        oa = self.observer_args(o, hint)
        self.script.append((o, oa))
        self.degenerate += bool(self.panel.degenerate(o, oa, self.state.study))
        self.prev_obs, self.nsteps = o, self.nsteps + 1
        for t in THRESHOLDS:
            assert not (m == "append" and crosses(v0, self.panel.v, t)) or "cross" in hint, (self.seed, self.nsteps, v0, self.panel.v)

    def run(self):
        while (self.nsteps < STEPS or self.wanted or self.sequences or self.queue or self.extras) and self.nsteps < STEPS_CAP:
            self.step()
        return self.script


@functools.lru_cache(maxsize=None)
def script(index):
    """The walk WALKS[index] as a tuple of (op, arguments)."""
    return tuple(Planner(index).run())


def replay(index, upto=None):
    """The State after the first `upto` ops of a script (all of them by default)."""
    st = State(WALKS[index][1])
    for op, a in script(index)[:upto]:
        if op in MUTATORS:
            st.apply(op, a)
    return st

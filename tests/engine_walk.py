"""What the walks over a carrier-count engine share (no test here, no GPU): a numpy model of the state of a full engine
(DESIGN.md 4.23), the seeded generator of the walks -- long random sequences of calls as plain data -- and the expected answer of
every observer, through the numpy statements and the bounds the section tests already have.

Everything a full engine returns is documented to be a function of the TOTAL integer matrix S, the measure set, the bound
companion's matrix Q with its V, and the call's arguments alone (include/pcoa.h).  The model holds exactly that;
tests/test_engine_walk_cpu.py holds the model and the scripts, tests/test_gpu_engine_walk.py walks an engine through a script and
compares it, at every observer, with a fresh engine brought straight to the model's state.

A script is a list of (op, arguments): a step is one mutator, at most one ("refuse", ...) and one observer, in that order."""
import functools

import numpy as np

import complete_cohort as C
import measure_cohort as M
from conftest import int_gram, load_oracle, load_pkg, planted_callsets
from ld_cohort import ld_cohort, ld_rule
from loadings_cohort import loadings_rule, summation_bound

INT32_MAX = 2 ** 31 - 1
CLASSES = ("append", "reset", "load", "import", "reduce", "subset", "measure", "binding")
CLASS_OF = {"append": "append", "reset": "reset", "load": "load", "export_import": "import", "reduce_from": "reduce",
            "reduce_peers": "reduce", "subset": "subset", "set_similarity": "measure", "bind": "binding",
            "companion_append": "binding", "companion_reset": "binding", "reserve": "neutral", "set_stream": "neutral"}
MUTATORS = tuple(CLASS_OF)
OBSERVERS = ("gram", "gram_block", "export", "pairs", "center", "matvec", "compute", "loadings", "getters")
READERS = ("gram", "gram_block", "export", "pairs", "center", "matvec", "compute")      # the observers that read S
NON_READERS = ("loadings", "getters")             # these leave buffered operand generations in flight for the next mutator
# input forms of an append.  bed_calls feeds the engine and its companion from one read, so it exists under a binding only;
# ld_prune feeds two chunks through LdPruner(accumulate=True), the kept rows by ld_cohort.ld_rule, outside a binding only
FORMS = ("f32_host", "f32_dev", "u8_host", "u8_dev", "bits_host", "bits_dev", "csr_host", "csr_pinned", "csr_dev", "bed_host",
         "bed_dev", "bed_calls", "ld_prune", "ragged", "empty")
READ_FORMS = tuple(f for f in FORMS if f != "empty")     # an empty call queues nothing a reader could miss
MULT_FORMS = ("f32_host", "f32_dev", "u8_host", "u8_dev")                                # the forms that carry multiplicities
BED_FORMS = ("bed_host", "bed_dev", "bed_calls")
MEASURES = ("shared", "jaccard", "cosine")
REFUSALS = ("index_n", "block_outside", "compute_0", "compute_n1", "keep_repeat", "min_jaccard_0", "similarity_unknown",
            "jaccard_on_bound", "bind_on_measured", "bind_self", "bind_low_v")
GENERIC_REFUSALS = REFUSALS[:7] + ("bind_self",)
MIN_GAP = 0.01                     # the relative gap asked of a spectrum whose eigenvectors are compared
POPS = 6                           # planted populations: five structure eigenvalues above the bulk, so compute(5) has gaps
BIG_SCALE = 2 ** 27                # a seeded Gram times this leaves int32 and stays exact in fp64 (asserted in big_gram)
LOAD_ROWS = 200

# (seed, the first N, gram_kernel, operand, child environment or None)
WALKS = [(21, 130, "auto", "bits", None), (22, 65, "fp4", "bits", None), (23, 49, "i8", "bits", None),
         (24, 260, "f32", "bits", None), (25, 130, "auto", "fp4", None), (26, 260, "auto", "bits", None),
         (27, 130, "auto", "bits", "A"), (28, 65, "auto", "bits", "B")]
CHILD_ENV = {"A": {"PCOA_DEBUG_FOLD_THRESHOLD": "200", "PCOA_DEBUG_MAX_LAUNCH": "64", "PCOA_DEBUG_PACK_CHUNK": "256"},
             "B": {"PCOA_NO_NARROW": "1", "PCOA_DEBUG_FOLD_THRESHOLD": "200"}}
SIZES = (97, 64, 33, 32)           # subset takes N down through these
STEPS = 44
STEPS_CAP = 64
DEGENERATE_BUDGET = 4              # of a walk's observer steps (at most 10 %: tests/test_engine_walk_cpu.py)
DECK_SEED = 2025
MAX_ROWS = 2900                    # cumulative rows fed over a walk
CALL_SIZES = (17, 33, 40, 64, 100, 130, 200, 257, 320, 400)
# the order of a walk's segments: what the engine decomposes while the steps of the segment run
SEGMENTS = [("shared", "jaccard", "bound", "cosine"), ("jaccard", "bound", "shared", "cosine"), ("cosine", "shared", "bound", "jaccard"),
            ("bound", "cosine", "jaccard", "shared"), ("shared", "bound", "jaccard", "cosine"), ("cosine", "jaccard", "shared", "bound"),
            ("jaccard", "shared", "bound", "cosine"), ("bound", "shared", "cosine", "jaccard")]


F32_FORMS = ("f32_host", "f32_dev", "u8_host", "u8_dev", "csr_host", "csr_pinned", "csr_dev")


def form_allowed(form, index):
    """the bitset and .bed boundaries need a packed-operand engine (not gram_kernel f32); a walk under debug knobs has no
    bound segment (a companion that folds or cannot narrow has an int64 part, which a centring refuses), so no bed_calls"""
    if WALKS[index][2] == "f32" and form not in F32_FORMS:     # (the pruner's accumulation is the bitset boundary)
        return False
    return form != "bed_calls" or WALKS[index][4] is None


def vp():
    return load_pkg("variants_pca")


class Expected(object):
    """What one observer must return.  error: the name of the PCOA_ERR_* code or None; exact: name -> array that must be equal;
    close: name -> (reference, bound per entry); note: what only the caller can check."""

    def __init__(self, error=None, exact=None, close=None, note=None):
        self.error, self.exact, self.close, self.note = error, exact or {}, close or {}, note or {}


# ---- the model ------------------------------------------------------------------------------------------------------------------
class Companion(object):
    """The bound companion: its total matrix Q, the V it is bound with, and whether the engine owns it (a subset's)."""

    def __init__(self, q, v, owned=False):
        self.q, self.v, self.owned = np.array(q, dtype=np.int64), int(v), bool(owned)


class Model(object):
    """A full engine as the header defines its answers: N, the create flags, the total S, the measure, the companion."""

    def __init__(self, n, kernel="auto", operand="bits", s=None, measure="shared", comp=None):
        self.n, self.kernel, self.operand = int(n), kernel, operand
        self.s = np.zeros((self.n, self.n), dtype=np.int64) if s is None else np.array(s, dtype=np.int64)
        self.measure, self.comp = measure, comp
        self._memo = {}

    def copy(self):
        comp = None if self.comp is None else Companion(self.comp.q, self.comp.v, self.comp.owned)
        return Model(self.n, self.kernel, self.operand, self.s, self.measure, comp)

    # -- mutators
    def _changed(self):
        self._memo = {}

    def append(self, carriers, missing=None):
        """rows as they are fed: S += X^T X; under a binding the companion takes the missing rows and V grows by the call"""
        self.s = self.s + int_gram(carriers)
        if self.comp is not None and missing is not None:
            self.comp.q = self.comp.q + int_gram(missing)
            self.comp.v += carriers.shape[0]
        self._changed()

    def reset(self):
        self.s = np.zeros_like(self.s)
        self._changed()

    def load(self, s):
        self.s = np.array(s, dtype=np.int64)
        self._changed()

    def add(self, s):
        self.s = self.s + np.asarray(s, dtype=np.int64)
        self._changed()

    def subset(self, keep):
        keep = np.asarray(keep, dtype=np.int64)
        comp = None if self.comp is None else Companion(self.comp.q[np.ix_(keep, keep)], self.comp.v, owned=True)
        return Model(keep.size, self.kernel, self.operand, self.s[np.ix_(keep, keep)], self.measure, comp)

    def set_similarity(self, kind):
        assert self.comp is None or kind == "shared"
        self.measure = kind
        self._changed()

    def bind(self, v, fresh):
        """fresh: a new caller-owned companion with Q = 0; else the companion bound now with another V; v None: unbind"""
        assert self.measure == "shared"
        if v is None:
            self.comp = None
        elif fresh:
            self.comp = Companion(np.zeros_like(self.s), v)
        else:
            self.comp.v = int(v)
        self._changed()

    def companion_append(self, missing):
        """rows at which nobody carries anything: Q and V grow, S does not"""
        self.comp.q = self.comp.q + int_gram(missing)
        self.comp.v += missing.shape[0]
        self._changed()

    def companion_reset(self):
        self.comp.q = np.zeros_like(self.comp.q)
        self._changed()

    # -- the state behind the answers
    def _once(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def i64_live(self):
        """1 exactly when an entry of S lies beyond int32"""
        return int(np.abs(self.s).max() > INT32_MAX) if self.s.size else 0

    def plain(self):
        return self.comp is None and self.measure == "shared"

    def consistent(self):
        """under a binding every shared count is a count of jointly called variants: |K| <= 1, which the bounds assume"""
        if self.comp is None:
            return True
        c = self.comp.v - np.diagonal(self.comp.q)
        m = c[:, None] + c[None, :] - self.comp.v + self.comp.q
        return bool(np.all(c >= 0) and np.all(self.s <= np.maximum(m, 0)))

    def k64(self):
        if self.comp is not None:
            return vp().call_complete_measure(self.s, self.comp.q, self.comp.v)
        return vp().similarity_measure(self.s, self.measure)

    def centred(self):
        """(B float64 or longdouble, r, mm, nonzero_rows, exact): the oracle's own centring for the shared counts (exact: the
        device returns these bits, tests/test_gpu_parity.py), the long-double rule of the measure tests otherwise"""
        def make():
            if self.plain():
                b, rs, nz, mm = load_oracle().center_matrix(self.s)
                return b, rs, float(mm), int(nz), True
            if self.comp is not None:
                b, r, mm, nz = C.reference(self.s, self.comp.q, self.comp.v)
            else:
                b, r, mm, nz = M.reference(self.s, self.measure)
            return b, r, mm, int(nz), False
        return self._once("centred", make)

    def b64(self):
        def make():
            if self.plain():
                return self.centred()[0]
            return vp().centred_measure(self.k64())[0]
        return self._once("b64", make)

    def spectrum(self):
        """eigenpairs of B by numpy.linalg.eigh, largest |lambda| first (pcoa_compute selects by |lambda|)"""
        def make():
            w, z = np.linalg.eigh(self.b64())
            order = np.argsort(-np.abs(w), kind="stable")
            return w[order], z[:, order]
        return self._once("spectrum", make)

    def gaps_ok(self, k):
        w = np.abs(self.spectrum()[0])
        if w[0] == 0:
            return False
        return all((w[c] - w[c + 1]) / w[0] >= MIN_GAP for c in range(min(k, self.n - 1)))

    def degenerate(self):
        return (not self.s.any()) or bool((np.diagonal(self.s) == 0).any()) or self.n == 32

    # -- the observers
    def expect(self, op, a):
        n, s = self.n, self.s
        if op in ("gram", "export"):
            return Expected(exact={"s": s})
        if op == "gram_block":
            r0, c0, r, c = a["rect"]
            return Expected(exact={"s": s[r0:r0 + r, c0:c0 + c]})
        if op == "pairs":
            want = vp().related_pairs_rule(s, a["min_jaccard"])
            listed = want[:min(want.size, a["capacity"])]
            return Expected(exact={"found": np.array([want.size], dtype=np.int64), "i": listed["i"], "j": listed["j"],
                                   "shared": listed["shared"], "diag": np.diagonal(s).copy()})
        if op == "center":
            b, r, mm, nz, exact = self.centred()
            if exact:
                return Expected(exact={"b": b, "rs": r, "mm": np.array([mm]), "nz": np.array([nz], dtype=np.int64)})
            return Expected(exact={"nz": np.array([nz], dtype=np.int64)},
                            close={"b": (b, M.entry_bound(n)), "rs": (r, M.row_sum_bound(n)), "mm": (np.array([mm]), M.entry_bound(n))})
        if op == "matvec":
            x = vector_of(a["seed"], n)
            b, _, _, _, exact = self.centred()
            ab = np.abs(np.asarray(b, dtype=np.float64))
            ref = np.asarray(b, dtype=np.longdouble) @ x.astype(np.longdouble)
            # the shared counts: the summation bound of tests/test_gpu_centred_matvec_forms.py over the oracle's B; a measure
            # or a binding: measure_cohort.matvec_bound, which adds the entry bound on every term
            bound = n * 2.0 ** -52 * (ab @ np.abs(x)) if exact else M.matvec_bound(n, ab, x)
            return Expected(close={"y": (ref, bound)})
        if op == "compute":
            w, z = self.spectrum()
            k = a["k"]
            return Expected(exact={"nz": np.array([self.centred()[3]], dtype=np.int64)},
                            note={"eigenvalues": w[:k].copy(), "vectors": np.ascontiguousarray(z[:, :k]) if self.gaps_ok(k) else None})
        if op == "loadings":
            x, u, lam = loadings_of(a, n)
            want = loadings_rule(x, u, lam)
            return Expected(close={"w": (want, summation_bound(x, u, lam, want))})
        if op == "getters":
            return Expected(exact={"similarity": np.array([M.KIND[self.measure]], dtype=np.int64),
                                   "companion": np.array([0 if self.comp is None else 1, 0 if self.comp is None else self.comp.v],
                                                         dtype=np.int64)})
        raise ValueError("no observer %r" % (op,))


# ---- what a script's arguments stand for ------------------------------------------------------------------------------------
def rows_of(a, n):
    """(carriers uint8 [k][n] as the engine must count them, missing bool [k][n] or None) of an append: planted populations;
    zero1: sample 1 carries nothing; mult: multiplicities up to 127; missing: 8 % of the calls are missing (a missing call
    carries nothing), which the .bed forms code as 01 and a bound engine's companion is fed."""
    rng = np.random.default_rng(a["seed"])
    k = a["k"]
    x = planted_callsets(rng, n, k, k=POPS).astype(np.uint8) if k else np.zeros((0, n), dtype=np.uint8)
    if a.get("form") == "ld_prune":
        x = ld_cohort(n, k, a["seed"])                                 # rows that exceed at every threshold
    if a.get("zero1"):
        x[:, 1] = 0
    if a.get("mult"):
        x = (x * rng.integers(1, 128, size=x.shape)).astype(np.uint8)
    missing = None
    if a.get("missing"):
        missing = rng.random((k, n)) < 0.08
        x = np.where(missing, 0, x).astype(np.uint8)
    return x, missing


def ld_chunks(a, x):
    """(cut, keep [k] bool) of an ld_prune append: the rows go through one pruner in two calls, [0, cut) and [cut, k).  The
    rule does not depend on the split -- unless a reset falls between the calls: it drops the carried rows, so the second
    chunk starts a window of its own (and is all that S holds afterwards)."""
    cut = a["cut"]
    if a["reset_between"]:
        return cut, np.concatenate([ld_rule(x[:cut], a["window"], a["r2"]), ld_rule(x[cut:], a["window"], a["r2"])])
    return cut, ld_rule(x, a["window"], a["r2"])


def missing_rows(a, n):
    """the rows of a companion_append"""
    return np.random.default_rng(a["seed"]).random((a["k"], n)) < 0.08


def seeded_gram(seed, n):
    return int_gram(planted_callsets(np.random.default_rng(seed), n, LOAD_ROWS, k=POPS))


def big_gram(seed, n):
    """the seeded Gram scaled beyond int32; every sum of its entries stays an exact fp64 integer"""
    s = seeded_gram(seed, n) * BIG_SCALE
    assert s.max() > 2 ** 31 and s.max() < 2 ** 53 // n and s.max() < 2 ** 52 // (n * n)
    return s


def near_gram(seed, n):
    """the seeded Gram scaled so that its largest entry is just below 0.45 * 2^31: two of them fit int32, three do not"""
    s = seeded_gram(seed, n)
    s = s * int(0.45 * 2 ** 31 // s.max())
    assert 0.44 * 2 ** 31 < s.max() < 0.45 * 2 ** 31
    return s


def load_of(a, n):
    if a["kind"] == "zero":
        return np.zeros((n, n), dtype=np.int64)
    if a["kind"] == "near":
        return near_gram(a["seed"], n)
    return big_gram(a["seed"], n) if a["kind"] == "big" else seeded_gram(a["seed"], n)


def partner_rows(seed, n, k):
    return planted_callsets(np.random.default_rng(seed), n, k, k=POPS).astype(np.uint8)


def keep_of(a, n):
    return np.sort(np.random.default_rng(a["seed"]).choice(n, size=a["size"], replace=False)).astype(np.int32)


def vector_of(seed, n):
    return np.random.default_rng(seed).standard_normal(n)


def loadings_of(a, n):
    """(x uint8 [rows][n], u [n][num_pc], lam [num_pc]) of a loadings step: any vectors will do"""
    rng = np.random.default_rng(a["seed"])
    x = (rng.random((a["rows"], n)) < 0.2).astype(np.uint8)
    return x, rng.standard_normal((n, a["num_pc"])) + 0.3, rng.uniform(0.5, 800.0, size=a["num_pc"])


def buffer_needs(a, n, x):
    """{buffer: elements} an append asks of the ctx's `ensure` buffers (floor 1,024; csrc/capi_accumulate.hip): the tile of the
    host forms -- rows x the pitch rounded up to four for fp32, a quarter of that for uint8, rows x bitset words for .bed rows --
    and the index buffer of the pageable carrier lists.  (The offsets buffer takes rows + 1 <= 401 elements and never leaves its
    floor; thr_dev serves the synthetic generator only.)"""
    k, ld4, words = a["k"], (n + 3) // 4 * 4, (n + 31) // 32
    if a["form"] == "f32_host":
        return {"tile": k * ld4}
    if a["form"] == "u8_host":
        return {"tile": (k * ld4 + 3) // 4}
    if a["form"] in ("bed_host", "bed_calls"):
        return {"tile": k * words}
    if a["form"] == "csr_host":
        return {"csr_idx": int(np.count_nonzero(x))}
    return {}


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


def apply(model, op, a):
    """The model after mutator `op`; a subset returns the new model, a walk that comes back empty from a reduction a reset one."""
    n = model.n
    if op == "append":
        x, missing = rows_of(a, n)
        if a.get("form") == "ld_prune":
            cut, keep = ld_chunks(a, x)
            if a["reset_between"]:
                model.reset()
                x, keep = x[cut:], keep[cut:]
            x = x[keep]
        model.append(x, missing if model.comp is not None else None)
    elif op == "reset":
        model.reset()
    elif op == "load":
        model.load(load_of(a, n))
    elif op == "export_import":
        pass
    elif op == "reduce_from":
        model.add(near_gram(a["seed"], n) if a.get("near") else int_gram(partner_rows(a["seed"], n, a["k"])))
    elif op == "reduce_peers":
        if a["root_only"] and a["position"] > 0:
            model.reset()
        else:
            for g in range(2):
                model.add(int_gram(partner_rows(a["seed"] + g, n, a["k"])))
    elif op == "subset":
        return model.subset(keep_of(a, n))
    elif op == "set_similarity":
        model.set_similarity(a["kind"])
    elif op == "bind":
        model.bind(a["v"], a["fresh"])
    elif op == "companion_append":
        model.companion_append(missing_rows(a, n))
    elif op == "companion_reset":
        model.companion_reset()
    elif op in ("reserve", "set_stream"):
        pass
    else:
        raise ValueError("no mutator %r" % (op,))
    return model


# ---- the generator --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hands():
    """(pairs, forms) per walk: the deck of all (mutator class, observer) pairs without the appends', and the deck of all (input
    form, reader of S) pairs, shuffled and dealt round."""
    rng = np.random.default_rng(DECK_SEED)
    pairs = [(c, o) for c in CLASSES if c != "append" for o in OBSERVERS]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    forms = [(f, o) for f in READ_FORMS for o in READERS] + [(f, o) for f in ("f32_host", "bits_dev") for o in ("loadings", "getters")]
    forms = [forms[i] for i in rng.permutation(len(forms))]
    out_p, out_f = [[] for _ in WALKS], [[] for _ in WALKS]
    large = [w for w in range(len(WALKS)) if WALKS[w][1] >= 130]      # a subset pair needs a size to go down to
    plain = [w for w in range(len(WALKS)) if WALKS[w][4] is None]      # a binding pair needs a bound segment
    evens = [w for w in range(len(WALKS)) if w % 2 == 0] + [w for w in range(len(WALKS)) if w % 2]   # (odd walks start degenerate)
    i = j = b = r = 0
    for p in pairs:
        if p[0] == "reset":
            out_p[evens[r % len(evens)]].append(p)
            r += 1
        elif p[0] == "subset":
            out_p[large[j % len(large)]].append(p)
            j += 1
        elif p[0] == "binding":
            out_p[plain[b % len(plain)]].append(p)
            b += 1
        else:
            out_p[i % len(WALKS)].append(p)
            i += 1
    i = 0
    for p in forms:
        while not form_allowed(p[0], i % len(WALKS)):
            i += 1
        out_f[i % len(WALKS)].append(p)
        i += 1
    return tuple(tuple(x) for x in out_p), tuple(tuple(x) for x in out_f)


class Planner(object):
    """Writes the script of one walk, running the model alongside so that every step is chosen for the state it meets.  A walk
    is four segments (SEGMENTS): the engine decomposes the shared counts, a Jaccard or a cosine measure, or is bound to a
    companion.  Inside a segment appends (each taking an (input form, reader) pair of its hand) alternate with the other
    mutators (each taking a (class, observer) pair); the first append of a measured or bound segment is larger than any call
    the ctx has seen, so its buffers regrow there."""

    def __init__(self, index):
        seed, n0, kernel, operand, child = WALKS[index]
        self.index, self.seed, self.rng = index, seed, np.random.default_rng(seed)
        self.model = Model(n0, kernel, operand)
        self.pairs, self.forms = [list(h[index]) for h in hands()]
        self.mult_ok = kernel in ("auto", "i8", "f32")
        self.mult_before = ["reset", "load", "subset"] if self.mult_ok else []
        self.script, self.queue, self.trace = [], [], []
        self.nsteps = self.degenerate = self.appends = self.rows = self.max_call = 0
        self.next_seed = 1000 * seed
        self.segments = [g for g in SEGMENTS[index] if g != "bound" or child is None]
        self.mode, self.seg_left, self.grown = "shared", 0, True
        self.refused, self.refusals = set(), index
        self.last_append = False
        self.stream, self.finale, self.binds, self.emptied, self.neared, self.ld_reset = "null", False, 0, False, False, False

    # -- small draws
    def draw_seed(self):
        self.next_seed += 1
        return self.next_seed

    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    def room(self, optional=False):
        """the budget of degenerate steps; an optional one leaves room for the resets of the hand and the walk's last step"""
        pending = sum(1 for p in self.pairs if p[0] == "reset") + 1 if optional else 0
        return self.degenerate + pending < DEGENERATE_BUDGET

    def next_size(self):
        """the next smaller N; 32 itself is left to the last step of a walk (every state at N = 32 counts as degenerate)"""
        return next((s for s in SIZES if s < self.model.n and (s != 32 or self.finale)), None)

    # -- observers
    def observer_args(self, o):
        m, n, rng = self.model, self.model.n, self.rng
        if o in ("gram", "export", "center", "getters"):
            return {}
        if o == "gram_block":
            rects = [(n - 3, 0, 3, n), (0, n - 2, n, 2), (max(0, min(30, n - 6)), max(0, min(60, n - 9)), min(6, n), min(9, n))]
            if n > 70:
                rects.append((62, 30, 5, 40))
            return {"rect": self.pick(rects)}
        if o == "pairs":
            s = m.s
            d = np.diagonal(s)
            u = d[:, None] + d[None, :] - s
            iu = np.triu_indices(n, 1)
            ok = u[iu] > 0
            cut = 0.5
            if ok.any():
                ratio = np.sort(s[iu][ok] / u[iu][ok])
                at = int(ratio.size * self.pick((0.9, 0.97, 0.995)))
                at = min(max(at, 1), ratio.size - 1)
                # between two neighbouring ratios that differ: the rule is exact on both sides, nothing sits on the cut
                while at < ratio.size - 1 and ratio[at] - ratio[at - 1] < 1e-9:
                    at += 1
                cut = float((ratio[at] + ratio[at - 1]) / 2)
                if not 0 < cut <= 1:
                    cut = 0.5
            found = int(vp().related_pairs_rule(s, cut).size)
            cap = self.pick((0, max(found // 2, 0), found + 3, n * n))
            return {"min_jaccard": cut, "capacity": int(cap)}
        if o == "matvec":
            # form 1 needs N % 4 == 0 and no int64 part: what the model can promise only where no knob moves S into one
            forms = [0, 2] + ([1] if n % 4 == 0 and not m.i64_live() and WALKS[self.index][4] is None else [])
            return {"form": int(self.pick(forms)), "seed": self.draw_seed()}
        if o == "compute":
            ks = [k for k in ((1, 2, 5) if n >= 97 and m.comp is None else (1, 2)) if m.gaps_ok(k)]
            return {"k": int(self.pick(ks or [1]))}
        if o == "loadings":
            return {"rows": int(self.pick((1, 37, 130))), "num_pc": int(self.pick((1, 2, 3))), "seed": self.draw_seed()}
        raise ValueError(o)

    def fill_observer(self):
        return self.pick(OBSERVERS)

    # -- mutators
    def append_args(self, form=None, k=None, mult=False, zero1=False):
        m = self.model
        bound = m.comp is not None
        if form is None:
            form = self.pick([f for f in READ_FORMS if form_allowed(f, self.index) and (f != "bed_calls" or bound)
                              and (f != "ld_prune" or not bound)])
        if k is None and not m.s.any():
            k = self.pick((200, 257))                                  # enough rows that every sample carries something
        if k is None:
            if not self.grown and self.max_call < 400:
                k = next(c for c in CALL_SIZES if c > self.max_call)
            else:
                k = self.pick(CALL_SIZES[:6] if self.max_call < 130 else CALL_SIZES)
        if self.rows + k > MAX_ROWS and m.s.any():
            k = 17
        if form == "empty":
            k = 0
        self.appends += 1
        out = {"form": form, "k": int(k), "seed": self.draw_seed(), "mult": bool(mult), "zero1": bool(zero1),
               "missing": bool(bound or form in BED_FORMS), "ref_is_a1": bool(self.rng.random() < 0.5)}
        if form == "ld_prune":
            # once in a walk a reset falls between the two chunks (ld_drop_tail), where the budget of degenerate steps allows
            drop = not self.ld_reset and self.room(True) and self.nsteps >= 3 and self.rows + 400 <= MAX_ROWS
            self.ld_reset = self.ld_reset or drop
            if drop:
                out["k"] = 400                                         # (the second chunk alone must give every sample a carrier)
            out.update({"window": int(self.pick((7, 20))), "r2": float(self.pick((0.2, 0.5))), "reset_between": bool(drop),
                        "cut": int(self.rng.integers(1, out["k"]))})
            if drop:   # a cut at which the carried rows matter: the rule over all rows keeps other rows than the two chunks alone
                x = rows_of(out, m.n)[0]
                whole = ld_rule(x, out["window"], out["r2"])
                out["cut"] = next(c for c in range(140, 260) if not np.array_equal(
                    whole, ld_chunks(dict(out, cut=c), x)[1]))
        return out

    def take_form(self):
        bound = self.model.comp is not None
        for p in sorted(self.forms, key=lambda p: not (bound and p[0] == "bed_calls")):   # (stable: bed_calls first when bound)
            if (p[0] == "bed_calls" and not bound) or (p[0] == "ld_prune" and bound):
                continue
            self.forms.remove(p)
            return p
        return None

    def feasible(self, p):
        c, o = p
        bound = self.mode == "bound" and self.model.comp is not None
        if not self.model.s.any():
            return False
        if c == "reset":
            return self.room() and self.nsteps >= 3
        if c == "load":
            return not bound
        if c == "import":
            return True
        if c == "reduce":
            return not bound
        if c == "subset":
            return self.next_size() is not None and self.nsteps >= 8
        if c == "measure":
            return True
        if c == "binding":
            return bound
        return False

    def class_args(self, c):
        """(mutator, arguments) of class c in the state the walk is in"""
        m, rng = self.model, self.rng
        if c == "reset":
            return "reset", {}
        if c == "load":
            kind = self.pick(("gram", "big", "gram", "big", "zero")) if self.room(True) else self.pick(("gram", "big"))
            if m.comp is not None:
                kind = "zero"
            return "load", {"kind": kind, "seed": self.draw_seed()}
        if c == "import":
            return "export_import", {}
        if c == "reduce":
            which = self.pick(("from", "peers", "peers_root", "peers_nonroot"))
            if which == "peers_nonroot" and not (self.room(True) and self.nsteps >= 3):
                which = "peers_root"
            k = int(self.pick((40, 130)))
            if which == "from":
                return "reduce_from", {"seed": self.draw_seed(), "k": k}
            a = {"seed": self.draw_seed(), "k": k, "root_only": int(which != "peers"), "position": int(which == "peers_nonroot")}
            self.draw_seed()
            return "reduce_peers", a
        if c == "subset":
            return "subset", {"size": int(self.next_size()), "seed": self.draw_seed()}
        if c == "measure":
            return "set_similarity", {"kind": m.measure}                       # the same kind again
        if c == "binding":
            which = ("companion_reset", "new_v", "companion_append", "same_v")[(self.binds + self.index) % 4]   # each in turn
            self.binds += 1
            if which == "new_v":
                return "bind", {"v": m.comp.v + int(rng.integers(1, 50)), "fresh": False}
            if which == "same_v":
                return "bind", {"v": m.comp.v, "fresh": False}
            if which == "companion_append":
                return "companion_append", {"k": int(self.pick((17, 64))), "seed": self.draw_seed()}
            return "companion_reset", {}
        raise ValueError(c)

    def take_pair_observer(self, c):
        for p in self.pairs:
            if p[0] == c:
                self.pairs.remove(p)
                return p[1]
        return self.fill_observer()

    def transition(self):
        """the mutators that take the walk into its next segment"""
        target = self.segments.pop(0)
        m = self.model
        steps = []
        if m.comp is not None:
            steps.append(("bind", {"v": None, "fresh": False}))
        if target == "bound":
            if m.measure != "shared":
                steps.append(("set_similarity", {"kind": "shared"}))
            steps.append(("bind", {"v": "fresh", "fresh": True}))
        elif target != m.measure or not steps:
            steps.append(("set_similarity", {"kind": target}))
        self.queue = [(mm, ma, None) for mm, ma in steps] + self.queue
        self.mode, self.grown = target, target == "shared"
        self.seg_left = max((STEPS - self.nsteps) // (len(self.segments) + 1), 6)

    def choose(self):
        """(mutator, arguments, observer or None)"""
        if self.queue:
            return self.queue.pop(0)
        if self.seg_left <= 0 and self.segments and self.model.s.any():
            self.transition()
            return self.queue.pop(0)
        m = self.model
        if not m.s.any() or (np.diagonal(m.s) == 0).any():
            return ("append", None, None)
        if self.nsteps >= 16 and not self.neared and m.comp is None and self.index % 4 == 0:
            # three partials just below 0.45 * 2^31: the first reduction stays in int32 and must carry its bound of the entries
            # into the second, which leaves int32 -- a bound left behind would let the second add in place and wrap
            self.neared = True
            self.queue = [("reduce_from", {"seed": self.draw_seed(), "k": 0, "near": True}, self.pick(READERS)) for _ in range(2)]
            return ("load", {"kind": "near", "seed": self.draw_seed()}, None)
        if self.nsteps >= 7 and not self.emptied:
            self.emptied = True
            return ("append", {"form": "empty"}, None)
        if not self.last_append and (self.forms or self.rng.random() < 0.5):
            return ("append", None, None)
        for p in self.pairs:
            if self.feasible(p):
                self.pairs.remove(p)
                mut, ma = self.class_args(p[0])
                return self.with_mult(p[0], mut, ma, p[1])
        c = self.pick(("import", "neutral", "load", "reduce", "measure"))
        if c == "neutral":
            if self.rng.random() < 0.5:
                return ("reserve", {"variants": int(self.pick((0, 64, 500))), "num_pc": int(self.pick((0, 2, 5)))}, None)
            self.stream = "torch" if self.stream == "null" else "null"
            return ("set_stream", {"to": self.stream}, None)
        if not self.feasible((c, None)):
            c = "import"
        mut, ma = self.class_args(c)
        return self.with_mult(c, mut, ma, None)

    def with_mult(self, c, mut, ma, o):
        """the int8 redo in flight: an append with multiplicities directly in front of the first reset, load and subset"""
        if c in self.mult_before and self.model.comp is None and self.rows + 64 <= MAX_ROWS:
            self.mult_before.remove(c)
            self.queue.insert(0, (mut, ma, o))
            # behind a non-reader: a reader would flush the generation (finalize_impl) in front of the mutator
            return ("append", {"mult": True, "form": self.pick(MULT_FORMS), "k": int(self.pick((33, 64)))}, self.pick(NON_READERS))
        if c == "reset" and self.model.comp is None and not self.model.i64_live():
            # the reset meets an int64 part: load(beyond int32) -> reset -> append, the history that must leave none behind
            self.queue.insert(0, (mut, ma, o))
            return ("load", {"kind": "big", "seed": self.draw_seed()}, None)
        return (mut, ma, o)

    def refusal(self):
        if self.nsteps % 12 != 5:
            return None
        m = self.model
        kind = None
        low_v = m.comp is not None and np.diagonal(m.comp.q).max() >= 1 and "bind_low_v" not in self.refused
        if low_v and self.index % 2:
            kind = "bind_low_v"
        elif m.comp is not None and "jaccard_on_bound" not in self.refused:
            kind = "jaccard_on_bound"
        elif low_v:
            kind = "bind_low_v"
        elif m.measure != "shared" and "bind_on_measured" not in self.refused:
            kind = "bind_on_measured"
        else:
            kind = GENERIC_REFUSALS[self.refusals % len(GENERIC_REFUSALS)]
            self.refusals += 1
        self.refused.add(kind)
        return kind

    def step(self):
        mut, ma, o = self.choose()
        m = self.model
        if mut == "append":
            hint = ma or {}
            form = hint.get("form")
            if form is None and o is None:
                p = self.take_form()
                if p is not None:
                    form, o = p
            zero1 = self.index % 2 == 1 and self.appends == 0
            mult = hint.get("mult", False)
            if self.mult_ok and m.comp is None and (self.appends + 1) % 6 == 0 and not mult and hint.get("form") is None:
                # one append in six carries multiplicities: in the dense form the hand asks for, else in one drawn from them
                if form is not None and form not in MULT_FORMS:
                    self.forms.insert(0, (form, o))                    # (the pair goes back to the hand)
                    form, o = self.pick(MULT_FORMS), None
                elif form is None:
                    form = self.pick(MULT_FORMS)
                mult = True
            ma = self.append_args(form, hint.get("k"), mult, zero1)
            if ma["k"] > self.max_call and self.mode != "shared":
                self.grown = True
            self.max_call, self.rows = max(self.max_call, ma["k"]), self.rows + ma["k"]
        elif mut == "bind" and ma["v"] == "fresh":
            ma = {"v": int(max(int(m.s.max()), 1) + int(self.rng.integers(0, 20))), "fresh": True}
        if o is None:
            o = self.take_pair_observer(CLASS_OF[mut]) if CLASS_OF[mut] in CLASSES and mut != "append" else self.fill_observer()
        self.model = apply(m, mut, ma)
        if mut == "subset":
            self.max_call, self.grown = 0, self.mode == "shared"
        assert self.model.consistent(), (self.seed, self.nsteps, mut)
        self.script.append((mut, ma))
        self.last_append = mut == "append"
        kind = self.refusal()
        if kind:
            self.script.append(("refuse", {"kind": kind}))
        if o == "compute" and not self.model.gaps_ok(1) and self.model.s.any():
            o = "center"                                               # a spectrum without a gap says nothing about the vectors
        oa = self.observer_args(o)
        self.script.append((o, oa))
        self.degenerate += bool(self.model.degenerate())
        self.nsteps += 1
        self.seg_left -= 1

    def run(self):
        while (self.nsteps < STEPS or self.queue or self.segments or self.forms or self.pairs) and self.nsteps < STEPS_CAP:
            self.step()
        self.finale = True                                             # the walk ends one or two sizes further down
        for _ in range(2):
            if self.next_size() is not None and (self.next_size() != 32 or self.room()):
                self.queue = [("subset", {"size": int(self.next_size()), "seed": self.draw_seed()}, None)]
                self.step()
        return self.script


@functools.lru_cache(maxsize=None)
def script(index):
    """The walk WALKS[index] as a tuple of (op, arguments)."""
    return tuple(Planner(index).run())


def new_model(index):
    _, n0, kernel, operand, _ = WALKS[index]
    return Model(n0, kernel, operand)

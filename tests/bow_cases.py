"""Seeded generator of vocabularies, feature sets and keyframe-database sessions for the DBoW2 tests (CPU and GPU).  Everything is synthetic: small trees in the
format of loadFromTextFile, with about 5 % stopped words (weight 0), duplicate descriptors among siblings (the first-minimum tie) and features that are exact copies
of node descriptors.  Expected values come from tests/dbow_reference.py alone and are computed once per process."""
import functools
import numpy as np
import dbow_reference as R

VOCABS = {                      # name: (k, L, irregular)
    "k10L3": (10, 3, False),
    "k3L6irr": (3, 6, True),
    "k2L1": (2, 1, False),
    "k20L2": (20, 2, False),
    "k10L4": (10, 4, False),
}


def _weights(r, n):
    w = np.exp(r.uniform(-2.0, 2.5, n))                     # idf-like, full-precision doubles: sums depend on the order of the additions
    w[r.random(n) < 0.05] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def vocab(name):
    k, L, irregular = VOCABS[name]
    r = np.random.default_rng(1000 + sorted(VOCABS).index(name))
    parent, leaf, desc, depth = [], [], [], []

    def node(p, d, is_leaf, like=None):
        parent.append(p); depth.append(d); leaf.append(1 if is_leaf else 0)
        desc.append(desc[like - 1].copy() if like else r.integers(0, 256, 32, dtype=np.uint8))
        return len(parent)

    if not irregular:                                       # full tree, level by level: the children of a node are contiguous lines
        level = [0]
        for d in range(1, L + 1):
            nxt = []
            for p in level:
                first = None
                for c in range(k):
                    dup = first if (first and c in (1, k - 1) and ((p == 0 and c == 1) or r.random() < 0.3)) else None      # a sibling with the first child's descriptor
                    nid = node(p, d, d == L, dup)
                    first = first or nid
                    nxt.append(nid)
            level = nxt
    else:                                                   # depth first: siblings are NOT contiguous lines; early leaves; fewer than k children
        def grow(p, d):
            n_children = k if p == 0 else int(r.integers(1, k + 1))
            kids = []
            for c in range(n_children):
                early = (p == 0 and c == 0) or (d < L and r.random() < 0.15)                      # node 1 is a leaf at depth 1
                dup = kids[0] if (kids and c == n_children - 1 and r.random() < 0.4) else None
                kids.append(node(p, d, d == L or early, dup))
                if not leaf[kids[-1] - 1]:                  # the subtree follows its root at once: the next sibling's line comes after it
                    grow(kids[-1], d + 1)
        grow(0, 1)
    n = len(parent)
    weight = np.where(np.array(leaf) > 0, _weights(r, n), 0.0)
    if not np.any((weight == 0) & (np.array(leaf) > 0)):     # a small tree: one stopped word at least
        weight[np.nonzero(leaf)[0][-1]] = 0.0
    return R.Vocabulary(k, L, 0, 0, parent, leaf, np.array(desc, np.uint8), weight)


def features(name, n, seed, pool=40):
    """n descriptors: a third perturbed copies of a small pool of leaves (repeated words), a third exact copies of node descriptors, the rest random"""
    v = vocab(name)
    r = np.random.default_rng(seed)
    out = r.integers(0, 256, (n, 32), dtype=np.uint8)
    if n == 0:
        return out
    leaves = v.words[r.integers(0, v.n_words, min(pool, v.n_words))]
    for i in range(n):
        t = i % 3
        if t == 0:
            d = v.descriptor[int(leaves[r.integers(0, len(leaves))])].copy()
            for _ in range(int(r.integers(0, 4))):
                d[r.integers(0, 32)] ^= np.uint8(1 << int(r.integers(0, 8)))
            out[i] = d
        elif t == 1:
            out[i] = v.descriptor[int(r.integers(1, v.n_nodes))]
    return out


@functools.lru_cache(maxsize=None)
def expected(name, n, seed, levelsup):
    return vocab(name).transform(features(name, n, seed), levelsup, per_feature=True)


# ---- keyframe database sessions ----
SESSION_VOCAB = "k10L3"


@functools.lru_cache(maxsize=None)
def session(n_entries, steps=300, seed=0, rebow=True):
    """A list of operations on a database of `n_entries` entries (any entry may be the query):
         ("set_bow", e, desc[n, 32])   ("add", e)   ("erase", e)   ("clear",)   ("nb", e, nb[10])   ("query", kind, e, query_id, connected[], min_score)
       Entries see one of a few `places` (shared leaves), so queries find candidates; query ids come from {0 .. 5}."""
    v = vocab(SESSION_VOCAB)
    r = np.random.default_rng(7000 + 13 * n_entries + seed)
    n_places = max(1, n_entries // 6)
    places = [v.words[r.integers(0, v.n_words, 30)] for _ in range(n_places)]

    def view(place):
        m = int(r.integers(40, 70))
        d = r.integers(0, 256, (m, 32), dtype=np.uint8)
        for i in range(m):
            if r.random() < 0.85:
                d[i] = v.descriptor[int(places[place][r.integers(0, 30)])]
                if r.random() < 0.3:
                    d[i, r.integers(0, 32)] ^= np.uint8(1 << int(r.integers(0, 8)))
        return d

    ops, has_bow, live = [], [False] * n_entries, [False] * n_entries
    last_id = [-1, -1]                                      # per field group: loop, relocalisation / map fusion
    place_of = [int(r.integers(0, n_places)) for _ in range(n_entries)]
    for e in range(n_entries):                              # start populated: every BowVector first (a neighbour is a keyframe that has one)
        ops.append(("set_bow", e, view(place_of[e]))); has_bow[e] = True
    for e in range(n_entries):
        if e == 0 or r.random() < 0.8:
            ops.append(("add", e)); live[e] = True
        ops.append(("nb", e, _neighbours(r, e, n_entries)))
    while len(ops) < steps + 3 * n_entries:
        u = r.random(); e = int(r.integers(0, n_entries))
        if u < 0.10:
            if not rebow:                                   # (the adapter's session: a keyframe's BowVector is computed once)
                continue
            if live[e]:
                ops.append(("erase", e)); live[e] = False
            ops.append(("set_bow", e, view(place_of[e] if r.random() < 0.7 else int(r.integers(0, n_places))))); has_bow[e] = True
        elif u < 0.22:
            if has_bow[e] and not live[e]:
                ops.append(("add", e)); live[e] = True
        elif u < 0.30:
            if live[e]:
                ops.append(("erase", e)); live[e] = False
        elif u < 0.32:
            ops.append(("clear",)); live = [False] * n_entries
        elif u < 0.40:
            ops.append(("nb", e, _neighbours(r, e, n_entries)))
        elif has_bow[e]:
            if not any(live):                               # a query of an empty database finds nothing: put an entry in first (small databases are often empty)
                a = e if n_entries == 1 else int(r.integers(0, n_entries))
                if has_bow[a]:
                    ops.append(("add", a)); live[a] = True
            kind = int(r.integers(0, 3)); qid = int(r.integers(0, 6))
            if qid == last_id[min(kind, 1)] and r.random() < 0.6:      # a repeated id pushes nothing: met, but not most of the time
                qid = (qid + 1 + int(r.integers(0, 5))) % 6
            last_id[min(kind, 1)] = qid
            nc = int(r.integers(0, 4))
            conn = sorted(set(int(c) for c in r.integers(0, n_entries, nc))) if kind == 0 else []
            ms = float(np.float32([0.0, 0.02, 0.1][int(r.integers(0, 3))]))
            ops.append(("query", kind, e, qid, conn, ms))
    return ops


def _neighbours(r, e, n_entries):
    nb = np.full(R.N_NEIGHBOURS, -1, np.int32)
    m = int(r.integers(0, R.N_NEIGHBOURS + 1))
    near = [(e + o) % n_entries for o in (1, -1, 2, -2, 3, 5, 7, 11, 13, 17)]
    nb[:m] = near[:m]
    return nb


class ReferenceSession:
    """runs operations on tests/dbow_reference.py's KeyFrameDatabase; entries are KeyFrame objects that set_bow replaces (a new keyframe: state zero)"""

    def __init__(self, n_entries, levelsup=4):
        self.v = vocab(SESSION_VOCAB); self.levelsup = levelsup
        self.db = R.KeyFrameDatabase(self.v.n_words)
        empty = (np.zeros(0, np.uint32), np.zeros(0, np.float64))
        self.kf = [R.KeyFrame(0, empty, e) for e in range(n_entries)]
        self.nb = [np.full(R.N_NEIGHBOURS, -1, np.int32) for _ in range(n_entries)]

    def apply(self, op):
        if op[0] == "set_bow":
            t = self.v.transform(op[2], self.levelsup)
            self.kf[op[1]] = R.KeyFrame(0, (t[0], t[1]), op[1])
            return t
        if op[0] == "add":
            self.db.add(self.kf[op[1]])
        elif op[0] == "erase":
            self.db.erase(self.kf[op[1]])
        elif op[0] == "clear":
            self.db.clear()
        elif op[0] == "nb":
            self.nb[op[1]] = np.asarray(op[2], np.int32)
        elif op[0] == "query":
            _, kind, e, qid, conn, ms = op
            for o, nb in zip(self.kf, self.nb):
                o.neighbours = [self.kf[int(j)] for j in nb if j >= 0]
            q = self.kf[e]; q.mnId = qid; q.connected = set(self.kf[c] for c in conn)
            if kind == 0:
                out = self.db.DetectLoopCandidates(q, ms)
            elif kind == 1:
                out = self.db.DetectRelocalizationCandidates(q)
            else:
                out = self.db.DetectMapFusionCandidatesFromDB(q)
            return [o.name for o in out]
        return None

    def state(self):
        return state_array([o.state() for o in self.kf])


STATE_DTYPE = np.dtype([("loop_query", "<u8"), ("loop_words", "<i4"), ("loop_score", "<f4"), ("reloc_query", "<u8"), ("reloc_words", "<i4"), ("reloc_score", "<f4")])


def state_array(rows):
    a = np.zeros(len(rows), STATE_DTYPE)
    for i, s in enumerate(rows):
        a[i] = s
    return a


@functools.lru_cache(maxsize=None)
def session_expected(n_entries, steps=300, seed=0, rebow=True):
    """per operation: (result, state after it) for queries, the transform for set_bow, else None"""
    s = ReferenceSession(n_entries)
    out = []
    for op in session(n_entries, steps, seed, rebow):
        res = s.apply(op)
        out.append((res, s.state()) if op[0] == "query" else res)
    return out


def ints(tag, a):
    return tag + "".join(" %d" % int(x) for x in a)


def state_text(st):
    """the six fields per entry as the host programs print them: floats as bit patterns"""
    return ["st %d %d %08x %d %d %08x" % (s["loop_query"], s["loop_words"], int(s["loop_score"].view(np.uint32)), s["reloc_query"], s["reloc_words"], int(s["reloc_score"].view(np.uint32))) for s in st]

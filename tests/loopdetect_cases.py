"""Worlds for the DetectLoop tests (CPU and GPU): a covisibility map (covis_reference.Map), a BowVector per keyframe (dbow_reference.KeyFrame), a database with the
old keyframes in it, and a script of operations.  Everything is synthetic and chosen so that a test can say beforehand which keyframes a query finds:

  an OLD keyframe j owns the five words 5 j .. 5 j + 4, each with value 0.2, and is in the database from the start;
  a CURRENT keyframe (the ones DetectLoop is called for, in id order) holds the words of the old keyframes it `targets`, and two travel words of which it shares
  one with the current keyframe before it and one with the one after it, and the first word of the FILLER, an old keyframe every current keyframe is covisible
  with (weight 2) and hardly similar to: the filler's score is the minScore, low as after a real revisit, and a targeted old keyframe scores about
  1 / (number of targets);
  a current keyframe is connected to the three before it with weights 3, 2 and 1: with the threshold 2 of these tests the third is in the weight map
  (GetConnectedKeyFrames) but not in the ordered list (GetVectorCovisibleKeyFrames).

Covisibility comes from map points alone: an edge of weight w is w points seen by both keyframes, so the device builds the same rows with corb_covis_update."""
import functools

import numpy as np

import covis_reference as CR
import dbow_reference as DR
import loopdetect_reference as LR

TH = 2                          # UpdateConnections' threshold in these worlds
N_SLOTS = 96                    # the keyframe store of the GPU tests: two 64-bit words per group, the second half-used
MAX_CONNECTIONS = 72            # a small non-power of two above the hub's 70 connections
N_VOCAB_WORDS = 1000            # bow_cases.vocab("k10L3"): 10^3 leaves
TRAVEL0 = 700                   # travel words of the current keyframes
UNKNOWN = CR.NO_ID - 77         # an id the store never holds
PAD_FEATURES = 60
MAX_WORDS = 512                 # per database entry: room for a probe that holds every word of a world


def old_bow(j):
    return np.arange(5 * j, 5 * j + 5, dtype=np.uint32), np.full(5, 0.2, np.float64)


def cur_bow(k, targets, weight=None, n_words=5, filler=None):
    """current keyframe number k: the first n_words words of every target with weight[target] (1 by default), travel words k and k + 1 with 0.5, the filler's first
    word with 0.3; L1-normalised in ascending word order as BowVector::normalize does"""
    raw = {TRAVEL0 + k: 0.5, TRAVEL0 + k + 1: 0.5}
    if filler is not None:
        raw[5 * filler] = 0.3
    for t in targets:
        for w in range(5 * t, 5 * t + n_words):
            raw[w] = 1.0 if weight is None else float(weight[t])
    word = np.array(sorted(raw), np.uint32)
    value = np.array([raw[int(w)] for w in word], np.float64)
    norm = np.float64(0)
    for v in value:
        norm = norm + np.abs(v)
    return word, value / norm


class World:
    """old_edges: {(a, b): w} among old ids; currents: [(id, targets)] in id order; bad / unbound / not_live: sets of ids; extra_edges: {(a, b): w} between any two
    ids, UNKNOWN allowed as b; script: [("detect", id) | ("queue", [ids]) | ("last", id) | ("reset",) | ("clear",) | ("drop", id)]"""

    def __init__(self, old_ids, old_edges, currents, script, bad=(), unbound=(), not_live=(), extra_edges=None, neighbours=False, bows=None, seed=0, filler=None, no_filler=()):
        self.old_ids = list(old_ids); self.currents = list(currents); self.script = list(script)
        self.bad = set(bad); self.unbound = set(unbound); self.not_live = set(not_live); self.neighbours = neighbours
        self.cur_ids = [c for c, _ in self.currents]
        self.ids = sorted(self.old_ids + self.cur_ids)
        assert len(set(self.ids)) == len(self.ids) and max(self.old_ids) * 5 + 5 <= TRAVEL0 and TRAVEL0 + len(self.currents) + 2 <= N_VOCAB_WORDS
        edges = dict(old_edges)
        for k, c in enumerate(self.cur_ids):                        # the chain of the current keyframes
            for back, w in ((1, 3), (2, 2), (3, 1)):
                if k - back >= 0:
                    edges[(self.cur_ids[k - back], c)] = w
            if filler is not None and c not in no_filler:
                edges[(filler, c)] = 2
        edges.update(extra_edges or {})
        self.edges = edges
        self.words = {}
        for j in self.old_ids:
            self.words[j] = old_bow(j)
        for k, (c, targets) in enumerate(self.currents):
            self.words[c] = bows[c] if bows and c in bows else cur_bow(k, targets, filler=filler)
        rng = np.random.default_rng(seed)
        order = [self.ids[i] for i in rng.permutation(len(self.ids))]
        half = len(order) // 2
        first_b = max(70, half + 2) if len(order) < 60 else half + 2
        self.slot = {kid: (s if s < half else first_b + s - half) for s, kid in enumerate(order)}       # two runs of slots with empty ones between and behind
        assert max(self.slot.values()) < N_SLOTS
        self.order_a, self.order_b, self.first_b = order[:half], order[half:], first_b
        self.n_entries = len(self.ids) + 3
        ent = rng.permutation(self.n_entries)
        self.entry = {kid: int(ent[i]) for i, kid in enumerate(self.ids) if kid not in self.unbound}

    # ---- the definition's side ----
    def map(self):
        m = CR.Map()
        feats = {kid: [] for kid in self.ids}
        pid = 1000
        for (a, b), w in sorted(self.edges.items()):
            for _ in range(w):
                obs = {a: len(feats[a])}
                feats[a].append(pid)
                if b in feats:
                    obs[b] = len(feats[b]); feats[b].append(pid)
                else:
                    obs[b] = 0                                      # a keyframe the store does not hold
                m.mps[pid] = CR.MapPoint(pid, obs); pid += 1
        for kid in self.ids:
            f = feats[kid] + [CR.NO_ID] * max(PAD_FEATURES - len(feats[kid]), 1)
            m.kfs[kid] = CR.KeyFrame(kid, f, bad=kid in self.bad)
        for kid in self.ids:                                        # every keyframe connected once, in ascending id
            CR.update_connections(m, kid, TH)
        return m

    def reference(self, max_candidates=None, max_groups=None):
        """(LoopClosing, map, bow): a fresh definition of the world with the old keyframes in the database"""
        m = self.map()
        bow = {kid: DR.KeyFrame(kid, self.words[kid], kid) for kid in self.ids if kid not in self.unbound}
        db = DR.KeyFrameDatabase(N_VOCAB_WORDS)
        lc = LR.LoopClosing(m, db, bow, max_candidates, max_groups)
        for kid in bow:
            bow[kid].neighbours = [bow[i] for i in self.neighbour_ids(m, kid)]
        for j in self.old_ids:
            if j in bow and j not in self.not_live:
                db.add(bow[j]); lc.live.add(j)
        return lc, m, bow

    def neighbour_ids(self, m, kid):
        """GetBestCovisibilityKeyFrames(10) of a keyframe, those with a BowVector; none at all in a world without neighbours"""
        return [i for i in CR.get_best_covisibles(m, kid, 10) if i not in self.unbound] if self.neighbours else []


def run(world, lc=None, on_step=None):
    """the script on the definition: [(op, answer)] with answer = the DetectLoop dict, a list of them for a queue, "unbound" / "capacity" for the two errors, else None.
    After a DETECTED the caller's script says what CorrectLoop would (("last", id))."""
    lc = lc or world.reference()[0]
    out = []
    for op in world.script:
        ans = None
        try:
            if op[0] == "detect":
                ans = lc.DetectLoop(op[1])
            elif op[0] == "queue":
                ans = lc.DetectLoopQueue(op[1])
            elif op[0] == "last":
                lc.mLastLoopKFid = op[1]
            elif op[0] == "reset":
                lc.RequestReset()
            elif op[0] == "clear":
                lc.mvConsistentGroups = []
            elif op[0] == "drop":
                lc.drop(op[1])
        except LR.Unbound:
            ans = "unbound"
        except LR.Capacity:
            ans = "capacity"
        out.append((op, ans))
        if on_step:
            on_step(op, ans, lc)
    return out


# ---------------------------------------------------------------- hand-built worlds ----------------------------------------------------------------
# old keyframes 1 .. 7: 1 - 2 - 4 - 5 a chain (weights 3), 2 - 3 as well, 7 alone.  group(1) = {1, 2}, group(2) = {1, 2, 3, 4}, group(3) = {2, 3}, group(4) = {2, 4, 5},
# group(5) = {4, 5}, group(7) = {7}; 6 is the filler
OLD7 = dict(old_ids=[1, 2, 3, 4, 5, 6, 7], old_edges={(1, 2): 3, (2, 4): 3, (4, 5): 3, (2, 3): 3}, filler=6)


def _detects(ids):
    return [("detect", i) for i in ids]


@functools.lru_cache(maxsize=None)
def hand(name):
    if name == "sequence":                  # the counter runs 0, 1, 2, 3: DETECTED at the fourth keyframe
        return World(currents=[(100, [2]), (101, [2]), (102, [2]), (103, [2])], script=_detects([100, 101, 102, 103]), **OLD7)
    if name == "two_candidates_one_group":  # candidates 1 and 3 both meet the one previous group {1, 2, 3, 4}: only candidate 1 gives a group, both are enough
        return World(currents=[(100, [2]), (101, [2]), (102, [2]), (103, [1, 3])], script=_detects([100, 101, 102, 103]), **OLD7)
    if name == "one_candidate_two_groups":  # candidate 4 = {2, 4, 5} meets both previous groups, ({1, 2}, 1) and ({4, 5}, 0)
        return World(currents=[(100, [1]), (101, [1, 5]), (102, [4])], script=_detects([100, 101, 102]), **OLD7)
    if name == "no_connections":            # candidate 7 has no connection: its group is {7}
        return World(currents=[(100, [7])], script=_detects([100]), **OLD7)
    if name == "gap_and_none":              # GAP leaves the groups, NONE clears them
        return World(currents=[(100, [2]), (101, [2]), (102, []), (103, [2])], script=[("detect", 100), ("last", 95), ("detect", 101), ("reset",), ("detect", 103), ("detect", 102)], **OLD7)
    if name == "all_connected_bad":         # every covisible keyframe of 102 is bad: minScore stays 1 and nothing reaches it
        return World(currents=[(100, [2]), (101, [2]), (102, [2])], script=_detects([102]), bad={100, 101, 6}, **OLD7)
    if name == "unbound_covisible":         # 101 is covisible with 100, which has no BowVector entry
        return World(currents=[(100, [2]), (101, [2])], script=_detects([101]), unbound={100}, **OLD7)
    if name == "drop":                      # the stored group {7} loses 7: candidate 7 is no longer consistent with it
        return World(currents=[(100, [7]), (101, [7]), (102, [7]), (103, [7])], script=[("detect", 100), ("detect", 101), ("drop", 7), ("detect", 102), ("detect", 103)], **OLD7)
    if name == "hub":                       # old keyframe 71 is connected to 1 .. 70: a group of 71 slots; candidate 3 = {3, 71} meets it through 71 alone
        return World(old_ids=list(range(1, 73)), old_edges={(j, 71): 1 for j in range(1, 71)}, filler=72, currents=[(100, [71]), (101, [3])], script=_detects([100, 101]))
    raise KeyError(name)


HAND = ("sequence", "two_candidates_one_group", "one_candidate_two_groups", "no_connections", "gap_and_none", "all_connected_bad", "unbound_covisible", "drop", "hub")


# ---------------------------------------------------------------- seeded random walks ----------------------------------------------------------------
N_OLD, N_WALK, HUB, FILLER = 45, 40, 46, 47


@functools.lru_cache(maxsize=None)
def walk(seed):
    """45 old keyframes in a loose chain (j - j + 1 with weight 3, j - j + 2 with weight 1 or 2 at random, a few far edges), a hub (id 46) connected with weight 1 to
    every old keyframe and to the first 25 current ones: 70 connections, a group wider than 64 slots; a filler (id 47).  40 current keyframes whose ids step by 2 .. 5 revisit a place
    that drifts along the chain: each targets 0 .. 3 old keyframes near it, with random word weights and sometimes only four of a target's words.  Some current
    keyframes are bad, some old ones are not in the database, some rows name a keyframe the store does not hold.  The script detects the current keyframes in order and
    does what CorrectLoop does after a detection: mLastLoopKFid = that keyframe."""
    r = np.random.default_rng(9000 + seed)
    old = list(range(1, N_OLD + 1)) + [HUB, FILLER]
    edges = {}
    for j in range(1, N_OLD):
        edges[(j, j + 1)] = 3
        if j + 2 <= N_OLD and r.random() < 0.6:
            edges[(j, j + 2)] = int(r.integers(1, 3))
    for _ in range(8):
        a, b = sorted(int(x) for x in r.choice(np.arange(1, N_OLD + 1), 2, replace=False))
        edges.setdefault((a, b), int(r.integers(1, 4)))
    ids, kid = [], 100
    for _ in range(N_WALK):
        ids.append(kid); kid += int(r.integers(2, 6))
    extra = {(HUB, j): 1 for j in range(1, N_OLD + 1)}
    extra.update({(HUB, c): 1 for c in ids[:25]})
    for c in r.choice(ids, 5, replace=False):
        extra[(int(c), UNKNOWN)] = int(r.integers(1, 4))
    currents, bows, no_filler, place = [], {}, set(), int(r.integers(5, N_OLD - 5))
    for k, c in enumerate(ids):
        place = int(np.clip(place + r.integers(-1, 2), 3, N_OLD - 3)) if r.random() < 0.85 else int(r.integers(3, N_OLD - 3))
        n_t = 0 if r.random() < 0.25 else int(r.integers(1, 4))
        near = [place + o for o in (-2, -1, 0, 1, 2)] + ([HUB] if k >= 25 and r.random() < 0.2 else [])
        targets = sorted(int(t) for t in r.choice(near, min(n_t, len(near)), replace=False))
        currents.append((c, targets))
        weight = {t: float(r.uniform(0.7, 1.3)) for t in targets}
        if r.random() < 0.1:
            no_filler.add(c)                                        # no dissimilar covisible keyframe: minScore is high
        bows[c] = cur_bow(k, targets, weight, n_words=4 if r.random() < 0.1 else 5, filler=None if c in no_filler else FILLER)
    bad = set(int(c) for c in r.choice(ids, 4, replace=False))
    not_live = set(int(j) for j in r.choice(np.arange(1, N_OLD + 1), 4, replace=False))
    w = World(old, edges, currents, [], bad=bad, not_live=not_live, extra_edges=extra, neighbours=True, bows=bows, seed=seed, filler=FILLER, no_filler=no_filler)
    script, lc = [], w.reference()[0]
    for c in ids:                                                   # the script depends on the outcomes: written once, from the definition
        script.append(("detect", c))
        if lc.DetectLoop(c)["outcome"] == LR.DETECTED:
            script.append(("last", c)); lc.mLastLoopKFid = c
    w.script = script
    return w


WALK_SEEDS = (1, 12, 23)         # chosen by tests/test_loopdetect_reference.py's counts: every outcome at least three times per walk


# ---------------------------------------------------------------- the world on the device ----------------------------------------------------------------
class Dev:
    """the world in a KeyFrameStore of N_SLOTS slots, a MapPointStore, the graph over them (rows by corb_covis_update in ascending id), and per `fresh()` a new
    KeyFrameDatabase holding the old keyframes with a LoopDetector bound to it"""

    def __init__(self, corb, voc, world, F=96):
        import covis_cases as G
        self.corb = corb; self.voc = voc; self.w = world; self.m = world.map()
        m = self.m
        mp_order = sorted(m.mps)
        self.KF = corb.KeyFrameStore(N_SLOTS, F); self.MP = corb.MapPointStore(max(len(mp_order), 1), 4)
        for first, order in ((0, world.order_a), (world.first_b, world.order_b)):
            if not order:
                continue
            a = G.arrays(m, order, [])
            meta = np.zeros(len(order), corb.KF_META_DTYPE); meta["id"] = a["kf_ids"]; meta["nlevels"] = 8
            for s in range(len(order)):
                meta["Tcw"][s] = np.eye(4, dtype=np.float32).reshape(16); meta["TcwGBA"][s] = np.eye(4, dtype=np.float32).reshape(16)
            kp = np.zeros(len(a["mp_id"]), corb.KP_DTYPE)
            self.KF.put_batch(first, meta, a["feat_off"], kp, None, a["u_right"], a["depth"], a["mp_id"])
        a = G.arrays(m, [], mp_order)
        rec = np.zeros(len(mp_order), corb.MP_RECORD_DTYPE); rec["id"] = a["mp_ids"]; rec["n_obs"] = np.diff(a["obs_off"]); rec["ref_kf_id"] = CR.NO_ID
        self.MP.put(0, rec, a["obs_off"], a["obs_kf"], a["obs_idx"]); self.MP.build_index(0, len(mp_order))
        self.g = corb.Covisibility(self.KF, self.MP, MAX_CONNECTIONS)
        self.g.UpdateConnections([world.slot[k] for k in world.ids], th=TH)
        for k in world.ids:
            assert list(self.g.get(world.slot[k])[1][0]) == [i for i, _ in m.kfs[k].ordered], k
        for k in world.bad:
            self.KF.set_meta(world.slot[k], flags=1)
        self.id_of_slot = {s: k for k, s in world.slot.items()}
        self.id_of_entry = {e: k for k, e in world.entry.items()}
        self.db = self.det = None

    def fresh(self, max_candidates=8, max_groups=16, bind=True):
        w = self.w; corb = self.corb
        self.drop()
        self.db = self.new_db()
        self.det = corb.LoopDetector(self.g, self.db, max_candidates, max_groups)
        if bind:
            self.det.bind([w.slot[k] for k in w.entry], [w.entry[k] for k in w.entry])
        return self.det

    def new_db(self):
        """a second database with the same content as fresh() starts from"""
        w = self.w
        db = self.corb.KeyFrameDatabase(self.voc, w.n_entries, MAX_WORDS)
        for kid, e in w.entry.items():
            db.set_bow(e, *w.words[kid])
            nb = [w.entry[i] for i in w.neighbour_ids(self.m, kid)]
            db.set_neighbours(e, nb + [-1] * (10 - len(nb)))
        for j in w.old_ids:
            if j in w.entry and j not in w.not_live:
                db.add(w.entry[j])
        return db

    def groups(self, det=None):
        return [(sorted(self.id_of_slot[s] for s in mem), c) for mem, c in (det or self.det).get_groups()]

    def drop(self):
        for h in (self.det, self.db):
            if h is not None:
                h.close()
        self.det = self.db = None

    def close(self):
        self.drop(); self.g.close(); self.KF.close(); self.MP.close()


def stats(world):
    """how often the definition alone takes each outcome on the world's script, and how often the consistency pass meets its two special cases: a candidate consistent
    with two previous groups (`cand_two_groups`), a previous group met by two candidates (`group_two_cands`).  Also checks the closed form against the serial loop."""
    import collections
    lc = world.reference()[0]
    c = collections.Counter()
    previous = []

    def on_step(op, ans, lc):
        nonlocal previous
        if isinstance(ans, dict):
            c[ans["outcome"]] += 1
            if ans["candidates"]:
                groups = [(lc.connected(k) | {k}) if k in lc.m.kfs else set() for k in ans["candidates"]]
                cons = [[bool(g & p) for p, _ in previous] for g in groups]
                c["cand_two_groups"] += sum(1 for row in cons if sum(row) >= 2)
                c["group_two_cands"] += sum(1 for g in range(len(previous)) if sum(row[g] for row in cons) >= 2)
                new, enough = LR.closed_form(groups, previous)
                assert [(sorted(s), n) for s, n in new] == ans["groups"] and enough == ans["enough"]
        previous = [(set(s), n) for s, n in lc.mvConsistentGroups]

    run(world, lc, on_step)
    return c

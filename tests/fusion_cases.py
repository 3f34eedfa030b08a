"""Seeded generators for the whole-submap detection tests (CPU and GPU), on top of tests/bow_cases.py.  Expected values come from tests/fusion_reference.py alone and
are computed once per process; tests/test_fusion_reference.py asserts the conditions the generators are kept for on the definition's side."""
import functools
import numpy as np
import bow_cases as G
import dbow_reference as R
import fusion_reference as F

EXTRA = 4                       # entries behind the populated ones that are never added: three hold the BowVector of random descriptors (the "random" queries),
                                # the last one a single word that no populated entry holds (a query without a candidate)
FIRST_ID = 100


def populate_ops(n):
    """the operations bow_cases.session(n) populates its database with: every set_bow, then add (most entries) and nb per entry"""
    out, nbs = [], 0
    for op in G.session(n):
        if nbs == n:
            break
        assert op[0] in ("set_bow", "add", "nb")
        out.append(op); nbs += op[0] == "nb"
    return out


@functools.lru_cache(maxsize=None)
def database(n):
    """(Db of n + EXTRA entries, the operations that build it on a device: ("set_bow", e, word, value) / ("add", e) / ("nb", e, nb[10]))"""
    v = G.vocab(G.SESSION_VOCAB)
    db = F.Db(n + EXTRA); ops = []
    for op in populate_ops(n):
        if op[0] == "set_bow":
            t = v.transform(op[2], 4); db.set_bow(op[1], t[0], t[1]); ops.append(("set_bow", op[1], t[0], t[1]))
        elif op[0] == "add":
            db.add(op[1]); ops.append(op)
        else:
            db.set_neighbours(op[1], op[2]); ops.append(op)
    for k in range(EXTRA - 1):
        t = v.transform(G.features(G.SESSION_VOCAB, 50 + 7 * k, 4100 + 10 * n + k), 4)
        db.set_bow(n + k, t[0], t[1]); ops.append(("set_bow", n + k, t[0], t[1]))
    used = set(int(w) for b in db.bow if b is not None for w in b[0])
    lone = (np.array([min(w for w in range(v.n_words) if w not in used)], np.uint32), np.array([1.0]))
    db.set_bow(n + EXTRA - 1, *lone); ops.append(("set_bow", n + EXTRA - 1) + lone)
    return db, ops


def queries(n, with_random=True):
    """every entry once forward and once backward, then the random ones; ids FIRST_ID + position"""
    e = list(range(n)) + list(range(n - 1, -1, -1)) + (list(range(n, n + EXTRA)) if with_random else [])
    return np.array(e, np.int32), (FIRST_ID + np.arange(len(e))).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def expected(n, with_random=True):
    """(offsets, candidates, events, state after) of the batch on database(n)"""
    db = database(n)[0].copy()
    off, cand, ev = F.detect_batch(db, *queries(n, with_random))
    return off, cand, ev, db.state


def repeat_queries(state):
    """a second call on database(70) after queries(70): its first id is the one the first call left in entry 3 (and in the entries that met the same query), so
    those visits add to the count and push nothing; entry 3 is listed twice under different ids"""
    return np.array([3, 3, 9], np.int32), np.array([int(state["reloc_query"][3]), 7, 8], np.uint64)


def build(corb, voc, n, max_words=128):
    """database(n) on the device"""
    db = corb.KeyFrameDatabase(voc, n + EXTRA, max_words)
    apply_ops(db, database(n)[1])
    return db


def apply_ops(db, ops):
    for op in ops:
        if op[0] == "set_bow":
            db.set_bow(op[1], op[2], op[3])
        elif op[0] == "add":
            db.add(op[1])
        else:
            db.set_neighbours(op[1], op[2])


# ---- BowVectors of more than 64 words: several ballot rounds per entry, several search steps per word ----
WIDE_VOCAB = "k10L4"
WIDE_N = 6


@functools.lru_cache(maxsize=None)
def wide_database():
    v = G.vocab(WIDE_VOCAB)
    db = F.Db(WIDE_N); ops = []
    r = np.random.default_rng(77)
    for e in range(WIDE_N):
        t = v.transform(G.features(WIDE_VOCAB, 420 + 30 * e, 5200 + e % 3, pool=150), 4)      # entries e and e + 3 see the same place
        db.set_bow(e, t[0], t[1]); ops.append(("set_bow", e, t[0], t[1]))
    for e in range(WIDE_N):
        if e != 4:
            db.add(e); ops.append(("add", e))
        nb = G._neighbours(r, e, WIDE_N); db.set_neighbours(e, nb); ops.append(("nb", e, nb))
    return db, ops


def wide_queries():
    e = list(range(WIDE_N)) + list(range(WIDE_N - 1, -1, -1))
    return np.array(e, np.int32), (FIRST_ID + np.arange(len(e))).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def wide_expected():
    db = wide_database()[0].copy()
    off, cand, ev = F.detect_batch(db, *wide_queries())
    return off, cand, ev, db.state


# ---- the chain: a global map of 70 keyframes with map points, a submap of 12 keyframes that see some of them again ----
N_GLOBAL, N_SUB, CHAIN_F = 70, 12, 160
FV_LEVELSUP = 2                 # FeatureVector nodes one level below the root of k10L3: ten nodes, so a pair has several in common


@functools.lru_cache(maxsize=None)
def chain_case(seed=5):
    """dict: glob / sub = {slot: dict(n, desc, angle, mp_id, bad, fv, bow)}, entry_slot[N_GLOBAL + N_SUB], slot_of_global[g], query_slots / query_entries / query_ids,
    db (F.Db) and its device operations"""
    v = G.vocab(G.SESSION_VOCAB)
    r = np.random.default_rng(9000 + seed)
    n_places = 10
    places = [v.words[r.integers(0, v.n_words, 40)] for _ in range(n_places)]

    def flip(d, bits):
        d = d.copy()
        for b in r.choice(256, bits, replace=False):
            d[b >> 3] ^= np.uint8(1 << (b & 7))
        return d

    def record(desc, angle, mp_id, bad):
        t = v.transform(desc, FV_LEVELSUP)
        return dict(n=len(desc), desc=desc, angle=angle.astype(np.float32), mp_id=mp_id, bad=bad, fv=(t[2], t[3], t[4]), bow=(t[0], t[1]))

    empty = record(np.zeros((0, 32), np.uint8), np.zeros(0, np.float32), np.zeros(0, np.uint64), False)
    bad_g, no_slot_g, empty_g = {17, 33}, {5, 29}, {41}
    glob, place_of, slot_of = {}, [], {}
    for g in range(N_GLOBAL):
        p = g % n_places; place_of.append(p)
        m = int(r.integers(90, CHAIN_F - 20))
        desc = np.stack([flip(v.descriptor[int(places[p][r.integers(0, 40)])], 30) for _ in range(m)])
        mp = np.where(r.random(m) < 0.85, 1000 * (g + 1) + np.arange(m), F.NO_MAP_POINT).astype(np.uint64)
        rec = record(desc, r.uniform(0, 360, m), mp, g in bad_g)
        if g not in no_slot_g:
            slot_of[g] = (g * 11 + 3) % N_GLOBAL
            glob[slot_of[g]] = rec if g not in empty_g else dict(empty, bow=rec["bow"])
        else:
            glob[-1 - g] = rec                              # (held for its BowVector only)
    twins = [0, 3, 5, 8, 12, 17, 21, 29, 33, 41, 50, 64]    # the global keyframe each sub keyframe sees again: two bad ones, two without a record, one without features
    sub = {}
    for s, g in enumerate(twins):
        src = glob[slot_of[g]] if g in slot_of and g not in empty_g else glob.get(-1 - g)
        if src is None or src["n"] == 0:                    # the keyframe whose record is empty: seen from its place
            p = place_of[g]
            desc = np.stack([flip(v.descriptor[int(places[p][r.integers(0, 40)])], 30) for _ in range(100)]); ang = r.uniform(0, 360, 100)
        else:
            keep = np.nonzero(r.random(src["n"]) < 0.9)[0]; r.shuffle(keep)
            desc = np.stack([flip(src["desc"][j], 8) for j in keep]); ang = (src["angle"][keep] + r.normal(0, 3, len(keep))) % 360
        sub[N_SUB - 1 - s] = record(desc, ang, np.full(len(desc), F.NO_MAP_POINT, np.uint64), False)
    db = F.Db(N_GLOBAL + N_SUB); ops = []
    entry_slot = np.full(N_GLOBAL + N_SUB, -1, np.int32)
    for g in range(N_GLOBAL):
        rec = glob[slot_of[g]] if g in slot_of else glob[-1 - g]
        db.set_bow(g, *rec["bow"]); ops.append(("set_bow", g) + rec["bow"])
        entry_slot[g] = slot_of.get(g, -1)
    for g in range(N_GLOBAL):
        db.add(g); ops.append(("add", g))
        nb = G._neighbours(r, g, N_GLOBAL); db.set_neighbours(g, nb); ops.append(("nb", g, nb))
    for s in range(N_SUB):
        rec = sub[N_SUB - 1 - s]
        db.set_bow(N_GLOBAL + s, *rec["bow"]); ops.append(("set_bow", N_GLOBAL + s) + rec["bow"])
    glob = {k: x for k, x in glob.items() if k >= 0}
    return dict(glob=glob, sub=sub, entry_slot=entry_slot, db=db, ops=ops, twins=twins, bad=bad_g, no_slot=no_slot_g,
                query_slots=np.array([N_SUB - 1 - s for s in range(N_SUB)], np.int32), query_entries=np.arange(N_GLOBAL, N_GLOBAL + N_SUB, dtype=np.int32),
                query_ids=(5000 + 3 * np.arange(N_SUB)).astype(np.uint64))


@functools.lru_cache(maxsize=None)
def chain_expected(seed=5):
    """(rows, offsets, ids, state after) from the definition, SearchByBoW by the oracle"""
    from oracle import pyorc
    pyorc.build()
    c = chain_case(seed)
    db = c["db"].copy()
    off, cand, _ = F.detect_batch(db, c["query_entries"], c["query_ids"])

    def search(gs, ss):
        a, b = c["glob"][gs], c["sub"][ss]
        if a["n"] == 0 or b["n"] == 0:
            return np.full(b["n"], -1, np.int32), 0
        valid = (a["mp_id"] != F.NO_MAP_POINT).astype(np.uint8)
        m, n = pyorc.search_by_bow(0, a["desc"], a["angle"], valid, pyorc.FeatVec(*a["fv"]), b["desc"], b["angle"], np.ones(b["n"], np.uint8), pyorc.FeatVec(*b["fv"]), 0.75, 1)
        return np.asarray(m, np.int32), int(n)
    rows, ids = F.chain(off, cand, c["query_slots"], c["entry_slot"], c["sub"], c["glob"], search)
    return rows, off, ids, db.state


CAM = (718.856, 718.856, 607.19, 185.21, 386.0)          # fx, fy, cx, cy, bf of every record
POSE_QUERY = 1                                              # the keyframe of the submap whose matched map points lie where it sees them: the PnP RANSAC finds its pose


def keypoints(corb, x, first_id, slot):
    """a record's keypoints: its angles, and seeded positions and octaves (what the PnP RANSAC reads of the frame)"""
    kp = np.zeros(x["n"], corb.KP_DTYPE); kp["angle"] = x["angle"]
    r = np.random.default_rng(600 + first_id + slot)
    kp["x"], kp["y"], kp["octave"] = r.uniform(0, 1241, x["n"]), r.uniform(0, 376, x["n"]), r.integers(0, 8, x["n"])
    return kp


STORE_IDS = (1, 9001)                                       # keyframe id = first id of the store + slot: global, sub


def fill_stores(corb, c):
    """the chain case's two keyframe stores on the device"""
    glob = corb.KeyFrameStore(N_GLOBAL, CHAIN_F); sub = corb.KeyFrameStore(N_SUB, CHAIN_F)
    for store, recs, first_id in ((glob, c["glob"], STORE_IDS[0]), (sub, c["sub"], STORE_IDS[1])):
        for slot, x in recs.items():
            if x["n"] == 0:
                continue
            store.put(slot, keypoints(corb, x, first_id, slot), x["desc"], keyframe_id=first_id + slot); store.set_bow(slot, x["fv"])
            store.set_map_points(slot, x["mp_id"]); store.set_flags(slot, (x["mp_id"] != F.NO_MAP_POINT).astype(np.uint8))
            store.set_meta(slot, flags=corb.KF_BAD if x["bad"] else 0, fx=CAM[0], fy=CAM[1], cx=CAM[2], cy=CAM[3], bf=CAM[4], nlevels=8, client_id=1)
    return glob, sub


def pnp_records(corb, c, best_first=False):
    """the map-point records of every kept row's keyframe (MP_RECORD_DTYPE): seeded positions in front of the camera, but the points matched to keyframe POSE_QUERY
    of the submap lie exactly where that keyframe sees them from the identity pose, so its PnP RANSAC returns a refined pose.  best_first: of the points matched to
    keyframe 0, exactly mRansacMinInliers = int(0.5 N) lie where it sees them -- a hypothesis through four of them has that many inliers and enters the record, but its
    Refine() needs MORE than that many (PnPsolver.cc:341), so iterate() ends with bNoMore and the running best: the walk stops at keyframe 0 with mBestTcw"""
    rows, off, ids, _ = chain_expected()
    slots = sorted(set(r[2] for r in rows if r[4]))
    mp = np.concatenate([c["glob"][s]["mp_id"][c["glob"][s]["mp_id"] != F.NO_MAP_POINT] for s in slots])
    r = np.random.default_rng(77)
    rec = np.zeros(len(mp), corb.MP_RECORD_DTYPE)
    rec["id"] = mp; rec["world_pos"] = np.stack([r.uniform(-5, 5, len(mp)), r.uniform(-2, 2, len(mp)), r.uniform(4, 30, len(mp))], axis=1); rec["client_id"] = 1
    at = dict((int(i), k) for k, i in enumerate(mp))
    for query, part in ((POSE_QUERY, 1.0),) + (((0, 0.5),) if best_first else ()):
        row = next(x for x in rows if x[0] == query and x[4])
        slot = int(c["query_slots"][query]); kp = keypoints(corb, c["sub"][slot], STORE_IDS[1], slot)
        matched = [iF for iF in range(c["sub"][slot]["n"]) if int(ids[row[5] + iF]) != F.NO_MAP_POINT]
        for iF in matched[: int(part * len(matched))]:
            z = np.float32(6 + iF % 17)
            rec["world_pos"][at[int(ids[row[5] + iF])]] = [(kp["x"][iF] - CAM[2]) * z / CAM[0], (kp["y"][iF] - CAM[3]) * z / CAM[1], z]
    return rec


def camera(corb):
    return corb.TrackCamera.make(CAM[0], CAM[1], CAM[2], CAM[3], CAM[4], 0.537, 0.0, 1241.0, 0.0, 376.0, (np.float32(1.2) ** np.arange(8)).astype(np.float32))


def pnp_world(corb, c, best_first=False):
    """pnp_records in a map-point store with its id index, and the camera"""
    rec = pnp_records(corb, c, best_first)
    MP = corb.MapPointStore(len(rec) + 4, 4)
    MP.put(0, rec, np.zeros(len(rec) + 1, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint32)); MP.build_index(0, len(rec))
    return MP, camera(corb)


def pnp_draws(n=8 * 300 * 4):
    """the draws of one keyframe's solvers (the same for every keyframe)"""
    return np.random.default_rng(3).integers(0, 1 << 30, n).astype(np.int32)

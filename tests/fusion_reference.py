"""The definition of map-fusion detection for a whole submap (include/corb_map_fusion.h), on top of tests/dbow_reference.py and the oracle's SearchByBoW.

Two statements of the database part, held equal by tests/test_fusion_reference.py:
  * one_by_one(): the queries through dbow_reference.KeyFrameDatabase._reloc one after the other -- the reference's text, the meaning of the batch;
  * detect_batch(): the same result computed the way the batch call computes it, stage by stage over all queries: words in common per (query, entry); one walk per
    entry over the queries in order carrying mnRelocQuery / mnRelocWords; the scores of the pairs that pass minCommonWords; a second walk carrying mRelocScore, which
    gives the score each query's accumulation SEES in a neighbour (a neighbour that shares a word with the query but was not scored for it adds the score an earlier
    query left: the stale-score quirk); the selection per query.  It also counts the events the generators' conditions are about.
The chain (rows, kept, ids) is stated once, in chain(), on the result of either.
"""
import numpy as np
import dbow_reference as R

NO_MAP_POINT = 0xFFFFFFFFFFFFFFFF
STATE_DTYPE = np.dtype([("loop_query", "<u8"), ("loop_words", "<i4"), ("loop_score", "<f4"), ("reloc_query", "<u8"), ("reloc_words", "<i4"), ("reloc_score", "<f4")])


class Db:
    """a keyframe database as plain data: what corb_kfdb_set_bow / add / erase / set_neighbours keep per entry"""

    def __init__(self, n):
        empty = (np.zeros(0, np.uint32), np.zeros(0, np.float64))
        self.n = n; self.bow = [None] * n; self.live = [False] * n; self.seq = [0] * n; self.next_seq = 1
        self.nb = [np.full(R.N_NEIGHBOURS, -1, np.int32) for _ in range(n)]; self.state = np.zeros(n, STATE_DTYPE); self._empty = empty

    def set_bow(self, e, word, value):
        assert not self.live[e]
        self.bow[e] = (np.asarray(word, np.uint32), np.asarray(value, np.float64)); self.state[e] = np.zeros((), STATE_DTYPE)

    def add(self, e):
        assert self.bow[e] is not None and not self.live[e]
        self.live[e] = True; self.seq[e] = self.next_seq; self.next_seq += 1

    def set_neighbours(self, e, nb):
        self.nb[e] = np.asarray(nb, np.int32).copy()

    def copy(self):
        o = Db(self.n); o.bow = list(self.bow); o.live = list(self.live); o.seq = list(self.seq); o.next_seq = self.next_seq
        o.nb = [b.copy() for b in self.nb]; o.state = self.state.copy()
        return o


def one_by_one(db, entries, ids):
    """the queries through the reference's text, one after the other; db.state is updated -> list of candidate lists"""
    kfs = []
    for e in range(db.n):
        k = R.KeyFrame(0, db.bow[e] if db.bow[e] is not None else db._empty, e)
        s = db.state[e]
        k.mnLoopQuery, k.mnLoopWords, k.mLoopScore = int(s["loop_query"]), int(s["loop_words"]), np.float32(s["loop_score"])
        k.mnRelocQuery, k.mnRelocWords, k.mRelocScore = int(s["reloc_query"]), int(s["reloc_words"]), np.float32(s["reloc_score"])
        kfs.append(k)
    for e in range(db.n):
        kfs[e].neighbours = [kfs[int(j)] for j in db.nb[e] if j >= 0]
    n_words = 1 + max([int(b[0].max()) for b in db.bow if b is not None and len(b[0])], default=0)
    rdb = R.KeyFrameDatabase(n_words)
    for e in sorted((e for e in range(db.n) if db.live[e]), key=lambda e: db.seq[e]):        # the inverted file's lists are in insertion order
        rdb.add(kfs[e])
    out = []
    for e, i in zip(entries, ids):
        q = R.KeyFrame(int(i), kfs[int(e)].bow)          # (the query's own fields are not read: only mnId and mBowVec)
        out.append([o.name for o in rdb.DetectMapFusionCandidatesFromDB(q)])
    for e in range(db.n):
        db.state[e] = kfs[e].state()
    return out


def detect_batch(db, entries, ids):
    """the batch, stage by stage -> (offsets, candidates, events); db.state is updated.  events: queries, candidates, stale_additions (a neighbour that was not
    scored for the query added a non-zero score), stale_best (times such a neighbour took the place of the best keyframe in an accumulation), stale_best_queries
    (queries after whose accumulations such a neighbour IS the best keyframe of a scored entry), none (queries without a candidate), three (queries with three or more)"""
    nq, n = len(entries), db.n
    assert len(set(int(i) for i in ids)) == nq, "query ids must be pairwise distinct"
    common = np.zeros((nq, n), np.int64); first = np.zeros((nq, n), np.int64)
    for q in range(nq):                                  # (a)
        qw = db.bow[int(entries[q])][0]
        for e in range(n):
            if db.live[e] and len(db.bow[e][0]):
                c = np.intersect1d(qw, db.bow[e][0])
                common[q, e] = len(c); first[q, e] = int(c[0]) if len(c) else 0
    pushed = np.zeros((nq, n), bool); words = np.zeros((nq, n), np.int64); id_match = np.zeros((nq, n), bool); max_common = np.zeros(nq, np.int64)
    for e in range(n):                                   # (b) one walk per entry
        rq, rw = int(db.state["reloc_query"][e]), int(db.state["reloc_words"][e])
        for q in range(nq):
            if common[q, e] > 0:
                if rq != int(ids[q]):
                    rq, rw = int(ids[q]), int(common[q, e]); pushed[q, e] = True
                else:
                    rw += int(common[q, e])
            words[q, e] = rw; id_match[q, e] = rq == int(ids[q])
            if pushed[q, e]:
                max_common[q] = max(max_common[q], rw)
        db.state["reloc_query"][e] = rq; db.state["reloc_words"][e] = rw
    scored = np.zeros((nq, n), bool); score = np.zeros((nq, n), np.float32)
    for q in range(nq):                                  # (c)
        min_common = int(np.float32(max_common[q]) * np.float32(0.8))
        for e in range(n):
            if pushed[q, e] and words[q, e] > min_common:
                scored[q, e] = True; score[q, e] = np.float32(R.score(db.bow[int(entries[q])], db.bow[e]))
    seen = np.zeros((nq, n), np.float32)
    for e in range(n):                                   # (d) the walk once more
        cur = np.float32(db.state["reloc_score"][e])
        for q in range(nq):
            if scored[q, e]:
                cur = score[q, e]
            seen[q, e] = cur
        db.state["reloc_score"][e] = cur
    offsets, cands = [0], []
    ev = dict(queries=nq, candidates=0, stale_additions=0, stale_best=0, stale_best_queries=0, none=0, three=0)
    for q in range(nq):                                  # (e)
        order = sorted((e for e in range(n) if scored[q, e]), key=lambda e: (first[q, e], db.seq[e]))
        acc, best_acc, stale_best = [], np.float32(0), False
        for e in order:
            best_score = a = score[q, e]; best = e
            for e2 in db.nb[e]:
                if e2 < 0 or not id_match[q, e2]:
                    continue
                a = np.float32(a + seen[q, e2])
                if not scored[q, e2] and seen[q, e2] != 0:
                    ev["stale_additions"] += 1
                if seen[q, e2] > best_score:
                    ev["stale_best"] += not scored[q, e2]
                    best, best_score = int(e2), seen[q, e2]
            stale_best |= best != e and not scored[q, best]
            acc.append((a, best))
            if a > best_acc:
                best_acc = a
        keep = np.float32(np.float32(0.75) * best_acc); out = []
        for a, b in acc:
            if a > keep and b not in out:
                out.append(b)
        cands += out; offsets.append(len(cands))
        ev["candidates"] += len(out); ev["stale_best_queries"] += bool(stale_best); ev["none"] += not out; ev["three"] += len(out) >= 3
    return np.array(offsets, np.int32), np.array(cands, np.int32), ev


def chain(offsets, cands, query_slots, entry_slot, sub, glob, search, min_matches=15):
    """rows, kept and ids of corb_map_fusion_candidates_store from a detection's (offsets, cands).  sub / glob: {slot: dict(n=features, bad=bool, mp_id=u64[n])};
    search(global slot, sub slot) -> (match[n(sub slot)], n_matches), SearchByBoW variant 0.  -> (rows as tuples (query, entry, slot, n_matches, kept, ids_offset), ids)"""
    rows, ids = [], []
    for i in range(len(query_slots)):
        nq = sub[int(query_slots[i])]["n"]
        for e in cands[offsets[i]:offsets[i + 1]]:
            slot = int(entry_slot[int(e)]); nm = 0; m = None
            if slot >= 0:
                m, nm = search(slot, int(query_slots[i]))
            kept = slot >= 0 and glob[slot]["n"] > 0 and not glob[slot]["bad"] and nm >= min_matches
            rows.append((i, int(e), slot, int(nm), int(kept), len(ids) if kept else -1))
            if kept:
                mp = glob[slot]["mp_id"]
                ids += [int(mp[j]) if j >= 0 else NO_MAP_POINT for j in m[:nq]]
    return rows, np.array(ids, np.uint64)


def rows_text(rows, offsets, ids):
    """what the host program of the adapter prints"""
    out = ["offsets" + "".join(" %d" % o for o in offsets)]
    out += ["row %d %d %d %d %d %d" % tuple(r) for r in rows]
    out.append("ids" + "".join(" %x" % int(i) for i in ids))
    return out

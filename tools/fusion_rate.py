"""Host-to-host time of map-fusion detection for a whole submap (include/corb_map_fusion.h): corb_map_fusion_candidates_store for submaps of 1, 16 and 256
keyframes against a global database of 2 000 entries (keyframes of 2 000 features, BowVectors of the size the 10^4-word vocabulary k10L4 gives them), the median
of 30 calls with the 10th and 90th percentile.

Beside it stands the earlier route through the single calls, in the same process, on the same data and alternating with it: corb_kfdb_detect per keyframe,
corb_search_by_bow_slots per (candidate, keyframe) pair, the discards and the ids gathered on the host (from host copies of the records' ids and flags, which
favours the earlier route).  The two routes run on twin databases with the same query ids (fresh ids every repeat: a repeated id pushes nothing) and must leave
the same rows, ids and database fields; the tool fails if they do not.  No ratio is fixed.  Results: profiles/fusion_rate.json and one JSON line.
      python tools/fusion_rate.py [--entries 2000] [--features 2000] [--repeats 30]"""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import corbload                                                            # noqa: E402
import bow_cases as G                                                      # noqa: E402

VOCAB, PER_PLACE, BATCH = "k10L4", 10, 100


def flipped(rng, desc, bits):
    """desc with `bits` random bit positions per row flipped"""
    out = desc.copy()
    pos = rng.integers(0, 256, (len(desc), bits))
    for k in range(bits):
        out[np.arange(len(desc)), pos[:, k] >> 3] ^= (1 << (pos[:, k] & 7)).astype(np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=2000); ap.add_argument("--features", type=int, default=2000); ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--submaps", default="1,16,256"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_rate.json"))
    a = ap.parse_args()
    corb = corbload.load_pkg()
    v = G.vocab(VOCAB); f = v.flat()
    voc = corb.Vocabulary(f["k"], f["L"], f["parent"], f["is_leaf"], f["descriptor"], f["weight"])
    rng = np.random.default_rng(1)
    N, F = a.entries, a.features
    sizes = [int(s) for s in a.submaps.split(",")]; K = max(sizes)
    n_places = (N + PER_PLACE - 1) // PER_PLACE
    leaves = v.descriptor[v.words]
    scenes = [flipped(rng, leaves[rng.integers(0, len(leaves), F)], 30) for _ in range(n_places)]          # a place: F scene points near vocabulary words
    glob = corb.KeyFrameStore(N, F); sub = corb.KeyFrameStore(K, F)
    dbs = [corb.KeyFrameDatabase(voc, N + K, F) for _ in range(2)]
    mp_host, bad_host = [], np.zeros(N, bool)

    def fill(store, first, count, place_of, first_id, with_points):
        for b0 in range(0, count, BATCH):
            n = min(BATCH, count - b0)
            meta = np.zeros(n, corb.KF_META_DTYPE); meta["id"] = first_id + b0 + np.arange(n); meta["nlevels"] = 8
            desc = np.concatenate([flipped(rng, scenes[place_of(b0 + k)], 8) for k in range(n)])
            kp = np.zeros(n * F, corb.KP_DTYPE); kp["angle"] = rng.uniform(0, 360, n * F)
            mp = np.where(rng.random(n * F) < 0.85, (first_id + b0) * F + np.arange(n * F), corb.NO_MAP_POINT).astype(np.uint64) if with_points else np.full(n * F, corb.NO_MAP_POINT, np.uint64)
            store.put_batch(first + b0, meta, (np.arange(n + 1) * F).astype(np.int32), kp, desc, mp_id=mp)
            for k in range(n):
                if with_points:
                    store.set_flags(first + b0 + k, (mp[k * F:(k + 1) * F] != corb.NO_MAP_POINT).astype(np.uint8)); mp_host.append(mp[k * F:(k + 1) * F])
            slots = np.arange(first + b0, first + b0 + n, dtype=np.int32)
            for db in dbs:
                store.compute_bow(slots, voc, 2, db, slots + (0 if with_points else N))
    fill(glob, 0, N, lambda g: g % n_places, 1, True)
    twin = rng.permutation(N)[:K]
    fill(sub, 0, K, lambda s: int(twin[s]) % n_places, 10 ** 6, False)
    nb = np.stack([G._neighbours(rng, e, N) for e in range(N)])
    for db in dbs:
        for e in range(N):
            db.add(e)
        db.set_neighbours(np.arange(N, dtype=np.int32), nb)
    entry_slot = np.concatenate([np.arange(N), np.full(K, -1)]).astype(np.int32)
    words = [len(dbs[0].get_bow(e)[0]) for e in range(0, N, max(N // 20, 1))]

    def earlier(db, slots, entries, ids):
        rows, out, off = [], [], [0]
        for i, (qs, qe, qi) in enumerate(zip(slots, entries, ids)):
            for e in db.detect(2, int(qe), int(qi)):
                slot = int(entry_slot[e]); nm = 0; kept = False
                if slot >= 0:
                    m, nm = glob.SearchByBoW(slot, sub, int(qs), 0.75, True, 0)
                    kept = not bad_host[slot] and nm >= 15
                rows.append((i, int(e), slot, nm, int(kept), sum(len(x) for x in out) if kept else -1))
                if kept:
                    out.append(np.where(m >= 0, mp_host[slot][np.maximum(m, 0)], np.uint64(corb.NO_MAP_POINT)))
            off.append(len(rows))
        return rows, np.array(off, np.int32), (np.concatenate(out) if out else np.zeros(0, np.uint64))

    def stat(t):
        t = np.array(t) * 1e3
        return dict(median_ms=round(float(np.median(t)), 4), p10_ms=round(float(np.percentile(t, 10)), 4), p90_ms=round(float(np.percentile(t, 90)), 4))
    res = dict(entries=N, features=F, vocabulary=VOCAB, words_per_bow=[int(min(words)), int(np.median(words)), int(max(words))], repeats=a.repeats, submaps={})
    next_id = 10 ** 7
    for k in sizes:
        slots = np.arange(k, dtype=np.int32); entries = (N + slots).astype(np.int32)
        t_new, t_old, same, n_rows, n_kept = [], [], True, 0, 0
        for rep in range(a.repeats + 3):
            ids = (next_id + np.arange(k)).astype(np.uint64); next_id += k
            t0 = time.perf_counter()
            rows, off, mids = corb.map_fusion_candidates(dbs[0], sub, slots, entries, ids, glob, entry_slot, cap_rows=k * 64, cap_ids=k * 32 * F)
            t1 = time.perf_counter()
            e_rows, e_off, e_ids = earlier(dbs[1], slots, entries, ids)
            t2 = time.perf_counter()
            got = np.stack([rows[n].astype(np.int64) for n in corb.FUSION_ROW_DTYPE.names], axis=1) if len(rows) else np.zeros((0, 6), np.int64)
            same = same and np.array_equal(got, np.array(e_rows, np.int64).reshape(-1, 6)) and np.array_equal(off, e_off) and mids.tobytes() == e_ids.tobytes()
            if rep >= 3:
                t_new.append(t1 - t0); t_old.append(t2 - t1)
            n_rows, n_kept = len(rows), int(rows["kept"].sum())
        same = same and dbs[0].state().tobytes() == dbs[1].state().tobytes()
        res["submaps"][str(k)] = dict(rows=n_rows, kept=n_kept, one_call=stat(t_new), single_calls=stat(t_old), same_bytes=bool(same))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as o:
        json.dump(res, o, indent=1); o.write("\n")
    print(json.dumps(res))
    assert all(s["same_bytes"] for s in res["submaps"].values()), "the one call and the single calls disagree"
    for h in dbs + [glob, sub, voc]:
        h.close()


if __name__ == "__main__":
    main()

"""Host-to-host time of LoopClosing::DetectLoop on records (include/corb_loop_detect.h): corb_loop_detect_queue for a queue of 1 and of 8 keyframes on a map of 300
keyframes of 2 000 features (BowVectors from the 10^4-word vocabulary k10L4 by corb_kf_store_compute_bow), 20 covisible keyframes each, the last 50 keyframes
revisiting the places of the first 50; the median of the calls with the 10th and 90th percentile.

Beside it stands the route a host walks without the call, in the same process, on the same data and alternating with it: corb_covis_query, corb_kfdb_score with the
minimum taken on the host, corb_kfdb_detect(kind 0) with the connected set uploaded, one corb_covis_get per candidate, corb_kfdb_add, the group logic in Python.  The two
routes run on twin databases and must leave the same answers and the same bytes in the database's six fields; the tool fails if they do not.  After every repeat both
are put back: the queued keyframes erased, the groups cleared, and a query under another id run so that the next repeat pushes every entry again (a repeated id pushes
nothing).  No ratio is fixed.  Kernel times are not measured.  Results: profiles/loopdetect_rate.json and one JSON line.
      python tools/loopdetect_rate.py [--keyframes 300] [--features 2000] [--repeats 30]"""
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
import loopdetect_reference as R                                           # noqa: E402

VOCAB, PER_PLACE, HALF, WEIGHT, TH, BATCH, ID0 = "k10L4", 10, 10, 15, 15, 50, 100


def flipped(rng, desc, bits):
    """desc with `bits` random bit positions per row flipped"""
    out = desc.copy()
    pos = rng.integers(0, 256, (len(desc), bits))
    for k in range(bits):
        out[np.arange(len(desc)), pos[:, k] >> 3] ^= (1 << (pos[:, k] & 7)).astype(np.uint8)
    return out


def stats(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4), calls=len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=300); ap.add_argument("--features", type=int, default=2000); ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--queues", default="1,8"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loopdetect_rate.json"))
    a = ap.parse_args()
    corb = corbload.load_pkg()
    v = G.vocab(VOCAB); f = v.flat()
    voc = corb.Vocabulary(f["k"], f["L"], f["parent"], f["is_leaf"], f["descriptor"], f["weight"])
    rng = np.random.default_rng(1)
    N, F = a.keyframes, a.features
    n_new = 50; n_old = N - n_new
    queues = [int(q) for q in a.queues.split(",")]
    leaves = v.descriptor[v.words]
    n_places = (n_old + PER_PLACE - 1) // PER_PLACE
    scenes = [flipped(rng, leaves[rng.integers(0, len(leaves), F)], 30) for _ in range(n_places)]
    place = [k // PER_PLACE if k < n_old else (k - n_old) // PER_PLACE for k in range(N)]          # the last 50 keyframes are back where the first 50 were

    # covisibility from map points alone: keyframe k shares WEIGHT points with each of k +- 1 .. HALF (20 covisible keyframes inside the chain)
    KF = corb.KeyFrameStore(N, F)
    mp_of = np.full((N, F), corb.NO_MAP_POINT, np.uint64); used = np.zeros(N, np.int64)
    obs_kf, obs_idx, ids = [], [], []
    for k in range(N):
        for d in range(1, HALF + 1):
            if k + d < N:
                for _ in range(WEIGHT):
                    pid = 10 ** 6 + len(ids); ids.append(pid)
                    obs_kf += [ID0 + k, ID0 + k + d]; obs_idx += [used[k], used[k + d]]
                    mp_of[k, used[k]] = pid; mp_of[k + d, used[k + d]] = pid; used[k] += 1; used[k + d] += 1
    for b0 in range(0, N, BATCH):
        n = min(BATCH, N - b0)
        meta = np.zeros(n, corb.KF_META_DTYPE); meta["id"] = ID0 + b0 + np.arange(n); meta["nlevels"] = 8
        desc = np.concatenate([flipped(rng, scenes[place[b0 + k]], 8) for k in range(n)])
        KF.put_batch(b0, meta, (np.arange(n + 1) * F).astype(np.int32), np.zeros(n * F, corb.KP_DTYPE), desc, mp_id=mp_of[b0:b0 + n].reshape(-1))
    MP = corb.MapPointStore(len(ids), 4)
    rec = np.zeros(len(ids), corb.MP_RECORD_DTYPE); rec["id"] = ids; rec["n_obs"] = 2; rec["ref_kf_id"] = corb.NO_ID
    MP.put(0, rec, (2 * np.arange(len(ids) + 1)).astype(np.int32), np.array(obs_kf, np.uint64), np.array(obs_idx, np.uint32)); MP.build_index(0, len(ids))
    g = corb.Covisibility(KF, MP, 64)
    g.UpdateConnections(np.arange(N), th=TH)
    n_cov = [len(g.query(k)[0]) for k in (0, N // 2, N - 1)]

    dbs = [corb.KeyFrameDatabase(voc, N, F) for _ in range(2)]
    for db in dbs:                                                         # entry k is keyframe k's BowVector
        for b0 in range(0, N, BATCH):
            s = np.arange(b0, min(b0 + BATCH, N)); KF.compute_bow(s, voc, 4, db, s)
        for k in range(N):
            nb = [int(x) for x in g.query(k, N=10)[0]]
            db.set_neighbours(k, nb + [-1] * (10 - len(nb)))
        for k in range(n_old):
            db.add(k)
    det = corb.LoopDetector(g, dbs[0], 64, 128); det.bind(np.arange(N), np.arange(N))
    slot_of_id = {ID0 + k: k for k in range(N)}

    def host_route(db, slots, groups):
        """the five calls per keyframe and the definition's closed form; [(outcome, minScore bits, candidates)]"""
        out = []
        for s in slots:
            cov = g.query(s)[0]
            ms = np.float32(1)
            for x in db.score(s, cov):
                if np.float32(x) < ms:
                    ms = np.float32(x)
            conn = [slot_of_id[int(i)] for i in g.get(s)[0][0] if int(i) in slot_of_id]
            cands = [int(c) for c in db.detect(0, s, ID0 + s, conn, float(ms))]
            if not cands:
                db.add(s); groups[:] = []
                out.append((R.NONE, int(ms.view(np.uint32)), cands)); continue
            cg = [set(slot_of_id[int(i)] for i in g.get(c)[0][0] if int(i) in slot_of_id) | {c} for c in cands]
            new, enough = R.closed_form(cg, groups); groups[:] = new
            db.add(s)
            out.append((R.DETECTED if enough else R.NOT_ENOUGH, int(ms.view(np.uint32)), cands))
            if enough:
                break
        return out

    result = dict(config="%d keyframes of %d features, vocabulary %s, %d / %d / %d covisible keyframes at the ends and the middle, %d keyframes in the database, max_connections 64"
                  % (N, F, VOCAB, n_cov[0], n_cov[1], n_cov[2], n_old), timing="host to host; routes alternate call by call; kernel times not measured", queues={})
    for Q in queues:
        t_dev, t_host, n_cand, equal = [], [], 0, True
        for r in range(a.repeats + 3):
            first = n_old + (r * Q) % (n_new - Q + 1)
            slots = list(range(first, first + Q))
            t0 = time.perf_counter(); got = det.detect_queue(slots); t1 = time.perf_counter()
            groups = []
            t2 = time.perf_counter(); want = host_route(dbs[1], slots, groups); t3 = time.perf_counter()
            same = [(x["outcome"], x["min_score_bits"], x["cand_entries"]) for x in got] == want and dbs[0].state().tobytes() == dbs[1].state().tobytes() and \
                [(sorted(m), c) for m, c in det.get_groups()] == [(sorted(m), c) for m, c in groups]
            equal = equal and same
            n_cand += sum(len(x["cand_entries"]) for x in got)
            for db in dbs:                                                 # put both back
                for s in slots[:len(got)]:
                    db.erase(s)
                for s in slots:
                    db.detect(0, s, 7, [], 0.0)
            det.clear_groups()
            if r >= 3:
                t_dev.append((t1 - t0) * 1e3); t_host.append((t3 - t2) * 1e3)
        if not equal:
            raise SystemExit("loopdetect_rate: the two routes differ for a queue of %d" % Q)
        result["queues"][str(Q)] = dict(corb_loop_detect_queue=stats(t_dev), five_call_host_route=stats(t_host), candidates_per_call=round(n_cand / (a.repeats + 3), 2),
                                        routes_give_equal_bytes=True)
    result["note"] = "five_call_host_route drives the C calls from Python with the group logic in Python: its share of interpreter time is not separated"
    with open(a.out, "w") as fh:
        json.dump(result, fh); fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

"""Host-to-host time per call of keyframe insertion on records (include/corb_keyframe_insert.h) on a KITTI-shaped keyframe: 2000 features, about 1500 with depth, a
map of 2000 points of which the frame tracks about 400.  Calls 1 (corb_kfi_create_stereo_points), 3 (corb_kfi_process_new_keyframe) and 4
(corb_kfi_map_point_culling), each with apply != 0; every call ends in a synchronise and a read-back, so a host clock around it is the call's time.

Beside call 1 stands the route a record-resident client had to take for the same step through the existing C-ABI, in the same process and alternating with it:
fetch the record's features and ids (corb_kf_store_get, corb_kf_store_get_map_points), sort the depths on the host, build the records on the host (vectorised numpy:
unprojection, normal, distances, descriptor copy), corb_mp_store_put_host (+ counters and scratch), corb_kf_store_set_map_points (+ flags).  Both routes leave the same
ids in the keyframe record (checked); the host route's float fields are numpy's, compared within a tolerance.  Between repeats the records are put back as they were
and the index is rebuilt, outside the timed windows of both routes.  No ratio is fixed; the numbers go to profiles/kfinsert_rate.json and are printed as one JSON line.
      python tools/kfinsert_rate.py [--features 2000] [--repeats 30]"""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import corbload                                                            # noqa: E402
import kfinsert_cases as G                                                 # noqa: E402
import kfinsert_reference as R                                             # noqa: E402
from kfinsert_stores import to_stores, mp_arrays                           # noqa: E402

TH_DEPTH, N_OLD, KF_ID = 35.0, 2000, 40


def scene(n, seed):
    rng = np.random.default_rng(seed)
    depth = np.where(rng.random(n) < 0.75, rng.uniform(3, 80, n), -1).astype(np.float32)
    kfs = [G.keyframe(rng, 10 + 6 * s, n) for s in range(5)] + [G.keyframe(rng, KF_ID, n, depth)]
    new = kfs[5]
    olds = []
    for q in range(N_OLD):
        ids = rng.permutation([10, 16, 22, 28, 34])[: int(rng.integers(1, 5))]
        olds.append(G.point(rng, 500 + q, [(int(k), int(rng.integers(0, n))) for k in ids], found=int(rng.integers(1, 6)), visible=5, first_kf=KF_ID - int(rng.integers(0, 5))))
    tracked = rng.permutation(n)[: n // 5]
    new["mp_id"][tracked] = 500 + rng.permutation(N_OLD)[: len(tracked)]; new["flags"][tracked] = R.HAS_MP
    sc = dict(kfs=kfs, mps=olds + [None] * (n + 8), cam=G.CAM, F=max(n, 64), O=8, index={})
    R.build_index(sc, 0, N_OLD)
    return sc


def host_route(corb, KF, MP, slot, n_obs_of, cam, first_slot, first_id, frame_id):
    """the parent commit's route for the step of call 1"""
    g = KF.get(slot); ids = KF.get_map_points(slot); meta = KF.get_meta(slot)                   # 1: fetch
    z = g["depth"]; cand = np.flatnonzero(z > 0)
    order = cand[np.lexsort((cand, z[cand]))]                                                    # 2: sort (z, i)
    near = int((~(z[order] > np.float32(TH_DEPTH))).sum()); J = max(100, near)
    order = order[: J + 1 if J < len(order) else len(order)]
    held = ids[order]
    create = (held == corb.NO_MAP_POINT) | np.array([n_obs_of.get(int(h), 1) < 1 for h in held])
    idx = order[create]; k = len(idx)
    T = meta["Tcw"].reshape(4, 4).astype(np.float64); Rwc = T[:3, :3].T; Ow = -Rwc @ T[:3, 3]     # 3: records
    zc = z[idx].astype(np.float64)
    Xc = np.stack([(g["kp"]["x"][idx] - cam["cx"]) * zc / cam["fx"], (g["kp"]["y"][idx] - cam["cy"]) * zc / cam["fy"], zc], 1)
    X = (Xc @ Rwc.T + Ow).astype(np.float32)
    v = X.astype(np.float64) - Ow; dist = np.linalg.norm(v, axis=1)
    rec = np.zeros(k, corb.MP_RECORD_DTYPE)
    rec["id"] = first_id + np.arange(k); rec["ref_kf_id"] = meta["id"]; rec["descriptor"] = g["desc"][idx]; rec["client_id"] = 1; rec["n_obs"] = 1; rec["world_pos"] = X
    rec["normal"] = (v / dist[:, None]).astype(np.float32)
    level = np.clip(g["kp"]["octave"][idx], 0, 7)
    rec["max_distance"] = (dist * cam["scale"][level]).astype(np.float32); rec["min_distance"] = rec["max_distance"] / cam["scale"][7]
    scr = np.zeros(k, corb.MP_SCRATCH_DTYPE); scr["first_kf_id"] = meta["id"]; scr["first_frame"] = frame_id; scr["n_obs_weight"] = np.where(g["u_right"][idx] >= 0, 2, 1)
    MP.put(first_slot, rec, np.arange(k + 1, dtype=np.int32), np.full(k, meta["id"], np.uint64), idx.astype(np.uint32))      # 4: upload
    MP.set_counters(first_slot, np.ones(k, np.int32), np.ones(k, np.int32)); MP.set_scratch(first_slot, scr)
    ids = ids.copy(); ids[idx] = rec["id"]; fl = g["flags"].copy(); fl[idx] |= 1
    KF.set_map_points(slot, ids); KF.set_flags(slot, fl)                                         # 5: the keyframe's ids
    return order, X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=2000); ap.add_argument("--repeats", type=int, default=30); ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfinsert_rate.json"))
    a = ap.parse_args()
    corb = corbload.load_pkg()
    if corb.device_count() < 1:
        raise SystemExit("kfinsert_rate: no MI355X visible; a time needs the device")
    sc = scene(a.features, a.seed); n = a.features
    KF, MP = to_stores(corb, sc)
    cam = corb.TrackCamera.make(G.CAM["fx"], G.CAM["fy"], G.CAM["cx"], G.CAM["cy"], G.CAM["bf"], G.CAM["mb"], 0.0, 1241.0, 0.0, 376.0, G.CAM["scale"])
    h = corb.KeyframeInserter(sc["F"], 2 * n)
    rec, okf, oi, cnt, scr = mp_arrays(corb, sc)
    lens = rec["n_obs"][:N_OLD]; off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    flat_kf = np.concatenate([okf[s, : lens[s]] for s in range(N_OLD)]); flat_i = np.concatenate([oi[s, : lens[s]] for s in range(N_OLD)])
    ids0, flags0 = sc["kfs"][5]["mp_id"].copy(), sc["kfs"][5]["flags"].copy()
    n_obs_of = {int(p["id"]): len(p["obs"]) for p in sc["mps"][:N_OLD]}

    def restore():
        MP.put(0, rec[:N_OLD], off, flat_kf, flat_i); MP.set_counters(0, cnt["n_visible"][:N_OLD], cnt["n_found"][:N_OLD]); MP.set_scratch(0, scr[:N_OLD])
        KF.set_map_points(5, ids0); KF.set_flags(5, flags0); MP.build_index(0, N_OLD)

    t = dict(call1=[], host_route=[], call3=[], call4=[])
    check = {}
    for rep in range(a.repeats + 3):                                        # three warm-up rounds: code objects, the handle's tables at their final size
        restore()
        t0 = time.perf_counter()
        out = h.CreateStereoPoints(KF, 5, MP, cam, TH_DEPTH, 1, apply=True, first_mp_slot=N_OLD, first_mp_id=70000, client_id=1, frame_id=9)
        t1 = time.perf_counter()
        ids_dev = KF.get_map_points(5)
        MP.build_index(0, N_OLD + out["n_created"])
        t2 = time.perf_counter()
        a3 = h.ProcessNewKeyFrame(KF, 5, MP, 0, 6, 1.2, apply=True)
        t3 = time.perf_counter()
        recent = np.concatenate([np.arange(0, N_OLD, 4, dtype=np.int32), a3["recent_slots"]])
        t4 = time.perf_counter()
        a4 = h.MapPointCulling(MP, recent, KF_ID + 2, 3, KF, 0, 6, apply=True)
        t5 = time.perf_counter()
        restore()
        t6 = time.perf_counter()
        order, X = host_route(corb, KF, MP, 5, n_obs_of, G.CAM, N_OLD, 70000, 9)
        t7 = time.perf_counter()
        ids_host = KF.get_map_points(5)
        if rep >= 3:
            t["call1"].append(t1 - t0); t["call3"].append(t3 - t2); t["call4"].append(t5 - t4); t["host_route"].append(t7 - t6)
        check = dict(n_visited=out["n_visited"], n_created=out["n_created"], n_added=a3["n_added"], n_recent=len(a3["recent_slots"]), list_length=len(recent), n_culled=a4["n_culled"],
                     same_order=bool(np.array_equal(order, out["order"])), same_ids=bool(np.array_equal(ids_dev, ids_host)),
                     x3d_max_abs_diff=float(np.abs(X - out["x3d"]).max()) if len(X) == len(out["x3d"]) and len(X) else None)

    def stat(v):
        v = np.array(v) * 1e3
        return dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4), p10_ms=round(float(np.percentile(v, 10)), 4),
                    p90_ms=round(float(np.percentile(v, 90)), 4))
    res = dict(features=n, with_depth=int((sc["kfs"][5]["depth"] > 0).sum()), map_points=N_OLD, repeats=a.repeats, th_depth=TH_DEPTH,
               call1_create_stereo_points=stat(t["call1"]), call1_host_route=stat(t["host_route"]), call3_process_new_keyframe=stat(t["call3"]),
               call4_map_point_culling=stat(t["call4"]), check=check)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as o:
        json.dump(res, o, indent=1); o.write("\n")
    print(json.dumps(res))
    assert check["same_order"] and check["same_ids"], "the host route and the device call disagree"
    h.close(); KF.close(); MP.close()


if __name__ == "__main__":
    main()

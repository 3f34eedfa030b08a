"""Tracking::TrackLocalMap on records, one GPU: the one call (corb_track_local_map) beside the route it replaces, on the map of tools/localmap_rate.py.

The map: one client's synth.ba_problem_fast map -- about 2000 features per keyframe, 300 keyframes, every point seen by 3..8 keyframes next to each other in time.
The frame is a copy of a keyframe's record in a store of its own (it holds that keyframe's points); the normals point from its camera centre to the points, so its
neighbourhood is in view.  All descriptors of this map are zero: every point in view matches.

Three routes, alternating call by call in the same process; every call ends in a synchronise, so the host clock around it is the call's time (no kernel times are
taken here).  Before every call, untimed, the frame's record (ids, flags, pose) and the map's counters are put back.
  one_call          : KeyFrameStore.TrackLocalMap
  three_calls       : TrackUpdateLocalMap + TrackSearchLocalPoints + TrackPoseOptimization -- the bar: it leaves mnVisible / mnFound untouched
  three_calls_upkeep: the same plus what makes it equivalent: TRACKED read back, get_counters over the touched slots, the sums on the host, set_counters,
                      and the stereo outliers' ids taken out of the frame
Before timing, one_call and three_calls_upkeep must leave equal counters, frame ids and matches.  Each is run at the wrapper's default caps (128, 16384) and at
exact caps.  Prints one JSON line (and writes it to --out), times in ms as median [p10, p90] over --calls calls after --warmup.
usage: python tools/tracklocal_rate.py [--kf 300] [--ppk 360] [--calls 200] [--warmup 20] [--out profiles/tracklocal_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import corbload  # noqa: E402

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
FRAME_ID = 900000008


def stats(ts, calls):
    ts = np.sort(np.array(ts)) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(ts[int(0.1 * len(ts))]), 4), p90_ms=round(float(ts[int(0.9 * len(ts))]), 4), calls=calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=300)
    ap.add_argument("--ppk", type=int, default=360, help="new points per keyframe; a point is seen by ~5.5 keyframes")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracklocal_rate.json"))
    a = ap.parse_args()
    corb = corbload.load_pkg()
    from corb_slam_amd import synth
    prob = synth.ba_problem_fast(n_clients=1, kf_per_client=a.kf, pts_per_kf=a.ppk, seed=1000, obs_range=(3, 8), window=6)
    arr = synth.map_arrays(prob, a.kf, a.ppk)
    K, n_mp = len(arr["meta"]), len(arr["mp_records"])
    feats = np.diff(arr["feat_off"]); off = arr["feat_off"]
    out = dict(config="one client, %d keyframes, %d map points, features per keyframe median %d / max %d, observations per point max %d"
               % (K, n_mp, int(np.median(feats)), int(feats.max()), arr["max_obs"]),
               timing="host to host, every call ends in a synchronise; routes alternate call by call; kernel times not measured")
    if corb.device_count() < 1:
        raise SystemExit("no MI355X visible")
    cur = int(np.linspace(0, K - 1, 16).astype(int)[8])
    T = arr["meta"]["Tcw"][cur].reshape(4, 4).astype(np.float32); Ow = -T[:3, :3].T @ T[:3, 3]
    PO = arr["mp_records"]["world_pos"] - Ow; arr["mp_records"]["normal"] = (PO / np.maximum(np.linalg.norm(PO, axis=1), 1e-6)[:, None]).astype(np.float32)
    KF = corb.KeyFrameStore(K, arr["max_features"]); MP = corb.MapPointStore(n_mp, arr["max_obs"]); FR = corb.KeyFrameStore(1, arr["max_features"])
    KF.put_batch(0, arr["meta"], off, arr["kp"], None, arr["ur"], None, arr["mp_id"])
    MP.put(0, arr["mp_records"], arr["obs_off"], arr["obs_kf"], arr["obs_idx"]); MP.build_index(0, n_mp)
    meta = arr["meta"][cur: cur + 1].copy(); meta["id"] = FRAME_ID
    sl = slice(off[cur], off[cur + 1]); n = int(off[cur + 1] - off[cur])
    FR.put_batch(0, meta, np.array([0, n], np.int32), arr["kp"][sl], None, arr["ur"][sl], None, arr["mp_id"][sl])
    g = corb.Covisibility(KF, MP)
    g.UpdateConnections(np.arange(K, dtype=np.int32))
    m0 = arr["meta"][cur]
    cam = corb.TrackCamera.make(float(m0["fx"]), float(m0["fy"]), float(m0["cx"]), float(m0["cy"]), float(m0["bf"]), float(m0["bf"]) / float(m0["fx"]),
                                0.0, 2.0 * float(m0["cx"]), 0.0, 2.0 * float(m0["cy"]), (1.2 ** np.arange(8)).astype(np.float32))
    logs = float(np.float32(np.log(np.float32(1.2))))
    ids0 = np.array(arr["mp_id"][sl], np.uint64); flags0 = np.zeros(n, np.uint8)
    slot_of = {int(i): s for s, i in enumerate(arr["mp_records"]["id"])}
    zeros = np.zeros(n_mp, np.int32)

    def reset():
        FR.set_map_points(0, ids0); FR.set_flags(0, flags0); FR.set_meta_raw(0, meta[0]); MP.set_counters(0, zeros, zeros)

    def one_call(caps):
        return FR.TrackLocalMap(0, g, cam, T, FRAME_ID, logs, sensor=1, **caps)

    def three_calls(caps, upkeep):
        ks, ms, mids, info = FR.TrackUpdateLocalMap(0, g, (), **caps)
        res = FR.TrackSearchLocalPoints(0, MP, mids, cam, T, logs, th=1.0, want_tracked=upkeep)
        Tn, outl, inl = FR.TrackPoseOptimization(0, MP, cam, T, discard_outliers=False)
        if not upkeep:
            return res[0], None
        match, tracked = res[0], res[3]
        held = FR.get_map_points(0)
        own = np.array([slot_of.get(int(i), -1) for i in ids0], np.int64)                      # the frame's own points before the search: seen, visible + 1 each
        now = np.array([slot_of.get(int(i), -1) for i in held], np.int64)
        touched = np.concatenate([own[own >= 0], ms.astype(np.int64), now[now >= 0]])
        lo, hi = int(touched.min()), int(touched.max())
        c = MP.get_counters(lo, hi - lo + 1)
        np.add.at(c["n_visible"], own[own >= 0] - lo, 1)
        np.add.at(c["n_visible"], ms[tracked["valid"] != 0].astype(np.int64) - lo, 1)
        np.add.at(c["n_found"], now[(now >= 0) & ~outl] - lo, 1)
        MP.set_counters(lo, c["n_visible"], c["n_found"], c["replaced_by"])
        if outl.any():
            held[outl] = NONE; FR.set_map_points(0, held)
        return match, int(((now >= 0) & ~outl).sum())

    try:
        reset(); first = one_call({})
    except corb.CorbError as e:
        out["error"] = str(e)
        print(json.dumps(out)); return
    exact = dict(kf_cap=int(first["local"].n_kf), mp_cap=int(first["local"].n_mp))
    out["local_map"] = dict(n_kf=exact["kf_cap"], n_points=exact["mp_cap"], features=n, in_view=int(first["n_in_view"]), matches=int(first["n_matches"]),
                            pose_inliers=int(first["n_pose_inliers"]), matches_inliers=int(first["n_matches_inliers"]))
    # both routes leave equal bytes (the map has no bad point and every point has observations: the inliers are the held, non-outlier features)
    c_new = MP.get_counters(0, n_mp).tobytes(); ids_new = FR.get_map_points(0).tobytes()
    reset(); match_old, inl_old = three_calls({}, True)
    assert MP.get_counters(0, n_mp).tobytes() == c_new and FR.get_map_points(0).tobytes() == ids_new, "the two routes leave different counters or frame ids"
    assert np.array_equal(match_old, first["match"]) and inl_old == first["n_matches_inliers"], "the two routes match differently"
    out["routes_leave_equal_bytes"] = True
    for name, caps in (("default_caps", {}), ("exact_caps", exact)):
        ts = dict(one_call=[], three_calls=[], three_calls_upkeep=[])
        for i in range(a.warmup + a.calls):
            for route, fn in (("one_call", lambda: one_call(caps)), ("three_calls", lambda: three_calls(caps, False)), ("three_calls_upkeep", lambda: three_calls(caps, True))):
                reset()
                t0 = time.perf_counter(); fn(); t = time.perf_counter() - t0
                if i >= a.warmup:
                    ts[route].append(t)
        out[name] = dict(caps=dict(kf_cap=caps.get("kf_cap", 128), mp_cap=caps.get("mp_cap", 16384)), **{k: stats(v, a.calls) for k, v in ts.items()})
        out[name]["one_call_not_slower_than_three_calls"] = out[name]["one_call"]["median_ms"] <= out[name]["three_calls"]["median_ms"]
    g.close(); KF.close(); MP.close(); FR.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

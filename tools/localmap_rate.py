"""Tracking::UpdateLocalMap and the spanning tree on one GPU (corb_track_update_local_map, corb_covis_reparent_children): what a tracked frame and a culled keyframe
pay, beside the calls next to them in TrackLocalMap / LocalMapping.

The map is tools/covis_rate.py's: one client's synth.ba_problem_fast map of the configs[2] shape -- about 2000 features per keyframe, a few hundred keyframes, every
point seen by 3..8 keyframes next to each other in time.  The current frame is a copy of a keyframe's record in a store of its own (it holds that keyframe's points).
Every call is synchronous, so the host clock around it is the call's time.  Prints one JSON line, times in ms as median [p10, p90] over --calls calls after --warmup:
  update_local_map     : corb_track_update_local_map with the wrapper's default caps (kf_cap = 128, mp_cap = 16384)
  update_local_map_big : the same with kf_cap = max_connections = 512 and mp_cap = 65536 (the points pass's launch and the read-back follow the caps)
  reparent_children    : corb_covis_reparent_children of one keyframe; its tree and its children's are put back before every call (untimed), its row is NOT erased
  update_1             : corb_covis_update of one keyframe, tree upkeep included (tools/covis_rate.py's figure of the same name)
  local_window         : corb_covis_local_window of one keyframe
  search_local_points  : corb_track_search_local_points of the frame against the local points the update returned (all descriptors of this map are zero: every
                         point in view matches)
usage: python tools/localmap_rate.py [--kf 300] [--ppk 360] [--calls 200] [--warmup 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import corbload  # noqa: E402


def timed(fn, args_list, warmup, calls, before=None):
    ts = []
    for i in range(warmup + calls):
        args = args_list[i % len(args_list)]
        if before:
            before(*args)
        t0 = time.perf_counter(); fn(*args); t = time.perf_counter() - t0
        if i >= warmup:
            ts.append(t)
    ts = np.sort(np.array(ts)) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(ts[int(0.1 * len(ts))]), 4), p90_ms=round(float(ts[int(0.9 * len(ts))]), 4), calls=calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=300)
    ap.add_argument("--ppk", type=int, default=360, help="new points per keyframe; a point is seen by ~5.5 keyframes")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    corb = corbload.load_pkg()
    from corb_slam_amd import synth
    prob = synth.ba_problem_fast(n_clients=1, kf_per_client=a.kf, pts_per_kf=a.ppk, seed=1000, obs_range=(3, 8), window=6)
    arr = synth.map_arrays(prob, a.kf, a.ppk)
    K, n_mp = len(arr["meta"]), len(arr["mp_records"])
    feats = np.diff(arr["feat_off"]); off = arr["feat_off"]
    out = dict(config="one client, %d keyframes, %d map points, features per keyframe median %d / max %d, observations per point max %d"
               % (K, n_mp, int(np.median(feats)), int(feats.max()), arr["max_obs"]))
    if corb.device_count() < 1:
        raise SystemExit("no MI355X visible")
    some = [int(s) for s in np.linspace(0, K - 1, 16).astype(int)]
    cur = some[8]
    # normals that let the frame's keyframe see its neighbourhood: from its camera centre to the point
    T = arr["meta"]["Tcw"][cur].reshape(4, 4).astype(np.float32); Ow = -T[:3, :3].T @ T[:3, 3]
    PO = arr["mp_records"]["world_pos"] - Ow; arr["mp_records"]["normal"] = (PO / np.maximum(np.linalg.norm(PO, axis=1), 1e-6)[:, None]).astype(np.float32)
    KF = corb.KeyFrameStore(K, arr["max_features"]); MP = corb.MapPointStore(n_mp, arr["max_obs"]); FR = corb.KeyFrameStore(len(some), arr["max_features"])
    KF.put_batch(0, arr["meta"], off, arr["kp"], None, arr["ur"], None, arr["mp_id"])
    MP.put(0, arr["mp_records"], arr["obs_off"], arr["obs_kf"], arr["obs_idx"]); MP.build_index(0, n_mp)
    for j, s in enumerate(some):                                 # the frames: copies of 16 keyframes, each with an id of its own
        meta = arr["meta"][s: s + 1].copy(); meta["id"] = 900000000 + j
        sl = slice(off[s], off[s + 1])
        FR.put_batch(j, meta, np.array([0, off[s + 1] - off[s]], np.int32), arr["kp"][sl], None, arr["ur"][sl], None, arr["mp_id"][sl])
    g = corb.Covisibility(KF, MP)
    slots = np.arange(K, dtype=np.int32)
    g.UpdateConnections(slots)                                   # the graph and the tree of the whole map
    ks, ms, ids, info = FR.TrackUpdateLocalMap(8, g, [])
    out["local_map_of_slot_%d" % cur] = dict(n_kf=int(info.n_kf), n_voted=int(info.n_voted), n_points=int(info.n_mp), ref_slot=int(info.ref_slot))
    frames = [(j,) for j in range(len(some))]
    out["update_local_map"] = timed(lambda j: FR.TrackUpdateLocalMap(j, g, ks), frames, a.warmup, a.calls)
    out["update_local_map_big"] = timed(lambda j: FR.TrackUpdateLocalMap(j, g, ks, kf_cap=512, mp_cap=65536), frames, a.warmup, a.calls)
    trees = {s: g.GetTree(s) for s in range(K)}
    n_children = [len(trees[s][2]) for s in range(K)]
    with_children = [s for s in np.argsort(n_children)[::-1][:16] if n_children[s] > 0]
    slot_of = {int(i): s for s, i in enumerate(arr["meta"]["id"])}

    def restore(s):
        for x in [s] + [slot_of[int(c)] for c in trees[s][2]] + ([slot_of[trees[s][0]]] if trees[s][0] in slot_of else []):
            g.SetTree(x, *trees[x])
    out["reparent_children"] = timed(lambda s: g.ReparentChildren(s), [(int(s),) for s in with_children], a.warmup, a.calls, before=restore)
    out["reparent_children"]["children_median"] = int(np.median([n_children[s] for s in with_children]))
    for s in range(K):
        g.SetTree(s, *trees[s])
    out["update_1"] = timed(lambda s: g.UpdateConnections([s]), [(s,) for s in some], a.warmup, a.calls)
    out["local_window"] = timed(lambda s: g.LocalWindow(s, 256, 65536), [(s,) for s in some], a.warmup, a.calls)
    m = arr["meta"][cur]
    cam = corb.TrackCamera.make(float(m["fx"]), float(m["fy"]), float(m["cx"]), float(m["cy"]), float(m["bf"]), float(m["bf"]) / float(m["fx"]),
                                0.0, 2.0 * float(m["cx"]), 0.0, 2.0 * float(m["cy"]), (1.2 ** np.arange(8)).astype(np.float32))
    logs = float(np.float32(np.log(np.float32(1.2))))
    try:
        res = FR.TrackSearchLocalPoints(8, MP, ids, cam, T, logs)
        out["search_local_points"] = timed(lambda: FR.TrackSearchLocalPoints(8, MP, ids, cam, T, logs, want_match=False), [()], a.warmup, a.calls)
        out["search_local_points"].update(n_local=int(len(ids)), first_call_matches=int(res[1]), first_call_in_view=int(res[2]))
    except corb.CorbError as e:
        out["search_local_points"] = dict(error=str(e))
    g.close(); KF.close(); MP.close(); FR.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

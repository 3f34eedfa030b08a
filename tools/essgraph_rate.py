"""Optimizer::OptimizeEssentialGraph on records (corb_essential_graph_store, include/corb_essential_graph.h) beside the route through the earlier C-ABI, in the same
process on the same map: one client's synth.ba_problem_fast map put into the stores by synth.map_arrays, every keyframe connected, CorrectLoop's propagation run
for the newest keyframe, LoopConnections = {newest: {oldest}}.  Before every timed call the records are put back to that state (not timed).

  records     Covisibility.OptimizeEssentialGraph: plan, solve and commit in one call
  earlier     fetch (every header, row, tree entry and loop-edge set, every map-point record and its scratch), host flatten (tests/essgraph_reference.plan, plain
              Python: the definition, not a tuned flattener -- its time is reported on its own), corb_optimize_essential_graph on the arrays, then the write-back:
              set_meta per moved keyframe, corb_mp_store_put_host of every point, the scratch and the index again
The solve is the same kernels on both routes; set-up and write-back differ.  Both routes must leave the same poses and positions (checked, bit for bit).
Prints one JSON line and writes it to profiles/essgraph_rate.json: per call host to host, median of --calls with the 10th and 90th percentiles, in ms.
usage: python tools/essgraph_rate.py [--kf 120] [--ppk 120] [--calls 30] [--min-weight 30]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import corbload  # noqa: E402


def stats(ts):
    ts = np.sort(np.array(ts)) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(ts[int(0.1 * len(ts))]), 4), p90_ms=round(float(ts[int(0.9 * len(ts))]), 4), calls=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=120)
    ap.add_argument("--ppk", type=int, default=120)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--min-weight", type=int, default=30)
    a = ap.parse_args()
    corb = corbload.load_pkg()
    from corb_slam_amd import synth
    import covis_reference as R
    import essgraph_reference as ER
    import localmap_reference as LR
    if corb.device_count() < 1:
        raise SystemExit("no MI355X visible")
    prob = synth.ba_problem_fast(n_clients=1, kf_per_client=a.kf, pts_per_kf=a.ppk, seed=1000, obs_range=(3, 8), window=6)
    arr = synth.map_arrays(prob, a.kf, a.ppk)
    K, n_mp = len(arr["meta"]), len(arr["mp_records"])
    KF = corb.KeyFrameStore(K, arr["max_features"]); MP = corb.MapPointStore(n_mp, arr["max_obs"])
    KF.put_batch(0, arr["meta"], arr["feat_off"], arr["kp"], None, arr["ur"], None, arr["mp_id"])
    MP.put(0, arr["mp_records"], arr["obs_off"], arr["obs_kf"], arr["obs_idx"]); MP.build_index(0, n_mp)
    g = corb.Covisibility(KF, MP)
    g.UpdateConnections(np.arange(K, dtype=np.int32))
    cur, loop = K - 1, 0
    T = KF.get_meta(cur)["Tcw"].reshape(4, 4).astype(np.float64)
    import loopfix_reference as XR
    Scw = np.concatenate([XR.quat_from_R(T[:3, :3]), T[:3, 3] + [0.05, -0.02, 0.03], [1.0]])
    ks, co, nc, _ = g.CorrectLoop(cur, Scw, 1.2)
    lc = [(cur, [loop])]
    meta0 = [KF.get_meta(s) for s in range(K)]; rec0 = MP.get(0, n_mp)[0]; sc0 = MP.get_scratch(0, n_mp)
    ids = [int(m["id"]) for m in meta0]; slot = {k: s for s, k in enumerate(ids)}; cur_id = ids[cur]

    def restore():
        for s in range(K):
            KF.set_meta_raw(s, meta0[s])
        MP.put(0, rec0, arr["obs_off"], arr["obs_kf"], arr["obs_idx"]); MP.set_scratch(0, sc0); MP.build_index(0, n_mp)

    def after():
        return b"".join(KF.get_meta(s)["Tcw"].tobytes() for s in range(K)), MP.get(0, n_mp)[0]["world_pos"].tobytes()

    def records():
        t0 = time.perf_counter()
        o = g.OptimizeEssentialGraph(loop, cur, ks, co, nc, lc, min_weight=a.min_weight, scale_factor=0.0)
        return dict(total=time.perf_counter() - t0), o["result"]

    def earlier():
        t = {}
        t0 = time.perf_counter()
        metas = [KF.get_meta(s) for s in range(K)]; rows = [g.get(s) for s in range(K)]; trees = [g.GetTree(s) for s in range(K)]; loops = [g.GetLoopEdges(s) for s in range(K)]
        rec = MP.get(0, n_mp)[0]; sc = MP.get_scratch(0, n_mp)
        t["fetch"] = time.perf_counter() - t0; t0 = time.perf_counter()
        m = R.Map()
        for s in range(K):
            kf = ER.node(LR.tree(R.KeyFrame(ids[s], [])))
            kf.Tcw = metas[s]["Tcw"].reshape(4, 4); kf.bad = bool(int(metas[s]["flags"]) & 1); kf.fixed = bool(int(metas[s]["flags"]) & 2)
            kf.weights = dict(zip(rows[s][0][0].tolist(), rows[s][0][1].tolist())); kf.ordered = list(zip(rows[s][1][0].tolist(), rows[s][1][1].tolist()))
            kf.parent = None if trees[s][0] == corb.NO_ID else trees[s][0]; kf.children = set(trees[s][2].tolist()); kf.loop_edges = set(loops[s].tolist())
            m.kfs[ids[s]] = kf
        p = ER.plan(m, ids[loop], cur_id, {ids[s]: co[i] for i, s in enumerate(ks)}, {ids[s]: nc[i] for i, s in enumerate(ks)}, {ids[cur]: {ids[loop]}}, a.min_weight)
        rank = {k: r for r, k in enumerate(p["v_ids"])}
        idr = np.where(sc["corrected_by_kf"] == cur_id, sc["corrected_reference"], rec["ref_kf_id"])
        ref = np.array([rank.get(int(x), -1) if not int(f) & 3 else -1 for x, f in zip(idr, rec["flags"])], np.int32)
        t["flatten_python"] = time.perf_counter() - t0; t0 = time.perf_counter()
        G = corb.Optimizer.OptimizeEssentialGraph(dict(S=p["S"], fixed=p["fixed"], vi=p["vi"], vj=p["vj"], meas=p["meas"], points=rec["world_pos"], ref=ref), 20, False)
        t["solve"] = time.perf_counter() - t0; t0 = time.perf_counter()
        for r, k in enumerate(p["v_ids"]):
            if not m.kfs[k].fixed:
                KF.set_meta(slot[k], Tcw=G["Tiw"][r].reshape(16))
        rec = rec.copy(); rec["world_pos"] = G["points"]
        MP.put(0, rec, arr["obs_off"], arr["obs_kf"], arr["obs_idx"]); MP.set_scratch(0, sc); MP.build_index(0, n_mp)
        t["write_back"] = time.perf_counter() - t0
        t["total"] = sum(t.values())
        return t, p["counts"]

    out = dict(config="one client, %d keyframes, %d map points, max_connections 512, min_weight %d, 20 iterations" % (K, n_mp, a.min_weight))
    times = {"records": [], "earlier": []}
    left = {}
    for i in range(a.calls + 3):                                 # three warm-up rounds, the routes alternating
        for name, fn in (("records", records), ("earlier", earlier)):
            restore()
            t, info = fn()
            left[name] = after()
            if i >= 3:
                times[name].append(t)
            if name == "records":
                out["graph"] = info.graph.as_dict(); out["iters_done"] = info.iters_done; out["n_points_moved"] = info.n_points_moved
    out["both_routes_leave_the_same_bytes"] = left["records"] == left["earlier"]
    for name in times:
        out[name] = {k: stats([t[k] for t in times[name]]) for k in times[name][0]}
    out["earlier_without_python_flatten_median_ms"] = round(sum(out["earlier"][k]["median_ms"] for k in ("fetch", "solve", "write_back")), 4)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    line = json.dumps(out)
    open(os.path.join(ROOT, "profiles", "essgraph_rate.json"), "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

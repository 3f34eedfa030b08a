"""Covisibility-graph upkeep on one GPU (corb_covis_*): what a LocalMapping step pays for the graph, beside LocalBundleAdjustment's time per keyframe (README.md).

The map is one client's synth.ba_problem_fast map of the configs[2] shape -- about 2000 features per keyframe, a few hundred keyframes, every point seen by 3..8
keyframes next to each other in time -- put into the stores by synth.map_arrays.  Every call is synchronous (it ends in a device synchronisation), so the host clock
around it is the call's time.  Prints one JSON line, times in ms as median [p10, p90] over --calls calls after --warmup calls:
  update_1        : corb_covis_update of one keyframe (the graph already holds every keyframe: the steady state of LocalMapping)
  local_window    : corb_covis_local_window of one keyframe
  culling         : corb_covis_keyframe_culling of one keyframe
  query_best10    : corb_covis_query(N = 10)
  update_batch    : corb_covis_update of --batch keyframes in one call (the server's insert path), and the same divided by the batch
usage: python tools/covis_rate.py [--kf 300] [--ppk 360] [--calls 200] [--warmup 20] [--batch 256]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import corbload  # noqa: E402


def timed(fn, args_list, warmup, calls):
    for i in range(warmup):
        fn(*args_list[i % len(args_list)])
    ts = []
    for i in range(calls):
        t0 = time.perf_counter(); fn(*args_list[i % len(args_list)]); ts.append(time.perf_counter() - t0)
    ts = np.sort(np.array(ts)) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(ts[int(0.1 * len(ts))]), 4), p90_ms=round(float(ts[int(0.9 * len(ts))]), 4), calls=calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=300)
    ap.add_argument("--ppk", type=int, default=360, help="new points per keyframe; a point is seen by ~5.5 keyframes")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    corb = corbload.load_pkg()
    from corb_slam_amd import synth
    prob = synth.ba_problem_fast(n_clients=1, kf_per_client=a.kf, pts_per_kf=a.ppk, seed=1000, obs_range=(3, 8), window=6)
    arr = synth.map_arrays(prob, a.kf, a.ppk)
    K, n_mp = len(arr["meta"]), len(arr["mp_records"])
    feats = np.diff(arr["feat_off"])
    out = dict(config="one client, %d keyframes, %d map points, features per keyframe median %d / max %d, observations per point max %d"
               % (K, n_mp, int(np.median(feats)), int(feats.max()), arr["max_obs"]))
    if corb.device_count() < 1:
        raise SystemExit("no MI355X visible")
    KF = corb.KeyFrameStore(K, arr["max_features"]); MP = corb.MapPointStore(n_mp, arr["max_obs"])
    KF.put_batch(0, arr["meta"], arr["feat_off"], arr["kp"], None, arr["ur"], None, arr["mp_id"])
    MP.put(0, arr["mp_records"], arr["obs_off"], arr["obs_kf"], arr["obs_idx"]); MP.build_index(0, n_mp)
    g = corb.Covisibility(KF, MP)
    batch = min(a.batch, K)
    slots = np.arange(K, dtype=np.int32)
    g.UpdateConnections(slots)                                   # the graph of the whole map (also the warm-up of the batch shape's kernels)
    rows = [g.get(s) for s in range(K)]
    out["row_entries"] = dict(weight_map_median=int(np.median([len(r[0][0]) for r in rows])), ordered_median=int(np.median([len(r[1][0]) for r in rows])),
                              weight_map_max=int(max(len(r[0][0]) for r in rows)))
    some = [(int(s),) for s in np.linspace(0, K - 1, 16).astype(int)]
    out["update_1"] = timed(lambda s: g.UpdateConnections([s]), some, a.warmup, a.calls)
    ks, nl, ms = g.LocalWindow(some[8][0], K, n_mp)
    out["window_of_slot_%d" % some[8][0]] = dict(n_local=int(nl), n_fixed=int(len(ks) - nl), n_points=int(len(ms)))
    out["local_window"] = timed(lambda s: g.LocalWindow(s, 256, 65536), some, a.warmup, a.calls)
    out["culling"] = timed(lambda s: g.KeyFrameCulling(s, False, 35.0), some, a.warmup, a.calls)
    out["query_best10"] = timed(lambda s: g.GetBestCovisibilityKeyFrames(s, 10), some, a.warmup, a.calls)
    out["update_batch"] = timed(lambda: g.UpdateConnections(slots[:batch]), [()], 3, max(10, a.calls // 10))
    out["update_batch"]["batch"] = batch
    out["update_batch"]["median_ms_per_keyframe"] = round(out["update_batch"]["median_ms"] / batch, 4)
    g.close(); KF.close(); MP.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

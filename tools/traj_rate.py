"""The camera trajectory on records, one GPU: what corb_traj_frames and corb_traj_append cost, host to host.

(a) corb_traj_frames for a log of --entries frames (4541: the length of KITTI 00) over --kf keyframes of which 30 % are culled, beside the only route there is
    without it: corb_kf_store_get_meta and corb_covis_get_tree per keyframe, then the composition on the host by the Python definition (tests/traj_reference.py).
    That route is an UNTUNED HOST LOOP in Python, not a competitor: it is here because a client had nothing else, and there is no earlier figure for a new call.
    Both routes must give the same bytes before anything is timed.
(b) corb_traj_append(Tcr = NULL) per frame, beside corb_track_frame_finish(stage 1) alone and beside finish followed by an append with the returned Tcr: what the
    log costs a tracked frame.  The append alone does not synchronise; its figure is the host's enqueue time, and `append_Tcr_null_synced` adds a wait for the frame
    store's stream through a read of that frame's 240-byte header.

Routes alternate call by call in the same process on the same data; times in ms as median [p10, p90] over --calls calls after --warmup.  Kernel times are not taken.
Prints one JSON line (and writes it to --out).
usage: python tools/traj_rate.py [--kf 300] [--entries 4541] [--calls 200] [--warmup 20] [--out profiles/traj_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import corbload  # noqa: E402
import traj_reference as R  # noqa: E402


def stats(ts, calls):
    ts = np.sort(np.array(ts)) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(ts[int(0.1 * len(ts))]), 4), p90_ms=round(float(ts[int(0.9 * len(ts))]), 4), calls=calls)


def pose(rng, spread=3.0):
    return R.pose(R.rot(rng.normal(0, 1, 3), rng.uniform(0.05, 3.0)), rng.normal(0, spread, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=300)
    ap.add_argument("--entries", type=int, default=4541)
    ap.add_argument("--features", type=int, default=2000, help="features of the tracked frame of (b)")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_rate.json"))
    a = ap.parse_args()
    corb = corbload.load_pkg()
    if corb.device_count() < 1:
        raise SystemExit("no MI355X visible")
    rng = np.random.default_rng(7)
    K, F = a.kf, a.features
    KF = corb.KeyFrameStore(K, 4); MP = corb.MapPointStore(F, 4); g = corb.Covisibility(KF, MP, 8)
    traj = corb.Trajectory(g, a.entries + 1)
    meta = np.zeros(K, corb.KF_META_DTYPE); meta["id"] = np.arange(1, K + 1); meta["nlevels"] = 8
    meta["Tcw"] = np.stack([pose(rng).reshape(16) for _ in range(K)])
    KF.put_batch(0, meta, np.arange(K + 1, dtype=np.int32), np.zeros(K, corb.KP_DTYPE))
    parents = [R.NO_ID] + [int(rng.integers(1, k + 1)) for k in range(1, K)]            # ids: each parent's id is below its child's
    for s in range(K):
        g.SetTree(s, parents[s], False, [])
    culled = [s for s in range(1, K) if rng.uniform() < 0.30]
    for s in rng.permutation(culled):
        traj.set_bad_pose(int(s)); KF.set_meta(int(s), flags=R.KF_BAD)
    for s in range(K):
        KF.set_meta(s, Tcw=pose(rng).reshape(16))
    for i in range(a.entries):
        traj.append(None, 0, int(rng.integers(0, K)), pose(rng, 0.3), 1.4e9 + i / 10.0, bool(rng.uniform() < 0.1))
    out = dict(config="%d keyframes, %d culled, a log of %d frames; the tracked frame of (b) has %d features" % (K, len(culled), a.entries, F),
               timing="host to host; routes alternate call by call; kernel times not measured")

    # ---- (a) the export ----
    def device_route(fmt):
        return traj.frames(-1, fmt)

    entries = [e for e in traj.get_entries()]

    def host_route(fmt):
        store = []
        for s in range(K):
            m = KF.get_meta(s); p, _, _ = g.GetTree(s)
            store.append(dict(id=int(m["id"]), n=1, flags=int(m["flags"]), Tcw=np.array(m["Tcw"], np.float32).reshape(4, 4), parent=p))
        full = np.tile(np.eye(4, dtype=np.float32), (K, 1, 1))
        for s in range(K):
            if store[s]["flags"] & R.KF_BAD:
                full[s] = traj.get_tcp(s)
        return R.frames(entries, store, full, -1, fmt)

    frames = {}
    for fmt, name in ((R.KITTI, "kitti"), (R.TUM, "tum")):
        d = device_route(fmt); h = host_route(fmt)
        assert d[0].tobytes() == h[0].tobytes() and d[1].tobytes() == h[1].tobytes() and d[2].tolist() == h[2].tolist(), "%s: the two routes give different bytes" % name
        ts = dict(corb_traj_frames=[], host_loop_python_definition=[])
        for i in range(a.warmup + a.calls):
            for route, fn in (("corb_traj_frames", device_route), ("host_loop_python_definition", host_route)):
                t0 = time.perf_counter(); fn(fmt); t = time.perf_counter() - t0
                if i >= a.warmup:
                    ts[route].append(t)
        frames[name] = {k: stats(v, a.calls) for k, v in ts.items()}
        frames[name]["rows"] = int(len(d[0])); frames[name]["max_chain"] = int(d[3].max_chain); frames[name]["routes_give_equal_bytes"] = True
    frames["note"] = "host_loop_python_definition is an untuned host loop in Python (get_meta and get_tree per keyframe, then tests/traj_reference.py): not a competitor"
    out["frames"] = frames

    # ---- (b) the append beside the end of a tracked frame ----
    rec = np.zeros(F, corb.MP_RECORD_DTYPE); rec["id"] = np.arange(100000, 100000 + F); rec["n_obs"] = 1
    MP.put(0, rec, np.arange(F + 1, dtype=np.int32), np.ones(F, np.uint64), np.zeros(F, np.uint32)); MP.build_index(0, F)
    FR = corb.KeyFrameStore(1, F)
    fm = np.zeros(1, corb.KF_META_DTYPE); fm["id"] = 900000; fm["nlevels"] = 8; fm["Tcw"] = pose(rng).reshape(16)
    FR.put_batch(0, fm, np.array([0, F], np.int32), np.zeros(F, corb.KP_DTYPE), mp_id=rec["id"].astype(np.uint64))
    ref = 0

    def finish_alone():
        return FR.TrackFrameFinish(0, KF, ref, MP, 1)

    def finish_then_append():
        traj.append(FR, 0, ref, FR.TrackFrameFinish(0, KF, ref, MP, 1), 1.0, False)

    def append_null():
        traj.append(FR, 0, ref, None, 1.0, False)

    def append_null_synced():
        traj.append(FR, 0, ref, None, 1.0, False); FR.get_meta(0)                        # a 240-byte read on the frame store's stream: the wait

    Tcr = finish_alone(); traj.reset(); append_null(); finish_then_append()
    e = traj.get_entries()
    assert e[0].tobytes() == e[1].tobytes() and e[0]["Tcr"].tobytes() == Tcr.tobytes(), "the two appends leave different entries"
    routes = dict(finish_stage1_alone=finish_alone, finish_then_append_Tcr=finish_then_append, append_Tcr_null_enqueue_only=append_null, append_Tcr_null_synced=append_null_synced)
    ts = {k: [] for k in routes}
    for i in range(a.warmup + a.calls):
        for name, fn in routes.items():
            traj.reset()
            t0 = time.perf_counter(); fn(); t = time.perf_counter() - t0
            if i >= a.warmup:
                ts[name].append(t)
    app = {k: stats(v, a.calls) for k, v in ts.items()}
    spread = app["finish_stage1_alone"]["p90_ms"] - app["finish_stage1_alone"]["p10_ms"]
    app["log_cost_ms"] = round(app["finish_then_append_Tcr"]["median_ms"] - app["finish_stage1_alone"]["median_ms"], 4)
    app["log_cost_within_finish_spread"] = bool(app["log_cost_ms"] <= spread)
    app["entries_equal"] = True
    out["append"] = app
    FR.close(); traj.close(); g.close(); KF.close(); MP.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

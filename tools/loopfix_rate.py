"""CorrectLoop's propagation and the spread of a global bundle adjustment on one GPU (corb_loop_correct_store, corb_gba_propagate_store): what a loop event pays on
records, beside the bytes a host round trip of the same records would move.

The map is synthetic and shaped for these two calls only: --kf keyframes of --features feature slots whose spanning tree is a CHAIN (keyframe i the only child of
keyframe i - 1: the deepest tree a map of that size can have, one queue entry per generation of the walk); keyframe i holds its own --ppk points and those of
keyframe i - 1; the last keyframe is the current one and shares one further point with each of the --set keyframes before it, so that UpdateConnections with th = 1
makes exactly them its covisible set.  A tenth of the keyframes and 60 % of the points start without the mark of the global BA.
Every call is synchronous, so the host clock around it is the call's time.  Prints one JSON line, times in ms as median [p10, p90] over --calls calls after --warmup:
  correct_loop        : corb_loop_correct_store with scale_factor 1.2; the scratch of the set's points is cleared before every call (untimed) so that every call moves them
  gba_propagate_first : the first corb_gba_propagate_store (a tenth of the chain is composed), one call
  gba_propagate       : the following calls (every keyframe carries the mark by then: the walk pops and pushes, the points are all set or moved)
  *_round_trip_bytes  : the keyframe headers (256 B) and map-point records the call reads and writes, once down and once up
usage: python tools/loopfix_rate.py [--kf 1200] [--ppk 100] [--features 320] [--set 100] [--calls 50] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import corbload  # noqa: E402

LOOP_KF = 4242


def timed(fn, warmup, calls, before=None):
    ts = []
    for i in range(warmup + calls):
        if before:
            before()
        t0 = time.perf_counter(); fn(); t = time.perf_counter() - t0
        if i >= warmup:
            ts.append(t)
    ts = np.sort(np.array(ts)) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(ts[int(0.1 * len(ts))]), 4), p90_ms=round(float(ts[int(0.9 * len(ts))]), 4), calls=calls)


def poses(rng, n):
    """n rigid poses as float32 [n, 16]"""
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1)[:, None]
    x, y, z, w = q.T
    T = np.zeros((n, 4, 4)); T[:, 3, 3] = 1
    T[:, 0, 0] = 1 - 2 * (y * y + z * z); T[:, 0, 1] = 2 * (x * y - z * w); T[:, 0, 2] = 2 * (x * z + y * w)
    T[:, 1, 0] = 2 * (x * y + z * w); T[:, 1, 1] = 1 - 2 * (x * x + z * z); T[:, 1, 2] = 2 * (y * z - x * w)
    T[:, 2, 0] = 2 * (x * z - y * w); T[:, 2, 1] = 2 * (y * z + x * w); T[:, 2, 2] = 1 - 2 * (x * x + y * y)
    T[:, :3, 3] = rng.normal(size=(n, 3)) * 3
    return T.reshape(n, 16).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=1200)
    ap.add_argument("--ppk", type=int, default=100, help="own points per keyframe")
    ap.add_argument("--features", type=int, default=320)
    ap.add_argument("--set", type=int, default=100, help="covisible keyframes of the current one")
    ap.add_argument("--connections", type=int, default=128, help="max_connections of the graph")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    K, ppk, F, ns = a.kf, a.ppk, a.features, min(a.set, a.kf - 1)
    assert F >= 2 * ppk + ns and a.connections > ns
    corb = corbload.load_pkg()
    if corb.device_count() < 1:
        raise SystemExit("no MI355X visible")
    rng = np.random.default_rng(7)
    n_mp = K * ppk + ns
    KF = corb.KeyFrameStore(K, F); MP = corb.MapPointStore(n_mp, 4)
    cur = K - 1
    # keyframe records: own points at features [0, ppk), the previous keyframe's at [ppk, 2 ppk), the shared points of the set behind them
    step = 2000
    for first in range(0, K, step):
        n = min(step, K - first)
        meta = np.zeros(n, corb.KF_META_DTYPE); ids = np.arange(first, first + n, dtype=np.uint64) + 1
        meta["id"] = ids; meta["nlevels"] = 8; meta["Tcw"] = poses(rng, n); meta["TcwGBA"] = poses(rng, n)
        meta["ba_global_for_kf"] = np.where((ids % 10 == 0) & (ids > 1), 0, LOOP_KF)
        cnt = np.full(n, 2 * ppk + 1, np.int32)
        if first + n == K:
            cnt[-1] = 2 * ppk + ns
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        mp_id = np.full(off[-1], corb.NO_ID, np.uint64)
        for j in range(n):
            i = first + j; o = off[j]
            mp_id[o: o + ppk] = np.arange(i * ppk, (i + 1) * ppk)
            if i > 0:
                mp_id[o + ppk: o + 2 * ppk] = np.arange((i - 1) * ppk, i * ppk)
            if cur - ns <= i < cur:
                mp_id[o + 2 * ppk] = K * ppk + (i - (cur - ns))
            if i == cur:
                mp_id[o + 2 * ppk: o + 2 * ppk + ns] = K * ppk + np.arange(ns)
        kp = np.zeros(off[-1], corb.KP_DTYPE); kp["octave"] = rng.integers(0, 8, off[-1])
        KF.put_batch(first, meta, off, kp, None, None, None, mp_id)
    # map-point records: point p of keyframe i = p // ppk is seen by i (feature p % ppk) and i + 1 (feature ppk + p % ppk); a shared point by its member and the current keyframe
    pstep = 500000
    for first in range(0, n_mp, pstep):
        n = min(pstep, n_mp - first)
        p = np.arange(first, first + n)
        own = p < K * ppk
        i = np.where(own, p // ppk, cur - ns + (p - K * ppk))
        rec = np.zeros(n, corb.MP_RECORD_DTYPE); rec["id"] = p; rec["ref_kf_id"] = i + 1; rec["n_obs"] = np.where(own & (i == K - 1), 1, 2)
        rec["world_pos"] = rng.normal(size=(n, 3)) * 4; rec["pos_gba"] = rng.normal(size=(n, 3)) * 4
        rec["ba_global_for_kf"] = np.where(rng.random(n) < 0.4, LOOP_KF, 0)
        obs_off = np.concatenate([[0], np.cumsum(rec["n_obs"])]).astype(np.int32)
        okf = np.zeros(obs_off[-1], np.uint64); oidx = np.zeros(obs_off[-1], np.uint32)
        okf[obs_off[:-1]] = i + 1; oidx[obs_off[:-1]] = np.where(own, p % ppk, 2 * ppk)
        two = rec["n_obs"] == 2
        okf[obs_off[:-1][two] + 1] = np.where(own, i + 2, cur + 1)[two]
        oidx[obs_off[:-1][two] + 1] = np.where(own, ppk + p % ppk, 2 * ppk + (p - K * ppk))[two]
        MP.put(first, rec, obs_off, okf, oidx)
    MP.build_index(0, n_mp)
    g = corb.Covisibility(KF, MP, a.connections)
    for first in range(0, K, 4096):
        g.UpdateConnections(np.arange(first, min(K, first + 4096), dtype=np.int32), th=1)
    for s in range(K):                                           # the chain
        g.SetTree(s, corb.NO_ID if s == 0 else s, False, [s + 2] if s + 1 < K else [])
    out = dict(config="%d keyframes of %d feature slots, %d map points, a chain-shaped tree %d deep, max_connections %d" % (K, F, n_mp, K, a.connections))
    cov = g.GetVectorCovisibleKeyFrames(cur)
    Scw = np.array([0.01, -0.02, 0.015, 0.9996, 0.3, -0.2, 0.1, 0.9])
    Scw[:4] /= np.linalg.norm(Scw[:4])
    lo = (cur - ns) * ppk; zero = np.zeros(n_mp - lo, corb.MP_SCRATCH_DTYPE)
    ks, co, nc, npts = g.CorrectLoop(cur, Scw, 1.2)
    out["correct_loop"] = timed(lambda: g.CorrectLoop(cur, Scw, 1.2), a.warmup, a.calls, before=lambda: MP.set_scratch(lo, zero))
    out["correct_loop"].update(set=int(len(ks)), covisibles=int(len(cov)), points_corrected=int(npts))
    out["correct_loop_round_trip_bytes"] = 2 * (int(len(ks)) * 256 + int(npts) * MP.record_bytes())
    t0 = time.perf_counter(); r = g.PropagateGlobalBA([0], LOOP_KF); t = time.perf_counter() - t0
    out["gba_propagate_first"] = dict(ms=round(t * 1e3, 4), **{k: getattr(r, k) for k, _ in r._fields_})
    calls = max(3, a.calls // 5) if K > 5000 else a.calls
    out["gba_propagate"] = timed(lambda: g.PropagateGlobalBA([0], LOOP_KF), min(a.warmup, 2), calls)
    out["gba_propagate_round_trip_bytes"] = 2 * (K * 256 + n_mp * MP.record_bytes())
    g.close(); KF.close(); MP.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

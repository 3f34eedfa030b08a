"""Per-call time of the Sim3Solver RANSAC on one GPU: corb_sim3_ransac (host arrays) and corb_sim3_ransac_store (records) for 1 and 3 candidates x 300 iterations x
N = 100 and N = 1000 correspondences, beside corb_optimize_sim3 on the same candidates in the same process for context.

Every call is timed host to host through ctypes with its arguments built beforehand (a host clock around a synchronous call), after 30 warm-up calls per shape;
the figure is the median of --calls calls, with the 90th percentile.  min_inliers = 20, p = 0.99, 30 % unrelated correspondences, so the cap stays at 300.
Launches per call: host arrays 2 (prepare, hypotheses); records 4 (prepare, scan, compaction, hypotheses).
Prints one JSON line.  usage: python tools/sim3_ransac_rate.py [--calls 200]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import corbload  # noqa: E402

K = (718.856, 718.856, 607.1928, 185.2157)
ITS = 300


def rot(rng):
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax); a = rng.uniform(0.1, 0.5)
    S = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * S + (1 - np.cos(a)) * S @ S


def candidate(seed, n):
    """camera coordinates of n correspondences of a similarity, 30 % of them unrelated"""
    rng = np.random.default_rng(seed)
    R, t, s = rot(rng), rng.uniform(-0.5, 0.5, 3), 1.1
    box = lambda m: np.stack([rng.uniform(-6, 6, m), rng.uniform(-2, 2, m), rng.uniform(5, 30, m)], axis=1)
    x2 = box(n); x1 = s * x2 @ R.T + t + rng.normal(scale=0.002, size=(n, 3))
    bad = rng.random(n) < 0.3; x1[bad] = box(int(bad.sum()))
    return dict(p1c=x1.astype(np.float32), p2c=x2.astype(np.float32), sigma2_1=np.ones(n, np.float32), sigma2_2=np.ones(n, np.float32), K1=K, K2=K,
                R12=R, t12=t, s12=s)


def timed(fn, calls):
    for _ in range(30):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    ts = np.sort(np.array(ts)) * 1e6
    return dict(median_us=round(float(np.median(ts)), 1), p90_us=round(float(ts[int(0.9 * len(ts))]), 1))


def host_call(corb, cands, rv):
    L = corb.load(); n = len(cands); N = len(cands[0]["p1c"])
    arr = (corb._Sim3RansacProblem * n)(*[corb._Sim3RansacProblem(N, corb._p(c["p1c"]), corb._p(c["p2c"]), corb._p(c["sigma2_1"]), corb._p(c["sigma2_2"]), *K, *K) for c in cands])
    cap = np.zeros(n, np.int32); ne = np.zeros(n, np.int32); ev = np.zeros((n, ITS), corb.SIM3_EVENT_DTYPE); fl = np.zeros((n, ITS, N), np.uint8)

    def fn():
        rc = L.corb_sim3_ransac(C.cast(arr, C.c_void_p), n, 0.99, 20, ITS, 0, corb._p(rv), ITS, N, corb._p(cap), corb._p(ne), corb._p(ev), corb._p(fl), None, None, 0)
        assert rc == 0
    return fn, (cap, ne)


def record_call(corb, cands, rv):
    """keyframe 1 at slot 0 and the candidates behind it, identity poses: the points' world coordinates are their camera coordinates"""
    L = corb.load(); n = len(cands); N = len(cands[0]["p1c"])
    KF = corb.KeyFrameStore(n + 1, N); MP = corb.MapPointStore((n + 1) * N, 2)
    kp = np.zeros(N, corb.KP_DTYPE); desc = np.zeros((N, 32), np.uint8)
    rec = np.zeros((n + 1) * N, corb.MP_RECORD_DTYPE); rec["id"] = 1 + np.arange(len(rec)); rec["n_obs"] = 1
    rec["world_pos"][:N] = cands[0]["p1c"]                            # (one keyframe 1 for all candidates: only candidate 0's points fit it)
    for c, cd in enumerate(cands):
        rec["world_pos"][(c + 1) * N: (c + 2) * N] = cd["p2c"]
    okf = np.repeat(np.arange(n + 1), N).astype(np.uint64) + 10; oidx = np.tile(np.arange(N), n + 1).astype(np.uint32)
    MP.put(0, rec, np.arange(len(rec) + 1, dtype=np.int32), okf, oidx); MP.build_index(0, len(rec))
    for slot in range(n + 1):
        KF.put(slot, kp, desc, None, None, keyframe_id=10 + slot)
        KF.set_meta(slot, id=10 + slot, client_id=1, flags=0, fx=K[0], fy=K[1], cx=K[2], cy=K[3], bf=386.0, nlevels=8, Tcw=np.eye(4, dtype=np.float32).reshape(16))
        KF.set_map_points(slot, rec["id"][slot * N: (slot + 1) * N])
    cam = corb.TrackCamera.make(K[0], K[1], K[2], K[3], 386.0, 0.537, 0.0, 1241.0, 0.0, 376.0, (np.float32(1.2) ** np.arange(8)).astype(np.float32))
    cams = (corb.TrackCamera * n)(*[cam] * n); slots = np.arange(1, n + 1, dtype=np.int32)
    ids = np.concatenate([rec["id"][(c + 1) * N: (c + 2) * N] for c in range(n)]).astype(np.uint64)
    cap = np.zeros(n, np.int32); ne = np.zeros(n, np.int32); ev = np.zeros((n, ITS), corb.SIM3_EVENT_DTYPE); fl = np.zeros((n, ITS, N), np.uint8); nc = np.zeros(n, np.int32)

    def fn():
        rc = L.corb_sim3_ransac_store(KF.h, 0, corb._p(slots), n, MP.h, C.byref(cam), C.cast(cams, C.c_void_p), corb._p(ids), 0.99, 20, ITS, 0, corb._p(rv), ITS,
                                      corb._p(cap), corb._p(ne), corb._p(ev), corb._p(fl), corb._p(nc), None, None, None)
        assert rc == 0
    return fn, (cap, ne, nc), (KF, MP)


def optimize_call(corb, cands):
    def proj(x):
        return np.stack([K[0] * x[:, 0] / x[:, 2] + K[2], K[1] * x[:, 1] / x[:, 2] + K[3]], axis=1).astype(np.float32)
    probs = [dict(p1c=c["p1c"], p2c=c["p2c"], obs1=proj(c["p1c"]), obs2=proj(c["p2c"]), inv_sigma2_1=np.ones(len(c["p1c"]), np.float32), inv_sigma2_2=np.ones(len(c["p1c"]), np.float32),
                  fx1=K[0], fy1=K[1], cx1=K[2], cy1=K[3], fx2=K[0], fy2=K[1], cx2=K[2], cy2=K[3], R12=c["R12"], t12=c["t12"], s12=c["s12"]) for c in cands]
    return lambda: corb.Optimizer.OptimizeSim3(probs, 10.0, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    corb = corbload.load_pkg()
    if corb.device_count() < 1:
        raise SystemExit("no MI355X visible")
    out = {}
    for n_cand in (1, 3):
        for N in (100, 1000):
            cands = [candidate(50 + 7 * c + N, N) for c in range(n_cand)]
            rv = np.random.RandomState(N + n_cand).randint(0, 2 ** 31, (n_cand, ITS, 3)).astype(np.int32)
            key = "%dx%dx%d" % (n_cand, ITS, N)
            fn, res = host_call(corb, cands, rv)
            r = timed(fn, a.calls); r.update(ransac_max_its=res[0].tolist(), n_events=res[1].tolist())
            out["host_arrays_" + key] = r
            fn, res, stores = record_call(corb, cands, rv)
            r = timed(fn, a.calls); r.update(ransac_max_its=res[0].tolist(), n_events=res[1].tolist(), n_corr=res[2].tolist())
            out["records_" + key] = r
            for s in stores:
                s.close()
            out["optimize_sim3_%dx%d" % (n_cand, N)] = timed(optimize_call(corb, cands), a.calls)
    out["launches_per_call"] = dict(host_arrays=2, records=4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

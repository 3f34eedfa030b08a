"""Per-call time of the PnPsolver RANSAC on one GPU: corb_pnp_ransac (host arrays) and corb_pnp_ransac_store (records) for 1 and 8 candidates x N = 100 and N = 1000
correspondences with the reference's parameters (0.99, 10, 300, 4, 0.5, 5.991: a cap of 35 hypotheses per candidate, Refine() at every record), beside
corb_track_pose_optimization on the same frame record in the same process for context, and beside the serial CPU loop: tests/host/pnp_math_main.cpp (csrc/pnp_math.h
built with the host compiler, -O3 -ffp-contract=off) evaluating the same drawn sets plus one Refine()-sized set per candidate.

Every library call is timed host to host through ctypes with its arguments built beforehand (a host clock around a synchronous call), after 30 warm-up calls per
shape; the figure is the median of --calls calls, with the 90th percentile.  60 % of the correspondences are true, 0.5 px of noise.  Launches per call: host arrays 3
(prepare, hypotheses, Refine); records 5 (prepare, scan, compaction, hypotheses, Refine).
Prints one JSON line.  usage: python tools/pnp_ransac_rate.py [--calls 200]"""
import argparse
import ctypes as C
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import corbload  # noqa: E402

K = (718.856, 718.856, 607.1928, 185.2157)
PAR = (0.99, 10, 300, 4, 0.5, 5.991)
ITS = 300
SCALE = (np.float32(1.2) ** np.arange(8)).astype(np.float32)


def rot(rng):
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax); a = rng.uniform(0.1, 0.5)
    S = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * S + (1 - np.cos(a)) * S @ S


def frame(seed, n):
    """pixels of n features of a frame at a known pose"""
    rng = np.random.default_rng(seed)
    R, t = rot(rng), rng.uniform(-0.5, 0.5, 3)
    Xc = np.stack([rng.uniform(-6, 6, n), rng.uniform(-2, 2, n), rng.uniform(5, 30, n)], axis=1)
    uv = np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1) + rng.normal(scale=0.5, size=(n, 2))
    return dict(R=R, t=t, Xc=Xc, uv=uv.astype(np.float32))


def candidate(seed, fr):
    """world points matched to the frame's features, 60 % of them the true ones"""
    rng = np.random.default_rng(seed); n = len(fr["uv"])
    W = (fr["Xc"] - fr["t"]) @ fr["R"]
    bad = rng.random(n) >= 0.6; W[bad] = rng.uniform(-8, 8, (int(bad.sum()), 3))
    return dict(p3dw=W.astype(np.float32), p2d=fr["uv"], sigma2=np.ones(n, np.float32), K=K)


def timed(fn, calls):
    for _ in range(30):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    ts = np.sort(np.array(ts)) * 1e6
    return dict(median_us=round(float(np.median(ts)), 1), p90_us=round(float(ts[int(0.9 * len(ts))]), 1))


def host_call(corb, cands, rv):
    L = corb.load(); n = len(cands); N = len(cands[0]["sigma2"])
    arr = (corb._PnPRansacProblem * n)(*[corb._PnPRansacProblem(N, corb._p(c["p3dw"]), corb._p(c["p2d"]), corb._p(c["sigma2"]), *K) for c in cands])
    cap = np.zeros(n, np.int32); mi = np.zeros(n, np.int32); nr = np.zeros(n, np.int32); rec = np.zeros((n, ITS), corb.PNP_RECORD_DTYPE)
    bf = np.zeros((n, ITS, N), np.uint8); rf = np.zeros((n, ITS, N), np.uint8); cnt = np.zeros((n, ITS), np.int32)

    def fn():
        rc = L.corb_pnp_ransac(C.cast(arr, C.c_void_p), n, *PAR, 0, corb._p(rv), ITS, N, corb._p(cap), corb._p(mi), corb._p(nr), corb._p(rec), corb._p(bf), corb._p(rf),
                               corb._p(cnt), None, None, 0)
        assert rc == 0
    return fn, (cap, nr, cnt, bf)


def record_call(corb, fr, cands, rv):
    L = corb.load(); n = len(cands); N = len(fr["uv"])
    KF = corb.KeyFrameStore(1, N); MP = corb.MapPointStore(n * N, 2)
    kp = np.zeros(N, corb.KP_DTYPE); kp["x"] = fr["uv"][:, 0]; kp["y"] = fr["uv"][:, 1]
    rec = np.zeros(n * N, corb.MP_RECORD_DTYPE); rec["id"] = 1 + np.arange(len(rec))
    for c, cd in enumerate(cands):
        rec["world_pos"][c * N: (c + 1) * N] = cd["p3dw"]
    MP.put(0, rec, np.zeros(len(rec) + 1, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint32)); MP.build_index(0, len(rec))
    KF.put(0, kp, np.zeros((N, 32), np.uint8), None, None, keyframe_id=10)
    T = np.eye(4, dtype=np.float32); T[:3, :3] = fr["R"]; T[:3, 3] = fr["t"]
    KF.set_meta(0, id=10, client_id=1, flags=0, fx=K[0], fy=K[1], cx=K[2], cy=K[3], bf=386.0, nlevels=8, Tcw=T.reshape(16))
    KF.set_map_points(0, rec["id"][:N])
    cam = corb.TrackCamera.make(K[0], K[1], K[2], K[3], 386.0, 0.537, 0.0, 1241.0, 0.0, 376.0, SCALE)
    ids = rec["id"].astype(np.uint64).copy()
    cap = np.zeros(n, np.int32); mi = np.zeros(n, np.int32); nr = np.zeros(n, np.int32); rcd = np.zeros((n, ITS), corb.PNP_RECORD_DTYPE)
    bf = np.zeros((n, ITS, N), np.uint8); rf = np.zeros((n, ITS, N), np.uint8); nc = np.zeros(n, np.int32)

    def fn():
        rc = L.corb_pnp_ransac_store(KF.h, 0, MP.h, C.byref(cam), corb._p(ids), n, *PAR, 0, corb._p(rv), ITS, corb._p(cap), corb._p(mi), corb._p(nr), corb._p(rcd), corb._p(bf),
                                     corb._p(rf), corb._p(nc), None, None, None, None)
        assert rc == 0

    def pose_opt():
        KF.TrackPoseOptimization(0, MP, cam, T)
    return fn, pose_opt, (cap, nr, nc), (KF, MP)


def cpu_serial(cands, rv, res, exe, tmp):
    """the same drawn sets (the first cap hypotheses per candidate) plus the first record's inlier set, evaluated one after the other by the host program"""
    if exe is None:
        return None
    cap, nr, cnt, bf = res
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pnpsolver_reference as R
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(cands)))
        for c, cd in enumerate(cands):
            N = len(cd["sigma2"])
            sets = [R.draw_set(rv[c, i], 4, N) for i in range(int(cap[c]))]
            if nr[c] > 0:
                sets.append(np.flatnonzero(bf[c, 0]).tolist())
            f.write(struct.pack("<ii4f", N, len(sets), *K))
            f.write(np.concatenate([cd["p3dw"], cd["p2d"], (cd["sigma2"] * np.float32(PAR[5]))[:, None]], axis=1).astype("<f4").tobytes())
            for s in sets:
                f.write(struct.pack("<i", len(s))); f.write(np.asarray(s, "<i4").tobytes())
    out = subprocess.run([exe, fin, fout, "50"], check=True, capture_output=True, text=True).stdout
    return round(float(out.split()[1]) * 1e6, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    corb = corbload.load_pkg()
    if corb.device_count() < 1:
        raise SystemExit("no MI355X visible")
    tmp = tempfile.mkdtemp(); exe = None
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx:
        exe = os.path.join(tmp, "pnp_math_main")
        subprocess.run([cxx, "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "pnp_math_main.cpp"),
                        "-o", exe], check=True)
    out = {}
    for n_cand in (1, 8):
        for N in (100, 1000):
            fr = frame(40 + N, N)
            cands = [candidate(50 + 7 * c + N, fr) for c in range(n_cand)]
            rv = np.random.RandomState(N + n_cand).randint(0, 2 ** 31, (n_cand, ITS, 4)).astype(np.int32)
            key = "%dx%d" % (n_cand, N)
            fn, res = host_call(corb, cands, rv)
            r = timed(fn, a.calls); r.update(ransac_max_its=res[0].tolist(), n_records=res[1].tolist())
            out["host_arrays_" + key] = r
            out["cpu_serial_us_" + key] = cpu_serial(cands, rv, res, exe, tmp)
            fn, pose_opt, res, stores = record_call(corb, fr, cands, rv)
            r = timed(fn, a.calls); r.update(ransac_max_its=res[0].tolist(), n_records=res[1].tolist(), n_corr=res[2].tolist())
            out["records_" + key] = r
            if n_cand == 1:
                try:
                    out["track_pose_optimization_%d" % N] = timed(pose_opt, a.calls)
                except corb.CorbError as e:                                # context only: the figure is left out, with the reason
                    out["track_pose_optimization_%d" % N] = str(e)
            for s in stores:
                s.close()
    out["launches_per_call"] = dict(host_arrays=3, records=5)
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

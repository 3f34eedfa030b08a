"""Per-call time of the monocular Initializer on one GPU: corb_mono_initialize for 1 and 8 problems x N = 100, 300 and 1000 matches with the reference's parameters
(sigma 1.0, 200 iterations: 400 hypotheses per problem, then up to 8 CheckRT passes), beside the serial CPU loop: tests/host/initializer_main.cpp (csrc/init_math.h
built with the host compiler, -O3 -ffp-contract=off) running the same problems and draws on one core.

Every library call is timed host to host through ctypes with its arguments built beforehand (a host clock around a synchronous call), after 30 warm-up calls per
shape; the figure is the median of --calls calls, with the 90th percentile.  General scenes (4-20 m depth, 0.3 m baseline, 0.5 px noise), 10 % of the keys of each
frame unmatched.  Four launches per call.  --only KEY (e.g. 8x1000) runs one shape, for a kernel trace.
Prints one JSON line.  usage: python tools/initializer_rate.py [--calls 200] [--only PxN]"""
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
ITS = 200


def scene(seed, N):
    rng = np.random.default_rng(seed)
    c, s = np.cos(0.02), np.sin(0.02)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]); t = np.array([0.3, 0.0, 0.0])
    uv1 = np.stack([rng.uniform(20, 1221, N), rng.uniform(20, 356, N)], axis=1)
    X = np.stack([(uv1[:, 0] - K[2]) / K[0], (uv1[:, 1] - K[3]) / K[1], np.ones(N)], axis=1) * rng.uniform(4.0, 20.0, N)[:, None]
    X2 = X @ R.T + t
    uv2 = np.stack([K[0] * X2[:, 0] / X2[:, 2] + K[2], K[1] * X2[:, 1] / X2[:, 2] + K[3]], axis=1)
    uv1 = uv1 + rng.normal(0, 0.5, uv1.shape); uv2 = uv2 + rng.normal(0, 0.5, uv2.shape)
    n1 = n2 = N + N // 10
    keys1 = np.stack([rng.uniform(0, 1241, n1), rng.uniform(0, 376, n1)], axis=1); keys2 = np.stack([rng.uniform(0, 1241, n2), rng.uniform(0, 376, n2)], axis=1)
    i1 = np.sort(rng.permutation(n1)[:N]); i2 = rng.permutation(n2)[:N]
    keys1[i1] = uv1; keys2[i2] = uv2
    m = np.full(n1, -1, np.int32); m[i1] = i2
    return dict(keys1=keys1.astype(np.float32), keys2=keys2.astype(np.float32), matches12=m)


def timed(fn, calls):
    for _ in range(30):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    ts = np.sort(np.array(ts)) * 1e6
    return dict(median_us=round(float(np.median(ts)), 1), p90_us=round(float(ts[int(0.9 * len(ts))]), 1))


def device_call(corb, prs, rv):
    L = corb.load(); n = len(prs)
    keep = [(corb._keys(p["keys1"]), corb._keys(p["keys2"]), p["matches12"]) for p in prs]
    arr = (corb._InitProblem * n)(*[corb._InitProblem(corb._p(a), len(a), corb._p(b), len(b), corb._p(m), *K) for a, b, m in keep])
    stride = max(len(a) for a, _, _ in keep)
    res = np.zeros(n, corb.INIT_RESULT_DTYPE); p3d = np.zeros((n, stride, 3), np.float32); tri = np.zeros((n, stride), np.uint8)

    def fn():
        rc = L.corb_mono_initialize(C.cast(arr, C.c_void_p), n, 1.0, ITS, 1.0, 50, corb._p(rv), stride, 0, corb._p(res), corb._p(p3d), corb._p(tri), None, None, None, 0)
        assert rc == 0
    return fn, res, keep


def cpu_serial(prs, rv, exe, tmp):
    if exe is None:
        return None
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<iiffi", len(prs), ITS, 1.0, 1.0, 50))
        for p in prs:
            f.write(struct.pack("<ii4f", len(p["keys1"]), len(p["keys2"]), *K))
            f.write(p["keys1"].astype("<f4").tobytes()); f.write(p["keys2"].astype("<f4").tobytes()); f.write(p["matches12"].astype("<i4").tobytes())
        f.write(np.ascontiguousarray(rv, "<i4").tobytes())
    out = subprocess.run([exe, fin, fout, "5"], check=True, capture_output=True, text=True).stdout
    return round(float(out.split()[1]) * 1e6, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    corb = corbload.load_pkg()
    if corb.device_count() < 1:
        raise SystemExit("no MI355X visible")
    tmp = tempfile.mkdtemp(); exe = None
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx and not a.only:
        exe = os.path.join(tmp, "initializer_main")
        subprocess.run([cxx, "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "initializer_main.cpp"),
                        "-o", exe], check=True)
    out = {}
    for n_prob in (1, 8):
        for N in (100, 300, 1000):
            key = "%dx%d" % (n_prob, N)
            if a.only and a.only != key:
                continue
            prs = [scene(60 + 7 * c + N, N) for c in range(n_prob)]
            rv = np.random.RandomState(N + n_prob).randint(0, 2 ** 31, (n_prob, ITS, 8)).astype(np.int32)
            fn, res, keep = device_call(corb, prs, rv)
            r = timed(fn, a.calls); r.update(status=res["status"].tolist(), model=res["model"].tolist(), n_inliers=res["n_inliers"].tolist())
            out["device_" + key] = r
            out["cpu_serial_us_" + key] = cpu_serial(prs, rv, exe, tmp)
    out["launches_per_call"] = 4
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

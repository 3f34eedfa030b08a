"""Host-to-host time of vocabulary training on the device (corb_voc_train) beside the level-by-level host function of csrc/voctrain_math.h on one core
(tests/host/voctrain_main.cpp built -O3 as a shared object and loaded into this process, the same machine), on the same seeded input: k = 10, L = 5, 2^20 descriptors in
512 images.  The descriptors are noisy copies of a few thousand centres, themselves noisy copies of a few dozen, so the tree is not degenerate.  The two vocabularies must
be equal bit for bit.  A new call has no parent-commit time; the host restatement is what the device time stands beside, and no ratio is fixed.  The device call is timed
by a host clock around it (it ends in a synchronise and a read-back), median of the repeats after one warm-up call; the host function runs once.  Writes
profiles/voc_train_rate.json and prints it as one JSON line.      python tools/voc_train_rate.py [--features 1048576] [--images 512] [--repeats 3] [--no-host]"""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import corbload                                                            # noqa: E402


def clustered(n, seed):
    r = np.random.default_rng(seed)

    def noisy(src, p):
        return np.bitwise_xor(src, np.packbits(r.random((len(src), 256)) < p, axis=1))
    top = r.integers(0, 256, (48, 32), dtype=np.uint8)
    mid = noisy(top[r.integers(0, len(top), 4096)], 0.10)
    return noisy(mid[r.integers(0, len(mid), n)], 0.04)


def build_partner(tmp):
    so = os.path.join(tmp, "libvt_host.so")
    subprocess.run([shutil.which("g++") or "c++", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DVT_HOST_SHARED", "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "voctrain_main.cpp"), "-o", so], check=True)
    H = C.CDLL(so)
    H.vt_host_train.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.POINTER(C.c_int)]
    return H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=1 << 20); ap.add_argument("--images", type=int, default=512); ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--k", type=int, default=10); ap.add_argument("--L", type=int, default=5); ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-host", action="store_true"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voc_train_rate.json"))
    a = ap.parse_args()
    corb = corbload.load_pkg()
    if corb.device_count() < 1:
        raise SystemExit("voc_train_rate: no MI355X visible; a time needs the device")
    desc = np.ascontiguousarray(clustered(a.features, a.seed))
    off = np.linspace(0, a.features, a.images + 1).astype(np.int32)
    sets = [desc[off[i]:off[i + 1]] for i in range(a.images)]
    times = []
    flat = stats = None
    for rep in range(a.repeats + 1):                                       # the first call is the warm-up: code objects, the LDS opt-in
        t0 = time.perf_counter()
        v = corb.Vocabulary.train(sets, a.k, a.L, a.seed, 100)
        dt = (time.perf_counter() - t0) * 1e3
        if rep:
            times.append(dt)
        flat, stats = v.flat(), v.train_stats
        v.close()
        print("device call %d: %.1f ms (inside the library %.1f ms)" % (rep, dt, stats["elapsed_ms"]), file=sys.stderr, flush=True)
    out = dict(k=a.k, L=a.L, features=a.features, images=a.images, seed=a.seed, repeats=a.repeats, small_limit=stats["small_limit"],
               device_ms=float(np.median(times)), device_spread_ms=float(max(times) - min(times)), device_ms_all=[round(t, 2) for t in times],
               nodes=stats["nodes"], words=stats["words"], launches=stats["launches"],
               level_launches=stats["level_launches"][:a.L], level_max_iterations=stats["level_max_iterations"][:a.L], level_nodes=stats["level_nodes"][:a.L],
               level_small_nodes=stats["level_small_nodes"][:a.L], level_large_nodes=stats["level_large_nodes"][:a.L],
               capped_nodes=stats["capped_nodes"], host_one_core_ms=None, equal_to_host=None)
    if not a.no_host:
        tmp = tempfile.mkdtemp(prefix="voc_train_rate")
        H = build_partner(tmp)
        cap = stats["nodes"] + 16
        p = np.zeros(cap, np.int32); lf = np.zeros(cap, np.int32); d = np.zeros((cap, 32), np.uint8); w = np.zeros(cap, np.float64); n = C.c_int(0)
        t0 = time.perf_counter()
        rc = H.vt_host_train(corb._p(desc), corb._p(off), a.images, a.k, a.L, a.seed, 100, corb._p(p), corb._p(lf), corb._p(d), corb._p(w), cap, C.byref(n))
        out["host_one_core_ms"] = (time.perf_counter() - t0) * 1e3
        m = n.value
        out["equal_to_host"] = bool(rc == 0 and m == len(flat["parent"]) and np.array_equal(p[:m], flat["parent"]) and np.array_equal(lf[:m], flat["is_leaf"]) and
                                    np.array_equal(d[:m], flat["descriptor"]) and np.array_equal(w[:m].view(np.uint64), flat["weight"].view(np.uint64)))
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as o:
        json.dump(out, o, indent=1); o.write("\n")
    print(json.dumps(out))
    assert a.no_host or out["equal_to_host"], "the device's vocabulary differs from the host function's"


if __name__ == "__main__":
    main()

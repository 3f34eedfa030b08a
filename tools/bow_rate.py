"""Host-to-host times of place recognition on the device beside the serial host code of csrc/bow_math.h (tests/host/bow_main.cpp built -O3, the same machine):
  transform : KeyFrameStore.compute_bow for 1 and 8 slots of n = 2000 features on a synthetic full k = 10, L = 6 vocabulary (1.1 M nodes), against today's route for
              the same slots in the same process -- corb_kf_store_get of the descriptors alone, the host transform, corb_kf_store_set_bow;
  queries   : one query of each kind at 1 000, 10 000 and 50 000 live entries of 1 500 words, against the host emulation.
The host code is loaded into this process as a shared object.  Medians of five repeats after a warm-up, with max - min as the spread; then the same calls once more under
corb_bow_profile for the kernel shares and the cost of the two in-order sums.  Prints one JSON line.    python tools/bow_rate.py [--entries 1000,10000,50000] [--repeats 5]"""
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


def full_vocab(k, L, seed=1):
    r = np.random.default_rng(seed)
    parent, start, count = [], 0, 1
    for _ in range(L):                                                     # level by level: the parents of a level are the nodes of the one above
        parent.append(np.repeat(np.arange(start, start + count), k)); start += count; count *= k
    parent = np.concatenate(parent).astype(np.int32); n = len(parent)
    leaf = np.zeros(n, np.int32); leaf[n - k ** L:] = 1
    desc = r.integers(0, 256, (n, 32), dtype=np.uint8)
    weight = np.where(leaf > 0, np.exp(r.uniform(-2, 2.5, n)), 0.0)
    return dict(k=k, L=L, parent=parent, is_leaf=leaf, descriptor=desc, weight=weight)


def build_partner(tmp):
    """tests/host/bow_main.cpp's serial code as a shared object, -O3, loaded into this process"""
    so = os.path.join(tmp, "libbow_host.so")
    subprocess.run([shutil.which("g++") or "c++", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DBOW_HOST_SHARED", "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"),
                    "-I", os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "tests", "host", "bow_main.cpp"), "-o", so], check=True)
    H = C.CDLL(so)
    H.bow_host_create.restype = C.c_void_p
    H.bow_host_create.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
    H.bow_host_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    H.bow_host_db_create.argtypes = [C.c_void_p, C.c_int]
    H.bow_host_db_set_add.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    H.bow_host_db_detect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_float, C.c_void_p, C.c_int]
    H.bow_host_destroy.argtypes = [C.c_void_p]
    return H


def median_ms(fn, repeats, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(repeats):
        a = time.perf_counter(); fn(); t.append((time.perf_counter() - a) * 1e3)
    return float(np.median(t)), float(max(t) - min(t))


def shares(corb):
    return dict((k, dict(ms=round(v[0], 4), launches=v[1])) for k, v in corb.bow_profile_read().items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", default="1000,10000,50000"); ap.add_argument("--repeats", type=int, default=5); ap.add_argument("--features", type=int, default=2000)
    a = ap.parse_args()
    corb = corbload.load_pkg()
    tmp = tempfile.mkdtemp(prefix="bow_rate")
    H = build_partner(tmp)
    f = full_vocab(10, 6)
    voc = corb.Vocabulary(f["k"], f["L"], f["parent"], f["is_leaf"], f["descriptor"], f["weight"])
    hv = H.bow_host_create(f["k"], f["L"], len(f["parent"]), corb._p(f["parent"]), corb._p(f["is_leaf"]), corb._p(f["descriptor"]), corb._p(f["weight"]))
    r = np.random.default_rng(2)
    out = dict(vocabulary=voc.info(), repeats=a.repeats, transform={}, queries={})
    L = corb.load()

    # ---- transform ----
    n = a.features
    st = corb.KeyFrameStore(8, n)
    first_leaf = len(f["parent"]) - 10 ** 6
    for s in range(8):
        d = f["descriptor"][r.integers(first_leaf, len(f["parent"]), n)].copy()      # leaves' descriptors with one flipped bit each: words repeat
        d[np.arange(n), r.integers(0, 32, n)] ^= np.uint8(1) << r.integers(0, 8, n).astype(np.uint8)
        st.put(s, np.zeros(n, corb.KP_DTYPE), d)
    desc = np.zeros((n, 32), np.uint8); node = np.zeros(n, np.uint32); off = np.zeros(n + 1, np.int32); idx = np.zeros(n, np.uint32); cnt = C.c_int(0)
    parts = dict(get=0.0, host=0.0, set=0.0)

    def today(slots):                                                      # today's route, all of it in this process
        for s in range(slots):
            t0 = time.perf_counter()
            rc = L.corb_kf_store_get(st.h, s, None, corb._p(desc), None, None, None, n, C.byref(cnt), None, None, None, None, None)      # the descriptors alone
            t1 = time.perf_counter()
            k = H.bow_host_transform(hv, corb._p(desc), cnt.value, 4, corb._p(node), corb._p(off), corb._p(idx))
            t2 = time.perf_counter()
            st.set_bow(s, (node[:k], off[:k + 1], idx[:off[k]]))
            t3 = time.perf_counter()
            assert rc == 0
            parts["get"] += t1 - t0; parts["host"] += t2 - t1; parts["set"] += t3 - t2
    for slots in (1, 8):
        dev, dev_spread = median_ms(lambda: st.compute_bow(list(range(slots)), voc, 4), a.repeats)
        got = [st.get(s)["fv"] for s in range(slots)]
        for k_ in parts:
            parts[k_] = 0.0
        tod, tod_spread = median_ms(lambda: today(slots), a.repeats)
        calls = (a.repeats + 2) * 1e-3
        for s in range(slots):                                             # both routes leave the same FeatureVector
            assert all(np.array_equal(x, y) for x, y in zip(got[s], st.get(s)["fv"]))
        corb.bow_profile(1)
        for _ in range(a.repeats):
            st.compute_bow(list(range(slots)), voc, 4)
        sh = shares(corb); corb.bow_profile(0)
        out["transform"]["%d_slots" % slots] = dict(compute_bow_ms=dev, spread_ms=dev_spread, today_ms=tod, today_spread_ms=tod_spread,
                                                    today_parts_ms=dict((k_, v / calls) for k_, v in parts.items()), profiled_calls=a.repeats, kernels=sh)

    # ---- queries ----
    n_words = voc.info()["n_words"]
    cand = np.zeros(64, np.int32)
    for n_e in [int(x) for x in a.entries.split(",") if x]:
        places = max(1, n_e // 50)
        pools = [np.sort(r.choice(n_words, 3000, replace=False)).astype(np.uint32) for _ in range(places)]
        db = corb.KeyFrameDatabase(voc, n_e + 1, 1600)
        H.bow_host_db_create(hv, n_e + 1)
        for e in range(n_e + 1):
            w = np.sort(r.choice(pools[e % places], 1500, replace=False)).astype(np.uint32); v = r.random(1500) + 0.01; v /= v.sum()
            db.set_bow(e, w, v); H.bow_host_db_set_add(hv, e, corb._p(w), corb._p(v), 1500, int(e < n_e))
            if e < n_e:
                db.add(e)
        res = {}
        qid = [10]
        for kind, name in enumerate(("loop", "relocalisation", "map_fusion")):
            def q():
                qid[0] += 1                                                # a new id every call: a repeated id would push nothing
                return db.detect(kind, n_e, qid[0], (), 0.0)

            def hq():
                qid[0] += 1
                return H.bow_host_db_detect(hv, kind, n_e, qid[0], 0.0, corb._p(cand), 64)
            dev, spread = median_ms(q, a.repeats)
            host, hspread = median_ms(hq, a.repeats)
            qid[0] += 1
            same = db.detect(kind, n_e, qid[0], (), 0.0).tolist()
            nh = H.bow_host_db_detect(hv, kind, n_e, qid[0], 0.0, corb._p(cand), 64)
            corb.bow_profile(1)
            for _ in range(a.repeats):
                q()
            sh = shares(corb); corb.bow_profile(0)
            res[name] = dict(device_ms=dev, spread_ms=spread, host_ms=host, host_spread_ms=hspread, candidates=len(same), same_as_host=bool(nh == len(same) and cand[:min(nh, 64)].tolist() == same[:64]),
                             profiled_calls=a.repeats, kernels=sh)
        out["queries"][str(n_e)] = res
        db.close()
    print(json.dumps(out))
    H.bow_host_destroy(hv)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

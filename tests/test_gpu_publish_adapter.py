"""GPU test: the adapter's MapPublishT (corb-slam_amd/host/corb_adapter_orbslam.hpp), compiled with g++ -Wall -Werror and driven by
tests/host/publish_adapter_main.cpp on the test doubles, files a server map and a client map through MapStoreT, packs the server's four sets of light handles with
transMs and applies the message on the client; it prints what the definition (tests/publish_reference.py) gives for the same maps."""
import os
import struct
import subprocess

import numpy as np
import pytest

import publish_cases as G
import publish_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _sets(c):
    """the four sets of the server's cache: unique ids in ascending order (std::set<LightKeyFrame>), each resolved to the lowest server slot that holds the id"""
    s = c["server"]; p = c["pack"]
    kf_slot = {}; mp_slot = {}
    for k, r in enumerate(s["kfs"]):
        kf_slot.setdefault(int(r["id"]), k)
    for k, r in enumerate(s["mps"]):
        mp_slot.setdefault(int(r["id"]), k)
    ids = lambda recs, slots: sorted({int(recs[q]["id"]) for q in slots})
    A, C = ids(s["kfs"], p["new_kf_slots"]), ids(s["kfs"], p["upd_kf_slots"]); B, D = ids(s["mps"], p["new_mp_slots"]), ids(s["mps"], p["upd_mp_slots"])
    return (A, B, C, D), ([kf_slot[i] for i in A], [kf_slot[i] for i in C], [mp_slot[i] for i in B], [mp_slot[i] for i in D])


def test_adapter_publishes_a_small_map(tmp_path, corb):
    exe = tmp_path / "publish_adapter_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           "-I", os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "tests", "host", "publish_adapter_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    c = G.case("f64"); s = c["server"]
    one = lambda k: dict(k, kp=np.zeros(1, G.KP_DTYPE)) if len(k["kp"]) == 0 else k           # (every keyframe of the doubles has a feature)
    cl = dict(c["client"], kfs=[one(k) for k in c["client"]["kfs"]])
    (A, B, C, D), (a_slots, c_slots, b_slots, d_slots) = _sets(c)
    trans = sorted(c["pack"]["trans"], key=lambda t: t[0])                                  # std::map<int, cv::Mat> iterates by client id
    fin = tmp_path / "in.bin"
    with open(fin, "wb") as o:
        o.write(struct.pack("<16i", c["F"], c["O"], cl["client_id"], len(s["kfs"]), len(s["mps"]), len(cl["kfs"]), len(cl["mps"]), cl["kf_n"], cl["kf_room"], cl["mp_n"], cl["mp_room"],
                            len(A), len(B), len(C), len(D), len(trans)))
        for k in s["kfs"] + cl["kfs"]:
            o.write(struct.pack("<Q3i", int(k["id"]), int(k["client_id"]), int(bool(k["kf_flags"] & R.KF_FIXED)), len(k["kp"]))); o.write(np.asarray(k["Tcw"], np.float32).tobytes())
        for p in s["mps"] + cl["mps"]:
            o.write(struct.pack("<Q2i", int(p["id"]), int(p["client_id"]), int(bool(p["flags"] & R.MP_FIXED)))); o.write(np.asarray(p["world_pos"], np.float32).tobytes())
        for ids in (A, B, C, D):
            o.write(np.asarray(ids, np.uint64).tobytes())
        for cid, T in trans:
            o.write(struct.pack("<i", cid)); o.write(np.asarray(T, np.float32).tobytes())
    got = subprocess.check_output([str(exe), str(fin)]).decode().split("\n")[:-1]

    # the definition on the same maps: the flags the doubles carry are the fixed bits only (the case's bad flags do not travel through the doubles)
    strip = lambda recs, key, bit: [dict(r, **{key: int(r[key]) & bit}) for r in recs]
    skfs, smps = strip(s["kfs"], "kf_flags", R.KF_FIXED), strip(s["mps"], "flags", R.MP_FIXED)
    cl2 = dict(cl, kfs=strip(cl["kfs"], "kf_flags", R.KF_FIXED), mps=strip(cl["mps"], "flags", R.MP_FIXED))
    msg = R.pack(skfs, a_slots, c_slots, smps, b_slots, d_slots, trans)
    w, after = R.apply(msg, cl2)
    assert w["n_kf_inserted"] >= 3 and w["n_mp_inserted"] >= 8 and w["n_kf_updated"] >= 3 and not w["capacity_error"]
    num = lambda a: " ".join(str(int(v)) for v in a)
    want = ["counts %d %d %d %d %d" % (len(A), len(B), len(C), len(D), len(trans)),
            "applied %d %d %d %d | %s | %s | %s | %s | %s | %s" % (w["n_kf_updated"], w["n_mp_updated"], w["no_transform"], int(w["capacity_error"]), num(w["kind_kf_new"]), num(w["kind_mp_new"]),
                                                                  num(w["kind_kf_upd"]), num(w["kind_mp_upd"]), num(w["kf_new_slots"]), num(w["mp_new_slots"]))]
    for k, r in enumerate(after["kfs"][: len(cl["kfs"])]):
        want.append("kf %d %d %d %d %s" % (k, r["id"], r["client_id"], r["kf_flags"], " ".join("%08x" % v for v in np.asarray(r["Tcw"], np.float32).reshape(-1).view(np.uint32))))
    for k, r in enumerate(after["mps"][: len(cl["mps"])]):
        want.append("mp %d %d %d %d %s" % (k, r["id"], r["client_id"], r["flags"], " ".join("%08x" % v for v in np.asarray(r["world_pos"], np.float32).view(np.uint32))))
    assert [" ".join(g.split()) for g in got] == [" ".join(x.split()) for x in want]

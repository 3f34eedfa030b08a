"""GPU test: the adapter's KeyFrameInsertT (corb-slam_amd/host/corb_adapter_orbslam.hpp), compiled with g++ -Wall -Werror and driven by
tests/host/kfinsert_adapter_main.cpp on the test doubles, files a map through MapStoreT and takes one keyframe through CreateStereoPoints, ProcessNewKeyFrame,
MapPointCulling and the NeedNewKeyFrame counts; it prints what the definition (tests/kfinsert_reference.py) gives for the same map."""
import os
import struct
import subprocess

import numpy as np
import pytest

import kfinsert_reference as R
import kfinsert_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def write_scene(o, sc, n_mp, slot, mode, kf_first, kf_n, extra, th_depth, scale_factor, first_mp_id, cur_kf_id):
    cam = sc["cam"]
    o.write(struct.pack("<9i2f2Q", len(sc["kfs"]), n_mp, sc["F"], sc["O"], slot, mode, kf_first, kf_n, len(extra), th_depth, scale_factor, first_mp_id, cur_kf_id))
    o.write(np.array([cam[f] for f in ("fx", "fy", "cx", "cy", "bf", "mb")] + list(cam["scale"][:8]), np.float32).tobytes())
    for k in sc["kfs"]:
        n = len(k["kp"])
        o.write(struct.pack("<Qi", int(k["id"]), n)); o.write(np.asarray(k["Tcw"], np.float32).tobytes())
        for a in (k["kp"]["x"], k["kp"]["y"], k["kp"]["octave"].astype(np.int32), k["u_right"], k["depth"], k["mp_id"], k["desc"]):
            o.write(np.ascontiguousarray(a).tobytes())
    for p in sc["mps"][:n_mp]:
        o.write(struct.pack("<2Q4iq", int(p["id"]), int(p["ref_kf_id"]), int(p["flags"] & R.MP_BAD), len(p["obs"]), int(p["n_found"]), int(p["n_visible"]), int(p["scratch"].get("first_kf_id", 0))))
        o.write(np.asarray(p["world_pos"], np.float32).tobytes())
        for kid, idx in p["obs"]:
            o.write(struct.pack("<QI", int(kid), int(idx)))
    o.write(np.asarray(extra, np.int32).tobytes())


def test_adapter_takes_one_keyframe_through_the_calls(tmp_path, corb):
    exe = tmp_path / "kfinsert_adapter_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           "-I", os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "tests", "host", "kfinsert_adapter_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    sc, a = G.assoc_case("n257")
    n_mp = sum(p is not None for p in sc["mps"])
    sc["mps"] = sc["mps"][:n_mp] + [None] * sc["F"]
    for k in sc["kfs"]:
        k["flags"][:] = 0                                           # MapStoreT::PutKeyFrame files no feature flags
    slot, first, n = a["slot"], a["kf_first"], a["kf_n"]
    extra = list(range(0, n_mp, 3)); cur_kf_id = int(sc["kfs"][slot]["id"]) + 1
    for s in extra[::4]:
        sc["mps"][s]["n_found"], sc["mps"][s]["n_visible"] = 1, 5      # rarely found: culled by the ratio
    fin = tmp_path / "in.bin"
    with open(fin, "wb") as o:
        write_scene(o, sc, n_mp, slot, 1, first, n, extra, 15.0, 1.2, 70000, cur_kf_id)
    got = subprocess.check_output([str(exe), str(fin)]).decode().split("\n")[:-1]

    w1, sc = R.create_stereo_points(sc, slot, 15.0, 1, True, first_mp_slot=n_mp, first_mp_id=70000, client_id=1, frame_id=77)
    R.build_index(sc, 0, n_mp + w1["n_created"])
    w3, sc = R.process_new_keyframe(sc, slot, first, n, 1.2, True)
    recent = extra + w3["recent_slots"].tolist()
    w4, sc = R.map_point_culling(sc, recent, cur_kf_id, 3, first, n, True)
    counts = R.need_keyframe_counts(sc, slot, 15.0, slot, 3, first, n)
    assert 100 < w1["n_visited"] < 257 and w1["n_created"] > 8 and w3["n_added"] > 8 and len(set(w4["decision"].tolist())) == 5
    want = ["points %d %d %s" % (w1["n_visited"], w1["n_created"], " ".join(["%d:%d" % (i, k) for i, k in zip(w1["order"], w1["kind"])] + ["%08x" % v for v in w1["x3d"].reshape(-1).view(np.uint32)])),
            "assoc %d %d %s" % (w3["n_added"], len(w3["recent_slots"]), " ".join([str(k) for k in w3["kind"]] + [str(s) for s in w3["recent_slots"]])),
            "cull %d %d %s" % (len(recent), len(w4["kept_slots"]), " ".join([str(d) for d in w4["decision"]] + [str(s) for s in w4["kept_slots"]])),
            "counts %d %d %d" % counts]
    assert [g.strip() for g in got] == [w.strip() for w in want]

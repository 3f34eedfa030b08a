"""GPU test: the spanning-tree methods and UpdateLocalMap of the adapter's corb::Covisibility<KeyFrame, Db> (corb-slam_amd/host/corb_adapter_orbslam.hpp), compiled with
g++ -Wall -Werror and driven by tests/host/localmap_adapter_main.cpp on test doubles, answer what tests/localmap_reference.py answers on one scripted session over a
seeded map: the tree UpdateConnections grows, the tree calls, UpdateLocalMap before and after keyframes are culled through EraseConnections + ReparentChildren."""
import os
import struct
import subprocess
import numpy as np
import pytest

import covis_reference as R
import covis_cases as G
import localmap_cases as C
import localmap_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_adapter_tree_and_local_map_match_the_reference_restatement(tmp_path, corb):
    exe = tmp_path / "localmap_adapter_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "localmap_adapter_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    kw, frames = C.LOCALMAP_CASES["k20"]
    m = G.random_map(**kw)
    seed, n, first, width, extra = frames[0]
    frame = C.frame_for(m, seed, n, first, width, **extra)
    order = list(m.kfs)
    m.kfs[C.FRAME_ID] = R.KeyFrame(C.FRAME_ID, frame.mp_ids)      # the frame's record is the last slot of the store; it is no keyframe of the map
    a = G.arrays(m, order + [C.FRAME_ID])
    del m.kfs[C.FRAME_ID]
    slot = {k: s for s, k in enumerate(order)}; mp_slot = {int(p): s for s, p in enumerate(a["mp_ids"])}
    ids = sorted(m.kfs)
    ops, want = [], []
    state = dict(local=[], ref=None)

    def tree_of(k, other):
        p, _, c = LR.get_tree(m, k)
        held = [x for x in c if x in m.kfs]
        ops.append((2, slot[k], slot[other], 0))
        want.append("T %d %d %d" % (slot[p] if p in m.kfs else -1, int(other in c), len(held)) + "".join(" %d" % slot[x] for x in held))

    def local_map():
        r = LR.update_local_map(m, frame, state["local"])
        state["local"] = r["kfs"]; state["ref"] = r["ref"] if r["ref"] is not None else state["ref"]
        ops.append((6, 0, 0, 0))
        want.append("M %d %d %d %d %d %d" % (len(r["kfs"]), len(r["mps"]), r["n_voted"], -1 if state["ref"] is None else slot[state["ref"]], int(r["counter_empty"]), r["n_cleared"])
                    + "".join(" %d" % slot[k] for k in r["kfs"]) + "".join(" %d" % mp_slot[p] for p in r["mps"]))

    def frame_store_forms():
        """FrameStoreT::UpdateLocalMap on slots, then its ids through FrameStoreT::SearchLocalPoints: this map has no geometry, so nothing is in view (0 0)"""
        r = LR.update_local_map(m, frame, state["local"])
        ops.append((7, 0, 0, 0))
        want.append("F %d %d %d %d %d 0 0" % (len(r["kfs"]), len(r["mps"]), r["n_voted"], -1 if r["ref"] is None else slot[r["ref"]], int(r["counter_empty"]))
                    + "".join(" %d" % slot[k] for k in r["kfs"]) + "".join(" %d" % mp_slot[p] for p in r["mps"]))

    for k in ids:
        ops.append((0, slot[k], 0, 0))
        f = LR.update_connections(m, k)
        want.append("U %d" % (-1 if f is None else slot[f]))
    for k in ids[::3]:
        tree_of(k, ids[4])
    local_map()
    frame_store_forms()
    for code, fn, k, o in ((3, LR.add_child, ids[2], ids[9]), (5, LR.change_parent, ids[5], ids[2]), (4, LR.erase_child, ids[4], ids[5]), (3, LR.add_child, ids[2], ids[9])):
        ops.append((code, slot[k], slot[o], 0)); fn(m, k, o)
    for k in (ids[2], ids[4], ids[5]):
        tree_of(k, ids[9])
    for k in C.culling_sequence(m, 5, 4):
        ops.append((1, slot[k], 0, 0))
        want.append("R %d %d" % tuple(int(x) for x in C.set_bad_flag(m, k)))
        local_map()
    frame_store_forms()
    for k in ids[::2]:
        tree_of(k, ids[5])
    F = int(np.diff(a["feat_off"]).max())
    blob = [struct.pack("<6i", len(order) + 1, F, len(a["mp_ids"]), 12, 0, len(ops)),
            a["kf_ids"].tobytes(), a["kf_bad"].astype("<u4").tobytes(), a["feat_off"].tobytes(), a["octave"].tobytes(), a["u_right"].tobytes(), a["depth"].tobytes(),
            a["mp_id"].tobytes(), a["mp_ids"].tobytes(), a["mp_bad"].astype("<u4").tobytes(), a["obs_off"].tobytes(), a["obs_kf"].tobytes(), a["obs_idx"].tobytes()]
    blob += [struct.pack("<4i", *op) for op in ops]
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    got = subprocess.check_output([str(exe), str(tmp_path / "in.bin")]).decode().split("\n")[:-1]
    assert len(got) == len(want) and len(want) > 40
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)

"""GPU test: AddLoopEdge, GetLoopEdges and OptimizeEssentialGraph of the adapter's corb::Covisibility<KeyFrame, Db> (corb-slam_amd/host/corb_adapter_orbslam.hpp),
compiled with g++ -Wall -Werror and driven by tests/host/essgraph_adapter_main.cpp on test doubles, leave in the objects what tests/essgraph_reference.py leaves in
its map on a seeded case of tests/essgraph_cases.py.  The final estimates the definition commits are the ones the Python route returns for the same case (the call
is deterministic: tests/test_gpu_essgraph.py); poses and positions are then EQUAL, normal and distances keep the project's bar (2e-7 absolute, 2e-6 relative)."""
import copy
import os
import struct
import subprocess

import numpy as np
import pytest

import covis_cases as G
import essgraph_cases as EC
import essgraph_reference as ER
import essgraph_stores as ES
import localmap_reference as LR
import loopfix_reference as XR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NO_ID = XR.NO_ID


def floats(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)


def test_adapter_essential_graph_matches_the_definition(tmp_path, corb):
    exe = tmp_path / "essgraph_adapter_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           "-I", os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "tests", "host", "essgraph_adapter_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    seed, min_weight, fix_scale, scale = EC.SEEDS[3], 3, False, 1.2
    c = EC.seeded(seed)
    # an id no store holds cannot be bound to an object: the adapter's maps hold objects, so such a loop-connection member is left out of this case
    c.loop_connections = {k: {j for j in v if j in c.m.kfs} for k, v in c.loop_connections.items()}
    m = c.m
    d = ES.Dev(corb, c, seed); d.add_loop_edges()
    order, mp_order, slot = d.order, d.mp_order, d.slot
    a = G.arrays(m, order, mp_order)
    f32 = lambda x: np.ascontiguousarray(x, np.float32).tobytes()
    i32 = lambda *x: struct.pack("<%di" % len(x), *x)
    u64 = lambda x: np.array(x, np.uint64).tobytes()
    kf_flags = np.array([(1 if m.kfs[k].bad else 0) | (2 if m.kfs[k].fixed else 0) for k in order], "<u4")
    mp_flags = np.array([(1 if m.mps[p].bad else 0) | (2 if m.mps[p].fixed else 0) for p in mp_order], "<u4")
    blob = [i32(len(order), int(np.diff(a["feat_off"]).max()), len(mp_order), 8, 64, 3),
            a["kf_ids"].tobytes(), kf_flags.tobytes(), a["feat_off"].tobytes(), a["octave"].tobytes(), a["u_right"].tobytes(), a["depth"].tobytes(),
            a["mp_id"].tobytes(), a["mp_ids"].tobytes(), mp_flags.tobytes(), a["obs_off"].tobytes(), a["obs_kf"].tobytes(), a["obs_idx"].tobytes(),
            f32([m.kfs[k].Tcw for k in order])]
    for k in order:
        kf = LR.tree(m.kfs[k]); ch = sorted(kf.children); lo = sorted(kf.loop_edges, reverse=True)
        blob.append(struct.pack("<Qi", NO_ID if kf.parent is None else kf.parent, len(ch)) + u64(ch) + i32(len(lo), *[slot[l] for l in lo]))
    pts = [m.mps[p] for p in mp_order]
    blob += [f32([p.pos for p in pts]), f32([p.normal for p in pts]), f32([[p.min_distance, p.max_distance] for p in pts]),
             u64([NO_ID if p.ref_kf is None else p.ref_kf for p in pts]), u64([p.corrected_by for p in pts]), u64([p.corrected_ref for p in pts])]
    upd = [slot[k] for k in sorted(m.kfs)]
    blob += [i32(len(upd), *upd), i32(slot[c.loop_id], slot[c.cur_id], int(fix_scale), min_weight), struct.pack("<f", scale)]
    ks = sorted(c.corrected)
    blob += [i32(len(ks), *[slot[k] for k in ks]), np.array([c.corrected[k] for k in ks], np.float64).tobytes(), np.array([c.non_corrected[k] for k in ks], np.float64).tobytes()]
    blob.append(i32(len(c.loop_connections)))
    for k, v in c.loop_connections.items():
        blob.append(i32(slot[k], len(v), *[slot[j] for j in sorted(v)]))
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    got = subprocess.check_output([str(exe), str(tmp_path / "in.bin")]).decode().split("\n")[:-1]
    # the same call through the Python route gives the final estimates; the definition commits them
    want = ER.plan(m, **c.inputs(min_weight))
    out = d.g.OptimizeEssentialGraph(bFixScale=fix_scale, scale_factor=scale, **d.args(min_weight))
    d.close()
    old = copy.deepcopy(m)
    n, moved = ER.commit(m, want, out["S"], c.cur_id, 0.0)
    r = [int(x) for x in got[0].split()[1:]]
    cnt = want["counts"]
    assert got[0].startswith("R ") and r[:7] == [cnt["n_vertices"], cnt["n_edges"]] + cnt["n_kind"] + [cnt["n_dropped"]] and r[7] == out["result"].iters_done
    assert r[8:13] == [n[k] for k in ("n_poses_set", "n_points_moved", "n_points_kept", "n_points_skipped", "n_points_fixed_ref")]
    assert r[13:] == [n["n_poses_set"], n["n_points_moved"]] and n["n_points_moved"] > 20 and n["n_points_kept"] > 0      # addUpdateKeyframe / addUpdateMapPoint calls
    K = len(order)
    for s, k in enumerate(order):
        w = got[1 + s].split()
        assert w[0] == "L" and int(w[1]) == s and sorted(int(x) for x in w[2:]) == sorted(m.kfs[k].loop_edges)
        w = got[1 + K + s].split()
        assert w[0] == "K" and np.array_equal(floats(w[2:18]).reshape(4, 4), m.kfs[k].Tcw), k
        assert (not np.array_equal(m.kfs[k].Tcw, old.kfs[k].Tcw)) == (not m.kfs[k].bad and not m.kfs[k].fixed)
    for s, p in enumerate(mp_order):
        w = got[1 + 2 * K + s].split(); mp = m.mps[p]
        pos, normal, mm = floats(w[2:5]), floats(w[5:8]), floats(w[8:10])
        assert w[0] == "P" and np.array_equal(pos, mp.pos), (p, pos, mp.pos)
        if p in moved:
            probe = copy.copy(old.mps[p]); probe.pos = pos.copy()
            XR.update_normal_and_depth(m, probe, lambda k: m.kfs[k].Tcw, scale)
            for g_, w_ in ((normal, probe.normal), (mm, np.array([probe.min_distance, probe.max_distance]))):
                assert np.all(np.abs(np.asarray(g_, np.float64) - w_) <= 2e-7 + 2e-6 * np.abs(w_)), (p, g_, w_)
        else:
            assert np.array_equal(normal, old.mps[p].normal) and mm[0] == old.mps[p].min_distance and mm[1] == old.mps[p].max_distance

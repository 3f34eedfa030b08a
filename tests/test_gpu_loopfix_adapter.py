"""GPU test: CorrectLoop and PropagateGlobalBA of the adapter's corb::Covisibility<KeyFrame, Db> (corb-slam_amd/host/corb_adapter_orbslam.hpp), compiled with
g++ -Wall -Werror and driven by tests/host/loopfix_adapter_main.cpp on test doubles, leave in the objects what tests/loopfix_reference.py leaves in its map on one
scripted loop event over a seeded map: the connections, the correction, then the spread of a global bundle adjustment.  The arithmetic is held to its bars by
tests/test_gpu_loopfix.py; here the second call runs on the first one's rounded results, so floats are compared to 1e-5 and everything else exactly."""
import os
import struct
import subprocess

import numpy as np
import pytest

import covis_cases as G
import localmap_reference as LR
import loopfix_cases as C
import loopfix_reference as XR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NO_ID = XR.NO_ID


def floats(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)


def close(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= 1e-5 * np.maximum(1.0, np.abs(b).max()))


def test_adapter_loop_event_matches_the_reference_restatement(tmp_path, corb):
    exe = tmp_path / "loopfix_adapter_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           "-I", os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "tests", "host", "loopfix_adapter_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(5)
    m, cur = C.loop_map(C.LOOP_SEEDS[0], cur="middle")
    ids = sorted(m.kfs); order = [ids[i] for i in rng.permutation(len(ids))]; mp_order = sorted(m.mps)
    slot = {k: s for s, k in enumerate(order)}
    # the tree: a chain over the ids with one keyframe listed twice; the last three keyframes were not seen by the global BA; some keyframes carry a stored mTcwBefGBA
    for a, k in enumerate(ids):
        kf = XR.pose(m.kfs[k])
        LR.set_tree(m, k, ids[a - 1] if a else None, False, ids[a + 1: a + 2])
        kf.TcwGBA = C.random_pose(rng); kf.ba_global = C.LOOP_KF if a < len(ids) - 3 else 0
        if a % 4 == 1:
            kf.TcwBef = C.random_pose(rng)
    m.kfs[ids[2]].children.add(ids[5]); m.kfs[ids[1]].children.add(880000001)
    for p in mp_order:
        mp = m.mps[p]; mp.pos_gba = (rng.normal(size=3) * 4).astype(np.float32); mp.ba_global = C.LOOP_KF if rng.random() < 0.4 else 0
    a = G.arrays(m, order, mp_order)
    Scw = C.loop_scw(m, cur, 3, 0.8)
    f32 = lambda x: np.ascontiguousarray(x, np.float32).tobytes()
    blob = [struct.pack("<6i", len(order), int(np.diff(a["feat_off"]).max()), len(mp_order), 8, 64, 3),
            a["kf_ids"].tobytes(), a["kf_bad"].astype("<u4").tobytes(), a["feat_off"].tobytes(), a["octave"].tobytes(), a["u_right"].tobytes(), a["depth"].tobytes(),
            a["mp_id"].tobytes(), a["mp_ids"].tobytes(), a["mp_bad"].astype("<u4").tobytes(), a["obs_off"].tobytes(), a["obs_kf"].tobytes(), a["obs_idx"].tobytes(),
            f32([m.kfs[k].Tcw for k in order]), f32([m.kfs[k].TcwGBA for k in order]), f32([m.kfs[k].TcwBef for k in order]),
            np.array([m.kfs[k].ba_global for k in order], np.uint64).tobytes()]
    for k in order:
        kf = m.kfs[k]; ch = sorted(kf.children)
        blob.append(struct.pack("<Qi", NO_ID if kf.parent is None else kf.parent, len(ch)) + np.array(ch, np.uint64).tobytes())
    blob += [f32([m.mps[p].pos for p in mp_order]), f32([m.mps[p].pos_gba for p in mp_order]), np.array([m.mps[p].ba_global for p in mp_order], np.uint64).tobytes(),
             np.array([NO_ID if m.mps[p].ref_kf is None else m.mps[p].ref_kf for p in mp_order], np.uint64).tobytes(),
             np.array([m.mps[p].corrected_by for p in mp_order], np.uint64).tobytes()]
    op = lambda code, x, slots, v=np.zeros(8), scale=0.0: struct.pack("<4i", code, x, len(slots), 0) + np.asarray(v, np.float64).tobytes() + struct.pack("<f", scale) + np.array(slots, np.int32).tobytes()
    blob += [op(0, 3, [slot[k] for k in ids]), op(1, slot[cur], [], Scw, 1.2), op(2, C.LOOP_KF, [slot[ids[0]]])]
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    got = subprocess.check_output([str(exe), str(tmp_path / "in.bin")]).decode().split("\n")[:-1]
    # the same event on the definition
    before = {p: (m.mps[p].corrected_by, m.mps[p].corrected_ref) for p in mp_order}
    walk, co, nc, n_points = XR.correct_loop(m, cur, Scw, 1.2)
    r = XR.gba_propagate(m, [ids[0]], C.LOOP_KF, XR.default_queue_cap(len(order)), point_ids=mp_order)
    line = got[0].split()
    assert line[0] == "C" and [int(x) for x in line[1:5]] == [len(walk), n_points, len(walk), n_points] and [int(x) for x in line[5:]] == [slot[k] for k in walk]
    for i, k in enumerate(walk):
        v = np.array([float(x) for x in got[1 + i].split()[1:]])
        assert np.abs(v[:8] - co[i]).max() <= 1e-12 * max(1.0, np.abs(co[i]).max()) and np.abs(v[8:] - nc[i]).max() <= 1e-12 * max(1.0, np.abs(nc[i]).max())
    gl = got[1 + len(walk)].split()
    assert gl[0] == "G" and [int(x) for x in gl[1:8]] == [r[k] for k in ("n_popped", "n_reached", "n_propagated", "n_revisited", "n_points_set", "n_points_moved", "n_points_skipped")]
    assert [int(x) for x in gl[8:]] == [r["n_reached"], r["n_points_set"] + r["n_points_moved"]] and r["n_revisited"] > 0 and r["n_propagated"] == 3
    rest = got[2 + len(walk):]
    assert len(rest) == len(order) + len(mp_order)
    for s, k in enumerate(order):
        w = rest[s].split(); kf = m.kfs[k]
        assert w[0] == "K" and int(w[1]) == s and int(w[2]) == kf.ba_global
        T = floats(w[3:51]).reshape(3, 4, 4)
        assert close(T[0], kf.Tcw) and close(T[1], kf.TcwGBA) and close(T[2], kf.TcwBef), (k, T, kf.Tcw, kf.TcwGBA, kf.TcwBef)
    moved = 0
    for s, p in enumerate(mp_order):
        w = rest[len(order) + s].split(); mp = m.mps[p]
        assert w[0] == "P" and (int(w[2]), int(w[3])) == (mp.corrected_by, mp.corrected_ref if (mp.corrected_by, mp.corrected_ref) != before[p] else 0)
        assert close(floats(w[4:7]), mp.pos), (p, floats(w[4:7]), mp.pos)
        if (mp.corrected_by, mp.corrected_ref) != before[p]:
            moved += 1
            assert close(floats(w[7:10]), mp.normal) and close(floats(w[10:12]), [mp.min_distance, mp.max_distance])
    assert moved == n_points > 20

"""GPU test: the adapter's corb::Sim3Solver<KeyFrame, MapPoint> (corb-slam_amd/host/corb_adapter_orbslam.hpp), compiled with g++ and driven by
tests/host/sim3solver_main.cpp on test doubles, returns the iterate(5) sequence of the Python class for the same keyframes, matches and draws."""
import os
import subprocess
import numpy as np
import pytest
import sim3solver_reference as R
import gpu_sim3_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_adapter_sim3solver_matches_the_python_class(tmp_path, corb):
    exe = tmp_path / "sim3solver_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "sim3solver_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    sc = G.record_scene(); kf1, kf2 = sc["kf1"], sc["kfs2"][1]; n1, n2 = len(kf1["mp_id"]), len(kf2["mp_id"]); chunk, min_inliers = 5, 20
    sigma2 = (sc["scale"] * sc["scale"]).astype(np.float32)
    # the scene in the doubles' terms: KF1's point at feature i observes KF1 at index_kf1[i]; vpMatched12[i] = KF2's point at feature matched[i]
    pts = sc["points"]; id2 = {int(v): j for j, v in enumerate(kf2["mp_id"])}
    blob = [np.array([n1, n2, 0, min_inliers, chunk], np.int32).tobytes(), np.asarray(kf1["Tcw"], np.float32).tobytes(), np.asarray(kf2["Tcw"], np.float32).tobytes(),
            np.array(kf1["K"], np.float32).tobytes(), np.array(kf2["K"], np.float32).tobytes(), sigma2.tobytes()]
    points = {}; matched_ids = np.full(n1, R.NO_MAP_POINT, np.uint64); mp_id1 = np.arange(1000, 1000 + n1).astype(np.uint64)
    for i in range(n1):
        p = pts[1000 + i]; m = int(sc["matched"][1][i]); j = id2.get(m, -1)
        blob += [np.asarray(p["pos"], np.float32).tobytes(), np.array([kf1["octave"][i], p["obs"].get(11, -1), j, int(p["bad"])], np.int32).tobytes()]
        points[1000 + i] = p
        if j >= 0:
            matched_ids[i] = m
    for j in range(n2):
        p = pts[int(kf2["mp_id"][j])]
        blob += [np.asarray(p["pos"], np.float32).tobytes(), np.array([kf2["octave"][j], int(p["bad"])], np.int32).tobytes()]
        points[int(kf2["mp_id"][j])] = dict(pos=p["pos"], bad=p["bad"], obs={kf2["id"]: j})
    rv = sc["rand"][1]
    blob.append(np.ascontiguousarray(rv, np.int32).tobytes())
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    lines = subprocess.check_output([str(exe), str(tmp_path / "in.bin")]).decode().strip().split("\n")
    # the Python class on what the constructor leaves for the same scene
    pr, idx1 = R.constructor(dict(kf1, mp_id=mp_id1), kf2, points, matched_ids, sc["scale"], sc["scale"])
    s = corb.Sim3Solver(pr["x1"], pr["x2"], pr["sigma2_1"], pr["sigma2_2"], pr["K1"], pr["K2"], indices1=idx1, n1=n1, rand_values=rv)
    s.SetRansacParameters(0.99, min_inliers, 300)
    n_found = 0
    for line in lines:
        T, bNoMore, vb, n = s.iterate(chunk)
        head, mat = line.split("|")[0].split(), line.split("|")[1].split()
        assert [int(v) for v in head[:3]] == [int(T is not None), int(bNoMore), n]
        assert [int(v) for v in head[3:]] == np.nonzero(vb)[0].tolist()
        if T is not None:
            n_found += 1
            assert np.array_equal(np.array([float.fromhex(v) for v in mat], np.float32).view(np.uint32), T.reshape(-1).view(np.uint32))
            assert np.float32(float.fromhex(line.split("|")[2].strip())) == np.float32(s.GetEstimatedScale())
    assert bNoMore and n_found > 3 and len(lines) > n_found

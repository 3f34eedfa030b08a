"""GPU test: the adapter's corb::PnPsolver<Frame, KeyFrame, MapPoint> (corb-slam_amd/host/corb_adapter_orbslam.hpp), compiled with g++ and driven by
tests/host/pnpsolver_main.cpp on test doubles, returns the iterate(5) sequences of the Python class for the same frame, matches and draws -- all candidates evaluated by
one PnPsolver::RunBatch."""
import os
import subprocess
import numpy as np
import pytest
import pnpsolver_reference as R
import gpu_pnp_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_adapter_pnpsolver_matches_the_python_class(tmp_path, corb):
    exe = tmp_path / "pnpsolver_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "pnpsolver_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    sc = G.record_scene(); n = len(sc["kp"]); n_cand = 3; chunk, tail, n_calls = 5, sc["tail"], 4
    sigma2 = (sc["scale"] * sc["scale"]).astype(np.float32)
    blob = [np.array([n_cand, n, chunk, tail, n_calls], np.int32).tobytes(), np.array(sc["K"], np.float32).tobytes(), sigma2.tobytes()]
    for i in range(n):
        blob += [sc["kp"][i].astype(np.float32).tobytes(), np.array([sc["octave"][i]], np.int32).tobytes()]
    for c in range(n_cand):
        for i in range(n):
            p = sc["points"].get(int(sc["matched"][c][i]))
            blob += [np.asarray(p["pos"] if p else [0, 0, 0], np.float32).tobytes(), np.array([0 if p is None else (2 if p["bad"] else 1)], np.int32).tobytes()]
        blob.append(np.ascontiguousarray(sc["rand"][c], np.int32).tobytes())
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    lines = subprocess.check_output([str(exe), str(tmp_path / "in.bin")]).decode().strip().split("\n")
    assert len(lines) == n_cand * n_calls
    n_found = 0
    for c in range(n_cand):
        pr, idx = R.constructor(sc["kp"], sc["octave"], sc["matched"][c], sc["points"], sc["scale"], sc["K"])
        s = corb.PnPsolver(pr["p3dw"], pr["p2d"], pr["sigma2"], pr["K"], indices=idx, n_matches=n, rand_values=sc["rand"][c], tail_iterations=tail)
        s.SetRansacParameters(**{k: v for k, v in zip(("probability", "minInliers", "maxIterations", "minSet", "epsilon", "th2"), (0.99, 10, 300, 4, 0.5, 5.991))})
        for line in lines[c * n_calls: (c + 1) * n_calls]:
            T, bNoMore, vb, nInl = s.iterate(chunk)
            head, mat = line.split("|")[0].split(), line.split("|")[1].split()
            assert [int(v) for v in head[:4]] == [c, int(T is not None), int(bNoMore), nInl]
            assert [int(v) for v in head[4:]] == np.nonzero(vb)[0].tolist()
            if T is not None:
                n_found += 1
                assert np.array_equal(np.array([float.fromhex(v) for v in mat], np.float32).view(np.uint32), T.reshape(-1).view(np.uint32))
    assert n_found >= 4

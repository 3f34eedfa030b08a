"""GPU test: the adapter's corb::Initializer<Frame> (corb-slam_amd/host/corb_adapter_orbslam.hpp), compiled with g++ and driven by
tests/host/initializer_adapter_main.cpp on test doubles, returns what the Python Initializer class returns for the same frames, matches and draws -- through Initialize
on one pair and through one Initializer::RunBatch over three pairs, one of which fails."""
import os
import subprocess
import numpy as np
import pytest
import gpu_init_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_adapter_initializer_matches_the_python_class(tmp_path, corb):
    exe = tmp_path / "initializer_adapter_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "initializer_adapter_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    cases = [G.cases()[n] for n in ("general129", "planar65_ok", "rotation129")]; its = 200
    blob = [np.array([len(cases), its], np.int32).tobytes(), np.array(G.KITTI, np.float32).tobytes()]
    for c in cases:
        pr = c["problem"]
        blob += [np.array([len(pr["keys1"]), len(pr["keys2"])], np.int32).tobytes(), pr["keys1"].astype(np.float32).tobytes(), pr["keys2"].astype(np.float32).tobytes(),
                 pr["matches12"].astype(np.int32).tobytes(), np.ascontiguousarray(c["rand"], np.int32).tobytes()]
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    lines = subprocess.check_output([str(exe), str(tmp_path / "in.bin")]).decode().strip().split("\n")
    assert len(lines) == len(cases) + 1 and lines[0] == lines[1]                           # Initialize alone and within the batch
    n_ok = 0
    for line, c in zip(lines[1:], cases):
        pr = c["problem"]
        ini = corb.Initializer(pr["keys1"], pr["K"], sigma=1.0, iterations=its)
        ok, R21, t21, vP3D, vb = ini.Initialize(pr["keys2"], pr["matches12"], c["rand"])
        head, mot, pts = [x.split() for x in line.split("|")]
        assert [int(v) for v in head] == [cases.index(c), int(ok), int(ini.last["result"]["status"])]
        if not ok:
            assert not mot and not pts
            continue
        n_ok += 1
        got = np.array([float.fromhex(v) for v in mot], np.float32)
        assert np.array_equal(got.view(np.uint32), np.concatenate([R21.reshape(9), t21]).view(np.uint32))
        rows = np.array([[float.fromhex(v) if k else float(int(v)) for k, v in enumerate(pts[4 * i: 4 * i + 4])] for i in range(len(pts) // 4)], np.float32)
        assert len(rows) == len(pr["keys1"]) and np.array_equal(rows[:, 0].astype(bool), vb) and np.array_equal(rows[:, 1:].view(np.uint32), vP3D.view(np.uint32))
    assert n_ok == 2

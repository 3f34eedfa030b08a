"""GPU test: the C++ mirror's RgbdFrontend (corb-slam_amd/host/corb_host.hpp), driven by tests/host/rgbd_main.cpp, reproduces the Python one-call result"""
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cam_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_cpp_rgbd_frontend_reproduces_the_python_call(tmp_path, corb, synth):
    exe = tmp_path / "rgbd_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "rgbd_main.cpp"), "-o", str(exe), "-L", os.path.join(ROOT, "corb-slam_amd"),
                           "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    cam = R.TUM1
    fe = corb.RgbdFrontend(**{k: cam[k] for k in R.CAM_KEYS})
    packed = fe.pack_input([synth.rgbd_frame(7)])
    ref = fe.unpack_frame(fe.frames(packed))
    (tmp_path / "in.bin").write_bytes(packed.tobytes())
    args = [str(corb.SENSOR_RGBD), "3", "1", "640", "480", "1000"] + [repr(float(cam[k])) for k in R.CAM_KEYS] + [str(corb.DEPTH_U16)]
    out = subprocess.check_output([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")] + args).decode()
    b = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint8)
    n = int(b[:4].view(np.int32)[0])
    assert out.strip() == "n=%d" % n and n == len(ref["keys"]) > 500
    assert b[4:20].tobytes() == fe.bounds().tobytes()
    o = 20
    for key, size in (("keys", 28), ("keys_un", 28), ("desc", 32), ("u_right", 4), ("depth", 4)):
        assert b[o: o + n * size].tobytes() == ref[key].tobytes(), key
        o += n * size
    assert o == b.size
    fe.close()

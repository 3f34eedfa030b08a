"""csrc/rectify_math.h compiled for the host (tests/host/rectify_math_main.cpp, plain g++ -ffp-contract=off) against tests/rectify_reference.py: the float maps of
cv::initUndistortRectifyMap and their fixed-point entries for EuRoC left, EuRoC right and a seeded 8-coefficient calibration, compared bit for bit; a calibration
without an inverse and one whose map leaves the fixed-point range are refused.  The same program is built once more with the address and undefined-behaviour
sanitizers and run on its own on the same requests."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rectify_cases as G
import rectify_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
f64 = np.float64


def _build(tmp, name, extra=()):
    assert CXX is not None, "no host C++ compiler"
    exe = str(tmp / name)
    subprocess.run([CXX, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "rectify_math_main.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rectify_math")
    return _build(tmp, "rectify_math_main"), _build(tmp, "rectify_math_main_san", ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def seeded_calibration(seed=77):
    """an 8-coefficient (rational model) calibration with a tilted R and a P that differs from K: (K, D, R, P, (w, h))"""
    rng = np.random.default_rng(seed)
    K = np.array([[391.7 + rng.uniform(-5, 5), 0, 161.3], [0, 388.2 + rng.uniform(-5, 5), 118.9], [0, 0, 1]], f64)
    D = np.array([-0.21, 0.06, 7e-4, -4e-4, 0.011, 0.03, -0.012, 0.002], f64) * rng.uniform(0.8, 1.2, 8)
    a = rng.uniform(-0.02, 0.02, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
    Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
    Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
    P = np.array([[370.1, 0, 158.6, -41.3], [0, 370.1, 121.4, 0], [0, 0, 1, 0]], f64)
    return K.reshape(9), D, (Rz @ Ry @ Rx).reshape(9), P.reshape(12), (323, 241)


def requests():
    l, r, size, _ = G.euroc_eyes()
    K, D, Rm, P, sz = seeded_calibration()
    ok = [(l, size), (r, size), ((K, D, Rm, P), sz)]
    singular = ((K, D, np.array([1, 0, 0, 0, 1, 0, 1, 1, 0], f64), P), (16, 8))              # det(P3x3 R) == 0
    far = ((K * 1e9, np.zeros(8), Rm, P), (16, 8))                                            # entries of 1e11: refused by the fixed-point form
    return ok, singular, far


def _line(cal, size):
    v = np.concatenate([np.asarray(a, f64).reshape(-1) for a in cal])
    assert v.size == 38
    return "%d %d " % size + " ".join("%016x" % int(b) for b in v.view(np.uint64)) + "\n"


@pytest.mark.parametrize("which", [0, 1], ids=["plain", "sanitizers"])
def test_host_maps_equal_the_definition(programs, tmp_path, which):
    ok, singular, far = requests()
    assert R.init_undistort_rectify_map(*singular[0], singular[1]) is None and R.fix_maps(*R.init_undistort_rectify_map(*far[0], far[1])) is None
    fin, fout = str(tmp_path / "in.txt"), str(tmp_path / "out.bin")
    open(fin, "w").write("".join(_line(c, s) for c, s in ok + [singular, far]))
    subprocess.run([programs[which], fin, fout], check=True)
    got = np.fromfile(fout, np.uint8); pos = 0

    def take(dtype, n):
        nonlocal pos
        a = got[pos: pos + n * np.dtype(dtype).itemsize].view(dtype); pos += a.nbytes
        return a
    for cal, (w, h) in ok:
        assert take(np.int32, 1)[0] == 1
        mx, my = R.init_undistort_rectify_map(*cal, (w, h))
        ix, iy, ax, ay = R.fix_maps(mx, my)
        assert np.array_equal(take(np.uint32, w * h), mx.reshape(-1).view(np.uint32)), "map_x bits"
        assert np.array_equal(take(np.uint32, w * h), my.reshape(-1).view(np.uint32)), "map_y bits"
        assert np.array_equal(take(np.int16, w * h), ix.reshape(-1)) and np.array_equal(take(np.int16, w * h), iy.reshape(-1))
        assert np.array_equal(take(np.uint16, w * h), (ay * 32 + ax).reshape(-1).astype(np.uint16))
    assert take(np.int32, 1)[0] == 0 and take(np.int32, 1)[0] == -1 and pos == got.size

"""csrc/publish_math.h compiled for the host (tests/host/publish_math_main.cpp, -ffp-contract=off) against tests/publish_reference.py inverse4: the inverse of a float
4x4 compared as IEEE bit patterns, singular inputs included.  The same program is built once more with the address and undefined-behaviour sanitizers and run on its
own on the same requests."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import publish_cases as G
import publish_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
f32 = np.float32


def _build(tmp, name, extra=()):
    assert CXX is not None, "no host C++ compiler"
    exe = str(tmp / name)
    subprocess.run([CXX, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "publish_math_main.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("publish_math")
    return _build(tmp, "publish_math_main"), _build(tmp, "publish_math_main_san", ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _bits(a):
    return " ".join("%08x" % int(v) for v in np.asarray(a, f32).reshape(-1).view(np.uint32))


def requests():
    rng = np.random.default_rng(31); mats = []
    for k in range(120):
        T = G.pose(rng, scale=float(rng.choice([1.0, 0.013, 0.37, 41.0])), spread=float(rng.choice([0.0, 1.0, 1e3, 1e6])))
        if k % 3 == 0:
            T = (T * f32(1 + rng.uniform(-1e-2, 1e-2, (4, 4)))).astype(f32); T[3] = rng.uniform(-2, 2, 4).astype(f32)
        mats.append(T)
    S = np.eye(4, dtype=f32); S[2] = S[1]
    N = np.eye(4, dtype=f32); N[1, 2] = np.nan
    H = np.eye(4, dtype=f32) * f32(1e30)                           # the determinant overflows in float, not in double
    D = np.eye(4, dtype=f32) * f32(1e-30)
    mats += [np.eye(4, dtype=f32), np.zeros((4, 4), f32), S, N, H, D, np.full((4, 4), np.inf, f32)]
    out = []
    for T in mats:
        Ti = R.inverse4(T)
        out.append(("I " + _bits(T), "I singular" if Ti is None else "I " + _bits(Ti)))
    return out


@pytest.mark.parametrize("which", [0, 1], ids=["plain", "sanitizers"])
def test_host_inverse_equals_the_definition(programs, tmp_path, which):
    req = requests()
    assert sum(1 for _, w in req if w == "I singular") >= 4
    fin, fout = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    open(fin, "w").write("".join(r + "\n" for r, _ in req))
    subprocess.run([programs[which], fin, fout], check=True)
    got = open(fout).read().split("\n")[:-1]
    assert len(got) == len(req)
    for g, (r, w) in zip(got, req):
        assert g == w, (r[:120], g, w)

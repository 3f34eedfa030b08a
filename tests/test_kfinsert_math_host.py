"""csrc/kfinsert_math.h compiled for the host (tests/host/kfinsert_main.cpp, -ffp-contract=off) against tests/kfinsert_reference.py: the visit cut, the unprojection,
the normal and distances of a single observation and of a temporal point, the found ratio, the weighted nObs and the culling chain, compared as integers and IEEE bit
patterns.  The same program is built once more with the address and undefined-behaviour sanitizers and run on its own on the same requests."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import kfinsert_reference as R
import kfinsert_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
f32 = np.float32


def _build(tmp, name, extra=()):
    assert CXX is not None, "no host C++ compiler"
    exe = str(tmp / name)
    subprocess.run([CXX, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "kfinsert_main.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kfinsert_math")
    return _build(tmp, "kfinsert_main"), _build(tmp, "kfinsert_main_san", ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _hex(*vals):
    return " ".join("%08x" % int(np.asarray(v, f32).reshape(()).view(np.uint32)) for v in vals)


def _bits(a):
    return " ".join("%08x" % int(v) for v in np.asarray(a, f32).reshape(-1).view(np.uint32))


def requests():
    """(request line, the definition's answer line)"""
    rng = np.random.default_rng(77); out = []
    for m in (0, 1, 99, 100, 101, 102, 257, 2000):
        for near in sorted({0, 1, 99, 100, 101, m // 2, m} & set(range(m + 1))):
            for mode in (0, 1, 2):
                out.append(("V %d %d %d" % (m, near, mode), "V %d" % R.n_visited_closed_form(m, near, mode)))
    for z in (f32(0), f32(-0.0), f32(-1), f32(np.nan), f32(np.inf), f32(35), f32(35.000004), f32(1e-40), f32(12.5)):
        for th in (f32(35), f32(np.nan)):
            out.append(("C " + _hex(z, th), "C %d %d" % (1 if z > 0 else 0, 1 if z > th else 0)))
    scale = np.ones(16, f32); scale[:8] = G.SCALE
    for k in range(60):
        T = G._pose(rng)
        if k % 7 == 0:
            T = (T * f32(1 + rng.uniform(-1e-3, 1e-3, (4, 4)))).astype(f32)                     # (nothing relies on an orthonormal rotation)
        cam = dict(G.CAM); u, v, z = f32(rng.uniform(0, 1241)), f32(rng.uniform(0, 376)), f32(rng.uniform(0.3, 120))
        kp = np.zeros((), R.KP_DTYPE); kp["x"] = u; kp["y"] = v
        X = R.unproject(T, cam, kp, z)
        out.append(("U " + _bits(T) + " " + _hex(cam["fx"], cam["fy"], cam["cx"], cam["cy"], u, v, z), "U " + _bits(X)))
        octave = int(rng.integers(-1, 10)); nlevels = int(rng.choice([1, 4, 8]))
        n, mn, mx = R.single_observation(T, X, octave, nlevels, scale)
        out.append(("S %s %s %d %d %s" % (_bits(T), _bits(X), octave, nlevels, _bits(scale)), "S " + _bits(np.concatenate([n, [mn, mx]]))))
        n, mn, mx = R.temporal_point(T, X, octave, nlevels, scale)
        out.append(("T %s %s %d %d %s" % (_bits(T), _bits(X), octave, nlevels, _bits(scale)), "T " + _bits(np.concatenate([n, [mn, mx]]))))
    for found in (0, 1, 2, 3, 5, 1 << 24, (1 << 24) + 1, 2 ** 31 - 1):
        for visible in (0, 1, 3, 4, 5, 8, 12, 20, (1 << 26) + 3, 2 ** 31 - 1):
            out.append(("R %d %d" % (found, visible), "R %d" % (1 if R.found_ratio_culls(found, visible) else 0)))
    for at in (0, 1):
        for ur in (f32(-1), f32(0), f32(-0.0), f32(17.5), f32(np.nan)):
            out.append(("W %d %s" % (at, _hex(ur)), "W %d" % (2 if at and ur >= 0 else 1)))
    for bad in (0, 1):
        for found, visible in ((1, 1), (1, 5), (0, 0)):
            for cur, first in ((22, 22), (22, 21), (22, 20), (22, 19), (22, -1), (5, 9), (1000001, 999999)):
                for w in (0, 2, 3, 4):
                    for th in (2, 3):
                        out.append(("D %d %d %d %d %d %d %d" % (bad, found, visible, cur, first, w, th), "D %d" % R.cull_decision(bool(bad), found, visible, cur, first, w, th)))
    return out


@pytest.mark.parametrize("which", [0, 1], ids=["plain", "sanitizers"])
def test_host_arithmetic_equals_the_definition(programs, tmp_path, which):
    req = requests()
    fin, fout = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    open(fin, "w").write("".join(r + "\n" for r, _ in req))
    subprocess.run([programs[which], fin, fout], check=True)
    got = open(fout).read().split("\n")[:-1]
    assert len(got) == len(req)
    for g, (r, w) in zip(got, req):
        assert g == w, (r[:120], g, w)

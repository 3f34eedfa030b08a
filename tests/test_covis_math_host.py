"""csrc/covis_math.h compiled for the host (tests/host/covis_math_main.cpp) against tests/covis_reference.py on random inputs: the (weight, id) order, the fallback
pick, the weight of an observation and the culling decision -- the rules the kernels share, before a device is involved.  No GPU and no library."""
import os
import shutil
import subprocess
import numpy as np
import pytest

import covis_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert CXX is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("covis_math") / "covis_math_main")
    subprocess.run([CXX, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "covis_math_main.cpp"), "-o", exe], check=True)
    return exe


def f32(x):
    return int(np.float32(x).view(np.uint32))


def pick_of_walk(pairs):
    """the walk of KeyFrame.cc:450-455 over a map that ascends in the id: strict `>` from nmax = 0"""
    nmax, best = 0, None
    for i, w in sorted((i, w) for w, i in pairs):
        if w > nmax:
            nmax, best = w, i
    return best


def test_rules_match_the_reference_restatement(program, tmp_path):
    rng = np.random.default_rng(7)
    lines, want = [], []
    ids = [0, 1, 2, (1 << 63) - 1, 1 << 63, (1 << 64) - 2] + [int(x) for x in rng.integers(0, 1 << 62, 12)]
    for _ in range(400):
        wa, wb = (int(x) for x in rng.integers(0, 4, 2)); ia, ib = (ids[int(x)] for x in rng.integers(0, len(ids), 2))
        lines.append("B %d %d %d %d" % (wa, ia, wb, ib)); want.append(str(int((wa, ia) > (wb, ib))))        # pair<int, LightKeyFrame> descending
        lines.append("P %d %d %d %d" % (wa, ia, wb, ib)); want.append(str(int(wa > wb or (wa == wb and ia < ib))))
    m = R.Map(); m.kfs[1] = R.KeyFrame(1, [0, 0, 0], u_right=[-1.0, 0.0, 37.5])
    for idx in range(3):
        for in_store in (0, 1):
            mp = R.MapPoint(9, {(1 if in_store else 55): idx})
            lines.append("O %d %d" % (in_store, f32(m.kfs[1].u_right[idx]))); want.append(str(R.observations(m, mp)))
    for a in range(-1, 9):
        for b in range(0, 8):
            lines.append("C %d %d" % (a, b)); want.append(str(int(a <= b + 1)))
    for mono in (0, 1):
        for depth in (-1.0, -0.0, 0.0, 34.999, 35.0, 35.000004, 1e9):
            lines.append("D %d %d %d" % (mono, f32(depth), f32(35.0)))
            want.append(str(int((not mono) and (float(np.float32(depth)) > 35.0 or float(np.float32(depth)) < 0))))
    for n in list(range(0, 60)) + [99, 100, 101, 1000, 10 ** 6, 2 ** 31 - 1]:
        for r in sorted({0, n // 2, n * 9 // 10 - 1, n * 9 // 10, n * 9 // 10 + 1, n - 1, n} - {-1, -2}):
            lines.append("K %d %d" % (r, n)); want.append(str(int(r > 0.9 * n)))
    for n in (0, 1, 2, 3, 17, 64, 65, 300):
        for _ in range(6):
            chosen = rng.choice(1 << 20, n, replace=False) if n else []
            pairs = [(int(rng.integers(1, 5)), int(i) * ((1 << 43) + 1)) for i in chosen]
            lines.append("L %d %s" % (n, " ".join("%d %d" % p for p in pairs)))
            best = pick_of_walk(pairs)
            want.append("".join("%d:%d " % (i, w) for i, w in R.descending(pairs)) + "| %d" % (-1 if best is None else best))
    fin, fout = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    open(fin, "w").write("\n".join(lines) + "\n")
    subprocess.run([program, fin, fout], check=True)
    got = open(fout).read().split("\n")[:-1]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, lines[k], g, w)


def test_the_definition_uses_the_same_pick(tmp_path):
    """covis_reference.update_connections' fallback is the walk restated above (the lowest id among the maxima)"""
    m = R.Map()
    m.kfs[1] = R.KeyFrame(1, [10, 11, 12, 13]); m.kfs[5] = R.KeyFrame(5, []); m.kfs[3] = R.KeyFrame(3, []); m.kfs[9] = R.KeyFrame(9, [])
    m.mps[10] = R.MapPoint(10, {1: 0, 5: 0, 3: 0}); m.mps[11] = R.MapPoint(11, {1: 1, 5: 0, 3: 0}); m.mps[12] = R.MapPoint(12, {1: 2, 9: 0}); m.mps[13] = R.MapPoint(13, {1: 3})
    assert R.update_connections(m, 1) == pick_of_walk([(2, 5), (2, 3), (1, 9)]) == 3

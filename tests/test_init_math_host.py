"""csrc/init_math.h compiled for the host (tests/host/initializer_main.cpp, -ffp-contract=off) against tests/initializer_reference.py on every case of
tests/gpu_init_cases.py, outputs compared as bytes (a NaN equal to a NaN: payloads are not part of a reading; `parallax` is the same libm formula on both sides).  No
GPU and no library: this is the kernels' arithmetic before a device is involved."""
import os
import shutil
import struct
import subprocess
import numpy as np
import pytest

import initializer_reference as R
import gpu_init_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert CXX is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("init_math") / "initializer_main")
    subprocess.run([CXX, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "initializer_main.cpp"),
                    "-o", exe], check=True)
    return exe


def write_problems(path, cases):
    """cases of one parameter set"""
    p = cases[0]["params"]
    with open(path, "wb") as f:
        f.write(struct.pack("<iiffi", len(cases), p["max_iterations"], p["sigma"], p["min_parallax"], p["min_triangulated"]))
        for c in cases:
            pr = c["problem"]
            f.write(struct.pack("<ii4f", len(pr["keys1"]), len(pr["keys2"]), *pr["K"]))
            f.write(pr["keys1"].astype("<f4").tobytes()); f.write(pr["keys2"].astype("<f4").tobytes()); f.write(pr["matches12"].astype("<i4").tobytes())
        for c in cases:
            f.write(np.asarray(c["rand"], "<i4").tobytes())


def read_results(path, cases):
    raw = open(path, "rb").read(); off = 0; out = []
    for c in cases:
        pr = c["problem"]; n1 = len(pr["keys1"]); N = int((pr["matches12"] >= 0).sum()); its = c["params"]["max_iterations"]
        rec = np.frombuffer(raw, R.RESULT_DTYPE, 1, off)[0]; off += R.RESULT_DTYPE.itemsize
        p3d = np.frombuffer(raw, "<f4", n1 * 3, off).reshape(n1, 3); off += n1 * 12
        tri = np.frombuffer(raw, np.uint8, n1, off); off += n1
        ih = np.frombuffer(raw, np.uint8, N, off); off += N
        i_f = np.frombuffer(raw, np.uint8, N, off); off += N
        sc = np.frombuffer(raw, "<f4", its * 2, off).reshape(its, 2); off += its * 8
        out.append(dict(result=rec, p3d=p3d, triangulated=tri, inliers_h=ih, inliers_f=i_f, scores=sc))
    assert off == len(raw)
    return out


def same_bytes(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b).astype(a.dtype)
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        return a.shape == b.shape and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_host_program_matches_the_restatement_byte_for_byte(program, tmp_path):
    groups = {}
    for name, c in G.cases().items():
        groups.setdefault(tuple(sorted(c["params"].items())), []).append(c)
    n_checked = 0
    for k, cases in enumerate(groups.values()):
        fin, fout = str(tmp_path / ("in%d.bin" % k)), str(tmp_path / ("out%d.bin" % k))
        write_problems(fin, cases)                                       # (several problems per file: a batch of different N, n1 and n2)
        subprocess.run([program, fin, fout], check=True)
        for c, got in zip(cases, read_results(fout, cases)):
            want = G.expected(c["name"])
            for f in R.RESULT_DTYPE.names:
                assert same_bytes(got["result"][f], np.asarray(want[f], R.RESULT_DTYPE[f].base)), (c["name"], f, got["result"][f], want[f])
            for f in ("p3d", "triangulated", "inliers_h", "inliers_f", "scores"):
                assert same_bytes(got[f], want[f]), (c["name"], f)
            n_checked += 1
    assert n_checked == len(G.cases()) >= 20


def test_host_program_rejects_fewer_than_8_matches(program, tmp_path):
    c = dict(G.cases()["general8"]); pr = dict(c["problem"]); m = pr["matches12"].copy(); m[np.nonzero(m >= 0)[0][0]] = -1; pr["matches12"] = m; c["problem"] = pr
    write_problems(str(tmp_path / "in.bin"), [c])
    assert subprocess.run([program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")]).returncode == 3


def test_host_program_times_a_pass(program, tmp_path):
    c = G.cases()["general129"]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_problems(fin, [c])
    r = subprocess.run([program, fin, fout, "2"], check=True, capture_output=True, text=True)
    assert r.stdout.startswith("seconds_per_pass ") and float(r.stdout.split()[1]) > 0

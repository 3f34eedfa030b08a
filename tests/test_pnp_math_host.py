"""csrc/pnp_math.h compiled for the host (tests/host/pnp_math_main.cpp, -ffp-contract=off) against tests/pnpsolver_reference.py, bit for bit: compute_pose on drawn sets and
on Refine()-sized sets, CheckInliers over the whole problem.  No GPU and no library: this is the kernels' arithmetic before a device is involved."""
import os
import shutil
import struct
import subprocess
import numpy as np
import pytest

import pnpsolver_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert CXX is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pnp_math") / "pnp_math_main")
    subprocess.run([CXX, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "pnp_math_main.cpp"),
                    "-o", exe], check=True)
    return exe


def write_problems(path, problems):
    """problems: [(problem, [index lists])]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(problems)))
        for pr, sets in problems:
            f.write(struct.pack("<ii4f", pr["n"], len(sets), *[float(k) for k in pr["K"]]))
            rows = np.concatenate([pr["p3dw"], pr["p2d"], pr["max_err"][:, None]], axis=1).astype("<f4")
            f.write(rows.tobytes())
            for s in sets:
                f.write(struct.pack("<i", len(s))); f.write(np.asarray(s, "<i4").tobytes())


def read_results(path, problems):
    out = []; raw = open(path, "rb").read(); off = 0
    for pr, sets in problems:
        res = []
        for _ in sets:
            pose = np.frombuffer(raw, "<f8", 16, off); off += 128
            count = struct.unpack_from("<i", raw, off)[0]; off += 4
            flags = np.frombuffer(raw, np.uint8, pr["n"], off).astype(bool); off += pr["n"]
            res.append((pose, count, flags))
        out.append(res)
    assert off == len(raw)
    return out


def expected(pr, sets):
    out = []
    by_len = {}
    for k, s in enumerate(sets):
        by_len.setdefault(len(s), []).append(k)
    poses = [None] * len(sets)
    for n, ks in by_len.items():
        idx = np.array([sets[k] for k in ks], np.int64)
        p = ref.pose16(ref.compute_pose(*ref.gather_sets(pr, idx), pr["K"]))
        for k, row in zip(ks, p):
            poses[k] = row
    for p in poses:
        fl = ref.check_inliers(pr, p[:9], p[9:12])[0]
        out.append((p, int(fl.sum()), fl))
    return out


def cases():
    out = []
    for seed, n, share, noise, min_set in [(1, 60, 0.6, 0.0, 4), (2, 130, 0.5, 0.5, 4), (3, 65, 0.9, 0.5, 6), (4, 40, 0.0, 0.0, 4), (5, 100, 0.7, 0.3, 8)]:
        pr, truth = ref.scene(seed, n, share, noise)
        rv = ref.draws(seed, 1, 24, min_set)[0]
        sets = [ref.draw_set(r, min_set, n) for r in rv]
        inl = np.flatnonzero(truth["inlier"])
        if len(inl) >= 6:
            sets += [list(inl), list(inl[: len(inl) // 2]), list(range(n))]            # Refine()-sized sets, and one with the outliers in it
        out.append((pr, sets))
    return out


def special_problem():
    """the forced sets of the GPU suite's special case: coplanar points, a duplicated point, a correspondence on the camera plane and a non-finite pose"""
    import gpu_pnp_cases
    return gpu_pnp_cases.special()


def test_host_program_matches_the_restatement_bit_for_bit(program, tmp_path):
    problems = cases()
    pr, sets, _ = special_problem(); problems.append((pr, sets))
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_problems(fin, problems)
    subprocess.run([program, fin, fout], check=True)
    got = read_results(fout, problems)
    n_checked = 0
    for (pr, sets), res in zip(problems, got):
        for k, ((pose, count, flags), (epose, ecount, eflags)) in enumerate(zip(res, expected(pr, sets))):
            assert ref.same_bits(pose, epose), (pr["n"], k, sets[k][:8], pose, epose)
            assert count == ecount and np.array_equal(flags, eflags), (pr["n"], k)
            n_checked += 1
    assert n_checked >= 5 * 24


def test_host_program_times_a_pass(program, tmp_path):
    pr, _ = ref.scene(7, 100, 0.5, 0.5)
    sets = [ref.draw_set(r, 4, 100) for r in ref.draws(7, 1, 35)[0]]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_problems(fin, [(pr, sets)])
    r = subprocess.run([program, fin, fout, "3"], check=True, capture_output=True, text=True)
    assert r.stdout.startswith("seconds_per_pass ") and float(r.stdout.split()[1]) > 0

"""csrc/voctrain_math.h compiled for the host (tests/host/voctrain_main.cpp, -ffp-contract=off) against tests/voctrain_reference.py, output compared as text of integers
and IEEE bit patterns.  The host function trains level by level, as the device does, and renumbers the nodes afterwards; the definition is recursive and depth first: this
is the check, without a GPU, that level order gives the same vocabulary and the same statistics."""
import os
import shutil
import struct
import subprocess
import pytest

import voctrain_reference as V
import voctrain_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert CXX is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("voctrain_math") / "voctrain_main")
    subprocess.run([CXX, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "voctrain_main.cpp"),
                    "-o", exe], check=True)
    return exe


def run(program, tmp_path, cases, extra=()):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.txt")
    with open(fin, "wb") as o:
        o.write(struct.pack("<i", len(cases)))
        for c in cases:
            G.write_case(o, *c)
    subprocess.run([program, fin, fout] + list(extra), check=True)
    return open(fout).read().split("\n")[:-1]


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_level_order_on_the_host_equals_the_recursive_definition(program, tmp_path, name):
    got = run(program, tmp_path, [G.inputs(name)])
    want = G.result_text(*G.expected(name))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (g[:200], w[:200])


def test_refused_arguments_and_the_text_form(program, tmp_path):
    sets, k, L, seed, max_it = G.inputs("k3L3n200")
    bad = [(sets, 1, L, seed, max_it), (sets, 21, L, seed, max_it), (sets, k, 0, seed, max_it), (sets, k, 11, seed, max_it), (sets, k, L, seed, 0), ([sets[1]], k, L, seed, max_it)]
    got = run(program, tmp_path, bad)
    assert got == ["E k must be in [2, 20]"] * 2 + ["E L must be in [1, 10]"] * 2 + ["E max_iterations must be at least 1", "E no training feature"]
    for c in bad:
        with pytest.raises(ValueError):
            V.create(*c)
    flat = G.expected("k3L3n200")[0]
    for digits in (0, 17):
        text = str(tmp_path / ("voc%d.txt" % digits))
        run(program, tmp_path, [G.inputs("k3L3n200")], [str(digits), text])
        assert open(text, "rb").read() == V.save_text(flat, digits).encode()

"""GPU test: the adapter's corb::ORBVocabulary::create(training_features, k, L) and saveToTextFile (corb-slam_amd/host/corb_adapter_orbslam.hpp), compiled with g++ -Wall
-Werror and driven by tests/host/voctrain_adapter_main.cpp on a test double of cv::Mat, write the definition's vocabulary (tests/voctrain_reference.py) byte for byte."""
import os
import subprocess
import pytest

import voctrain_reference as V
import voctrain_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_adapter_create_and_save_write_the_definitions_text(tmp_path, corb):
    exe = tmp_path / "voctrain_adapter_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "voctrain_adapter_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    for name, digits in (("k3L3n200", 0), ("cap2small", 17)):
        fin, fout = tmp_path / "in.bin", tmp_path / "voc.txt"
        with open(fin, "wb") as o:
            G.write_case(o, *G.inputs(name))
        got = subprocess.check_output([str(exe), str(fin), str(fout), str(digits)]).decode().split()
        flat, st = G.expected(name)
        assert [int(x) for x in got] == [st["nodes"], st["words"], st["capped_nodes"], st["words"]]
        assert fout.read_bytes() == V.save_text(flat, digits).encode()

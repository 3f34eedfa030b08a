"""CPU compile tests of the rectifier's boundary: include/corb_stereo_rectify.h is pure C (compiles as C11), names its definition, and the C++ host mirror
corb::StereoRectifier (corb-slam_amd/host/corb_host.hpp) builds with plain g++ against the C-ABI only (tests/host/rectify_main.cpp)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "corb_stereo_rectify.h")


def test_header_is_c11_and_names_its_definition(tmp_path, corb):
    src = open(HDR).read()
    assert "tests/rectify_reference.py" in src and "stereo_euroc.cc" in src and "ros_stereo.cc" in src
    c = tmp_path / "t.c"
    c.write_text('#include <corb_stereo_rectify.h>\nint main(void){ CorbRectifyConfig c; (void)c; return sizeof(CorbRectifyEye) == 38 * 8 && sizeof(CorbRectifyConfig) == 8 + 2 * 38 * 8 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")])
    subprocess.check_call([str(tmp_path / "t")])
    assert ctypes.sizeof(corb.RectifyEye) == 38 * 8 and ctypes.sizeof(corb.RectifyConfig) == 8 + 2 * 38 * 8


def test_library_exports_every_symbol_the_header_declares(corb):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(corb_rect_[a-z0-9_]+)\s*\(", src)))
    L = corb.load()
    assert set(names) == set(corb.RECTIFY_EXPORTS) and len(names) == 6 and all(hasattr(L, n) for n in names)
    assert not set(corb.RECTIFY_EXPORTS) & set(corb.EXPORTS)
    # the arithmetic is stated once for the library and the stand-alone program
    mk = open(os.path.join(ROOT, "corb-slam_amd", "Makefile")).read()
    for f in ("csrc/rectify_kernels.hip", "csrc/corb_rectify.cpp", "csrc/rectify_math.h", "csrc/rectify_internal.h", "../include/corb_stereo_rectify.h"):
        assert f in mk, f


def test_cpp_host_mirror_compiles_and_links(tmp_path):
    out = tmp_path / "rectify_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "rectify_main.cpp"), "-o", str(out),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    assert out.exists()

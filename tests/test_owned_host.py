"""csrc/owned.h compiled for the host on its own (tests/host/owned_main.cpp; never loaded into Python), over an allocator that wraps malloc / free, counts its calls
and can be told to fail one: room below, at and above the capacity; a failed request; moves; empty owners; the list's release(keep); the id table's capacity.  Built
once plain and once with the address and undefined-behaviour sanitizers, whose leak check ends every run.  The sanitizer leg is asserted, not skipped: a compiler
that cannot link the runtime fails the module with its own message.  The same program with the owner replaced by one whose room() forgets to release the old
allocation must be reported: the check of the check."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
ASAN = ("-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
MODES = ("room", "fail", "move", "empty", "list", "table")


def _build(tmp, name, extra=("-O2",)):
    assert CXX is not None, "no host C++ compiler"
    exe = str(tmp / name)
    p = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "owned_main.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, "%s %s: %s" % (CXX, " ".join(extra), p.stdout)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("owned")
    return {"plain": _build(tmp, "owned"), "asan": _build(tmp, "owned_asan", ASAN), "asan_forgets": _build(tmp, "owned_asan_forgets", ASAN + ("-DOWNED_ROOM_FORGETS_RELEASE",))}


def _run(exe, what):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    return subprocess.run([exe, what], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)


@pytest.mark.parametrize("build", ["plain", "asan"])
@pytest.mark.parametrize("mode", MODES)
def test_owner(programs, build, mode):
    p = _run(programs[build], mode)
    assert p.returncode == 0 and ", 0 mismatches" in p.stdout, p.stdout      # status 0 under the sanitizers: no leak, no bad access, no undefined behaviour


def test_the_id_table_saw_every_size(programs):
    p = _run(programs["plain"], "table")
    assert "table: 78 requests" in p.stdout, p.stdout                        # (0, 1, 31, 32, 33 and 2^k - 1, 2^k, 2^k + 1 for k = 6 .. 12) up, down, and fresh


def test_growth_is_clean_with_the_owner(programs):
    p = _run(programs["asan"], "grow")
    assert p.returncode == 0 and "grow: capacity 64" in p.stdout, p.stdout


def test_the_leak_check_reports_a_room_that_forgets_to_release(programs):
    p = _run(programs["asan_forgets"], "grow")
    assert p.returncode != 0 and "LeakSanitizer" in p.stdout and "48 byte(s) leaked in 2 allocation(s)" in p.stdout, (p.returncode, p.stdout)

"""csrc/record_locks.h compiled for the host on its own (tests/host/record_locks_main.cpp; never loaded into Python): the id-table capacity against the six loops it
replaced and against its closed statement; the lock holder on every combination of owner, stores and map; and, built with the thread sanitizer, four threads that name
the two stores in opposite orders.  The sanitizer leg is asserted, not skipped: a compiler that cannot link the runtime fails the module with its own message.  The
same program with the holder replaced by one that locks in argument order must be reported: the check of the check."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
TSAN = ("-O1", "-g", "-fsanitize=thread")


def _build(tmp, name, extra=("-O2",)):
    assert CXX is not None, "no host C++ compiler"
    exe = str(tmp / name)
    p = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", "-pthread", *extra, "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "record_locks_main.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, "%s %s: %s" % (CXX, " ".join(extra), p.stdout)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("record_locks")
    return {"plain": _build(tmp, "record_locks"), "tsan": _build(tmp, "record_locks_tsan", TSAN),
            "tsan_argument_order": _build(tmp, "record_locks_tsan_argorder", TSAN + ("-DRECORD_LOCKS_ARGUMENT_ORDER",))}


def _run(exe, what):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    return subprocess.run([exe, what], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)


def test_capacity_equals_the_six_historic_loops_and_the_closed_statement(programs):
    p = _run(programs["plain"], "capacity")
    assert p.returncode == 0, p.stdout
    assert "63 inputs, 0 mismatches" in p.stdout, p.stdout                       # 0, 1, 2, 31, 32, 33 and 2^k - 1, 2^k, 2^k + 1 for k = 6 .. 24


def test_holder_holds_what_is_named_and_nothing_else(programs):
    p = _run(programs["plain"], "holder")
    assert p.returncode == 0, p.stdout
    assert "24 combinations, 0 mismatches" in p.stdout, p.stdout                 # owner x 6 store pairs x map


def test_four_threads_with_the_stores_swapped_take_one_order(programs):
    p = _run(programs["tsan"], "order")
    assert p.returncode == 0 and "order: 8000 takes" in p.stdout, p.stdout       # status 0: no lock-order-inversion report, no data-race report
    q = _run(programs["tsan"], "holder")
    assert q.returncode == 0, q.stdout


def test_the_sanitizer_reports_a_holder_that_locks_in_argument_order(programs):
    p = _run(programs["tsan_argument_order"], "order")
    assert p.returncode != 0 and "lock-order-inversion" in p.stdout, (p.returncode, p.stdout)

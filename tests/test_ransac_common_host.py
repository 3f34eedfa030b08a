"""The plain C++ part of csrc/ransac_common.h compiled for the host on its own (tests/host/ransac_common_main.cpp, -ffp-contract=off; never loaded into Python): the
draw rule of the three RANSAC routes against a literal std::vector emulation of the reference's loop -- every tuple of positions for a set of 3 at N = 3 .. 9 and for a
set of 4 at N = 4 .. 7, seeded random values for sets of 4 .. 8 at N = set size .. set size + 3 -- and draws, iteration caps, scattered flags and the range check
for a table of inputs against tests/ransac_reference.py and the caps of sim3solver_reference and pnpsolver_reference.  Built once plain and once with the address and
undefined-behaviour sanitizers as a stand-alone program; the sanitizer leg is asserted, not skipped."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pnpsolver_reference as P
import ransac_reference as R
import sim3solver_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
ASAN = ("-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
f32 = np.float32


def _build(tmp, name, extra=("-O2",)):
    assert CXX is not None, "no host C++ compiler"
    exe = str(tmp / name)
    p = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "ransac_common_main.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, "%s %s: %s" % (CXX, " ".join(extra), p.stdout)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ransac_common")
    return {"plain": _build(tmp, "ransac_common"), "asan": _build(tmp, "ransac_common_asan", ASAN)}


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    return subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_draw_rule_equals_the_literal_vector_emulation(programs, build):
    p = _run(programs[build], "check")
    # sets of 3: sum over N = 3 .. 9 of N (N - 1) (N - 2) = 1260 tuples; sets of 4: N = 4 .. 7: 24 + 120 + 360 + 840; 5 sizes x 4 N x 4000 seeded; 6 all-last
    assert p.returncode == 0 and p.stdout.strip().endswith("%d draws, 0 mismatches" % (1260 + 1344 + 80000 + 6)), p.stdout


def cap_rows():
    """(N, nMinInliers, float epsilon, probability, max_iterations, the solver's own cap): N just below, at and above min_inliers and well above it, epsilon 0.2, 0.4,
    0.5, max_iterations 1 and 300"""
    rows = []
    for max_its in (1, 300):
        for mn in (6, 20):
            for N in (mn - 1, mn, mn + 1, 2 * mn, 10 * mn + 3):
                rows.append((N, mn, f32(mn) / f32(N), 0.99, max_its, S.ransac_cap(N, 0.99, mn, max_its)))                  # Sim3Solver: epsilon = nMinInliers / N
        for eps in (0.2, 0.4, 0.5):
            for mn in (8, 10):
                for N in (mn - 1, mn, mn + 1, 2 * mn, 10 * mn + 3):
                    m = max(int(f32(N) * f32(eps)), mn, 4)                                                                   # PnPsolver's adjustments (:179-189)
                    e = max(f32(eps), f32(m) / f32(N))
                    cap, m_ref = P.ransac_parameters(N, 0.99, mn, max_its, 4, eps)
                    assert m == m_ref
                    rows.append((N, m, e, 0.99, max_its, cap))
    return rows


def table():
    """[(input line, expected answer line)]"""
    rng = np.random.default_rng(11)
    out = []
    for n in (3, 4, 6, 8):
        for N in (n, n + 1, n + 2, 40, 2000):
            for r in rng.integers(0, R.RAND_RANGE, size=(4, n)).tolist() + [[R.RAND_RANGE - 1] * n, [0] * n]:
                out.append(("draw %d %d %s" % (n, N, " ".join(map(str, r))), "".join("%d " % v for v in R.draw_set(r, n, N))))
    for N, m, e, prob, max_its, cap in cap_rows():
        assert R.iteration_cap(N, m, e, prob, max_its) == cap, (N, m, e, max_its)
        out.append(("cap %d %d %d %r %d" % (N, m, int(np.array([e], f32).view(np.uint32)[0]), prob, max_its), "%d" % cap))
    for N, stride in ((65, 65), (65, 80), (64, 64), (130, 100), (1, 1), (0, 4)):
        words = max((N + 63) // 64, 1)
        bits = rng.integers(0, 2, size=words * 64).astype(np.uint64)
        mask = [int(sum(int(b) << k for k, b in enumerate(bits[64 * w: 64 * w + 64]))) for w in range(words)]                # (bits behind N are set too: never read)
        out.append(("scatter %d %d %d 0 %s" % (N, stride, words, " ".join(map(str, mask))), "".join(map(str, R.scatter_flags(mask, N, None, stride)))))
        index = (rng.permutation(N + 6) - 3)[:N]                                                                             # some features outside [0, stride)
        out.append(("scatter %d %d %d 1 %s %s" % (N, stride, words, " ".join(map(str, mask)), " ".join(map(str, index))),
                    "".join(map(str, R.scatter_flags(mask, N, index, stride)))))
    out.append(("rand 4 0 1 2147483647 5", "ok"))
    out.append(("rand 0", "ok"))
    out.append(("rand 4 0 1 -1 -5", "who: rand_values[2] is outside [0, 2^31)"))
    out.append(("rand 1 -2147483648", "who: rand_values[0] is outside [0, 2^31)"))
    return out


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_draws_caps_flags_and_the_range_check_equal_the_reference(programs, build, tmp_path):
    rows = table()
    path = tmp_path / "table.txt"
    path.write_text("".join(line + "\n" for line, _ in rows))
    p = _run(programs[build], "table", str(path))
    got = p.stdout.split("\n")
    assert p.returncode == 0 and len(got) == len(rows) + 1 and got[-1] == "", p.stdout[-2000:]
    for (line, want), g in zip(rows, got):
        assert g == want, (line, g, want)
    assert sum(line.startswith("cap") for line, _ in rows) == 2 * (10 + 30)


def test_the_caps_cover_every_branch():
    caps = [(N, m, cap, max_its) for N, m, _, _, max_its, cap in cap_rows()]
    assert any(cap == 0 for _, _, cap, _ in caps) and any(N == m and cap == 1 for N, m, cap, _ in caps)                     # N < nMinInliers; nMinInliers == N
    assert any(cap == 300 for _, _, cap, _ in caps) and any(1 < cap < 300 for _, _, cap, _ in caps)                          # clamped above; the expression itself
    assert all(cap <= 1 for _, _, cap, max_its in caps if max_its == 1)

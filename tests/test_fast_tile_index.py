"""Host check of orb_fast_tile.h, the index arithmetic of orb_fast_kernel's 16-bit LDS tile (no GPU): a stand-alone program, built with the host
compiler and the address / undefined-behaviour sanitizers, walks every cell size cw, ch in 7 .. 70, every 4-pixel group, pair, ring row and all
three tile pitches, with the tile height at its tightest (fast_th = ch), and asserts that

  * every dword the kernel reads in phase 1 (compass) and phase 2 (ring of a listed pair) lies inside the row it belongs to and inside the slots
    the tile write initialises (all TP slots of the rows 0 .. ch-1), and so does every dword whose score bytes phases 2 and 3 touch,
  * the interior of every row starts 8-byte aligned and a 4-pixel group is one aligned 8-byte word,
  * the dynamic LDS the launch requests covers tile + row masks, and the carve's parts do not overlap."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corb-slam_amd", "csrc")

PROGRAM = r"""
#include "orb_fast_tile.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s  (TP %d cw %d ch %d g %d pair %d y %d dy %d)\n", #c, TP, cw, ch, g, pair, y, dy); return 1; } } while (0)

int main()
{
    long reads = 0, cases = 0;
    const int pitches[3] = {40, 48, 80};
    for (int pi = 0; pi < 3; pi++) {
        const int TP = pitches[pi];
        for (int cw = 7; cw <= 70; cw++)
            for (int ch = 7; ch <= 70; ch++) {
                int g = -1, pair = -1, y = -1, dy = 0;
                const int iw = cw - 6;
                // the pitch a level with this cell needs (wCell >= iw); a pitch class serves every requirement up to its own
                if (fast_tile_min_pitch(iw) > TP) continue;
                cases++;
                const int th = ch;                                  // tightest tile: fast_th = max hCell + 6 >= ch
                const int PD = fast_tile_row_dwords(TP), ng = fast_tile_groups(cw);
                CHECK(PD * 4 == TP * 2);                            // a row is TP 16-bit slots
                CHECK((PD * 4) % 8 == 0);                           // rows keep the 8-byte alignment of the tile base
                // model of the carve in bytes: 1 = initialised tile slot bytes, 3 = row masks
                const unsigned dyn = fast_dynamic_lds_bytes(TP, th);
                std::vector<unsigned char> lds(dyn, 0);
                CHECK(fast_tile_bytes(TP, th) == (unsigned)(PD * 4 * th));
                for (int r = 0; r < ch; r++) for (int b = 0; b < PD * 4; b++) lds[(size_t)r * PD * 4 + b] = 1;      // the tile write: every slot of rows 0 .. ch-1
                const long rm0 = (long)fast_tile_bytes(TP, th);
                CHECK(rm0 % 4 == 0);
                for (unsigned b = 0; b < fast_rowmask_bytes(th); b++) { const long a = rm0 + b; CHECK(a >= 0 && a < (long)dyn); CHECK(lds[a] == 0); lds[a] = 3; }
                CHECK(rm0 + (long)fast_rowmask_bytes(th) == (long)dyn);       // the launch's request is exactly tile + masks
                CHECK(fast_rowmask_bytes(th) >= 8u * (unsigned)(ch - 6));     // a mask pair per interior row
                CHECK(fast_cell_lds_bytes(TP, th) == dyn + 2u * FAST_LIST_CAP);
                CHECK(FAST_LIST_CAP >= FAST_LIST_SWEEP && FAST_LIST_SWEEP >= 128);   // a sweep appends at most 64 lanes x 2 pairs
                auto tile_dword_ok = [&](int row, int d) {          // dword d of tile row `row`: inside the row and initialised
                    if (row < 0 || row >= ch || d < 0 || d >= PD) return false;
                    const size_t a = ((size_t)row * PD + d) * 4;
                    return lds[a] == 1 && lds[a + 3] == 1;
                };
                for (y = 3; y < ch - 3; y++)
                    for (g = 0; g < ng; g++) {
                        // the interior starts at byte 8 of a row; a group is one aligned 8-byte word
                        CHECK(fast_tile_pair_dword(0, 0) * 4 == 8);
                        CHECK(((y * PD + fast_tile_pair_dword(g, 0)) * 4) % 8 == 0);
                        CHECK(fast_tile_pair_dword(g, 1) == fast_tile_pair_dword(g, 0) + 1);
                        // phase 1
                        for (dy = -3; dy <= 3; dy += 3) {
                            const int f = fast_tile_compass_first(g, dy), n = fast_tile_compass_count(dy);
                            CHECK(((y * PD + f) * 4) % 8 == 0 && n % 2 == 0);          // read as 8-byte words
                            for (int k = 0; k < n; k++) { CHECK(tile_dword_ok(y + dy, f + k)); reads++; }
                        }
                        // phase 2 (a listed pair: its first pixel lies inside the interior)
                        for (pair = 0; pair < 2; pair++) {
                            if (4 * g + 2 * pair >= iw) continue;
                            const int q = fast_tile_pair_dword(g, pair);
                            CHECK(2 * q == 4 + 4 * g + 2 * pair);                        // the dword holds tile columns 4 + px, 5 + px
                            for (dy = -3; dy <= 3; dy++) {
                                int nread = 0;
                                for (int k = -3; k <= 3; k++) {
                                    if (!fast_tile_ring_reads(dy, k)) continue;
                                    CHECK(k >= -fast_tile_ring_reach(dy) && k <= fast_tile_ring_reach(dy));
                                    CHECK(tile_dword_ok(y + dy, q + k)); reads++; nread++;
                                }
                                CHECK(nread == (dy == 0 ? 5 : (dy == 1 || dy == -1) ? 4 : (dy == 2 || dy == -2) ? 2 : 3));
                            }
                            dy = 0;
                            CHECK(tile_dword_ok(y, q));                                  // phase 2 stores the pair's two score bytes into its own dword
                            // phase 3: the score window of the pair, one row and one dword around it
                            for (dy = -1; dy <= 1; dy++) for (int k = -fast_tile_nms_reach(); k <= fast_tile_nms_reach(); k++) CHECK(tile_dword_ok(y + dy, q + k));
                            dy = 0;
                        }
                        pair = -1;
                        // phase 3 over groups (cells that needed a second list batch): both pair dwords of the group, the same window each
                        for (pair = 0; pair < 2; pair++)
                            for (dy = -1; dy <= 1; dy++) for (int k = -fast_tile_nms_reach(); k <= fast_tile_nms_reach(); k++) CHECK(tile_dword_ok(y + dy, fast_tile_pair_dword(g, pair) + k));
                        pair = -1; dy = 0;
                    }
            }
    }
    if (cases != (32 + 40 + 64) * 64) { std::printf("FAIL: %ld cases\n", cases); return 1; }      // interiors up to 32 / 40 / 64 columns x 64 heights
    std::printf("ok %ld cases %ld dword reads\n", cases, reads);
    return 0;
}
"""


def test_fast_tile_index_header(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = tmp_path / "fast_tile_check.cpp"
    exe = tmp_path / "fast_tile_check"
    src.write_text(PROGRAM)
    base = [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)]
    r = subprocess.run(base[:3] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[3:], capture_output=True, text=True)
    if r.returncode != 0:                        # a host without the sanitizer runtimes still checks the arithmetic
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr

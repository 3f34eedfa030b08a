"""csrc/bow_math.h compiled for the host (tests/host/bow_main.cpp, -ffp-contract=off) against tests/dbow_reference.py, output compared as text of integers and IEEE bit
patterns: the transform on every vocabulary of tests/bow_cases.py, the score on pairs of the transformed sets, and a scripted keyframe-database session.  No GPU and no
library: this is the kernels' arithmetic, and the (first common word, sequence number) order that replaces the inverted file, before a device is involved."""
import os
import shutil
import struct
import subprocess
import numpy as np
import pytest

import dbow_reference as R
import bow_cases as G
from bow_cases import ints, state_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
CODES = {"set_bow": 0, "add": 1, "erase": 2, "clear": 3, "nb": 4, "query": 5}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert CXX is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("bow_math") / "bow_main")
    subprocess.run([CXX, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "corb-slam_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "tests", "host", "bow_main.cpp"),
                    "-o", exe], check=True)
    return exe


def write_cases(path, v, sets, pairs, n_entries, levelsup, ops):
    f = v.flat()
    with open(path, "wb") as o:
        o.write(struct.pack("<5i", f["k"], f["L"], f["scoring"], f["weighting"], len(f["parent"])))
        o.write(f["parent"].astype("<i4").tobytes()); o.write(f["is_leaf"].astype("<i4").tobytes()); o.write(f["descriptor"].tobytes()); o.write(f["weight"].astype("<f8").tobytes())
        o.write(struct.pack("<i", len(sets)))
        for lu, d in sets:
            o.write(struct.pack("<ii", lu, len(d))); o.write(np.ascontiguousarray(d, np.uint8).tobytes())
        o.write(struct.pack("<i", len(pairs)))
        for a, b in pairs:
            o.write(struct.pack("<ii", a, b))
        o.write(struct.pack("<iii", n_entries, levelsup, len(ops)))
        for op in ops:
            o.write(struct.pack("<i", CODES[op[0]]))
            if op[0] == "set_bow":
                o.write(struct.pack("<ii", op[1], len(op[2]))); o.write(np.ascontiguousarray(op[2], np.uint8).tobytes())
            elif op[0] in ("add", "erase"):
                o.write(struct.pack("<i", op[1]))
            elif op[0] == "nb":
                o.write(struct.pack("<i", op[1])); o.write(np.asarray(op[2], "<i4").tobytes())
            elif op[0] == "query":
                o.write(struct.pack("<iiQfi", op[1], op[2], op[3], op[5], len(op[4]))); o.write(np.asarray(op[4], "<i4").tobytes())


def transform_text(t):
    word, value, node, off, idx, fw, fn = t
    return ["T %d %d" % (len(word), len(node)), ints("w", word), "v" + "".join(" %016x" % int(x) for x in value.view(np.uint64)), ints("n", node), ints("o", off), ints("i", idx),
            ints("fw", fw), ints("fn", fn)]


@pytest.mark.parametrize("name", sorted(G.VOCABS))
def test_transform_and_score_match_the_definition_byte_for_byte(program, tmp_path, name):
    v = G.vocab(name)
    shapes = [(n, lu) for n in (0, 1, 65, 257) for lu in (0, 2, 4, v.L, v.L + 1)]
    sets = [(lu, G.features(name, n, 40 + n)) for n, lu in shapes]
    pairs = [(a, b) for a in range(len(sets)) for b in (a, (a + 5) % len(sets), (a + 7) % len(sets))]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.txt")
    write_cases(fin, v, sets, pairs, 1, 0, [])
    subprocess.run([program, fin, fout], check=True)
    want = []
    exp = [G.expected(name, n, 40 + n, lu) for n, lu in shapes]
    for t in exp:
        want += transform_text(t)
    for a, b in pairs:
        want.append("S %016x" % int(np.float64(R.score(exp[a][:2], exp[b][:2])).view(np.uint64)))
    assert open(fout).read().split("\n")[:-1] == want


@pytest.mark.parametrize("n_entries", [1, 2, 70])
def test_database_session_matches_the_definition(program, tmp_path, n_entries):
    ops = G.session(n_entries); exp = G.session_expected(n_entries)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.txt")
    write_cases(fin, G.vocab(G.SESSION_VOCAB), [], [], n_entries, 4, ops)
    subprocess.run([program, fin, fout], check=True)
    want = []
    for op, e in zip(ops, exp):
        if op[0] == "query":
            want.append(ints("Q %d" % len(e[0]), e[0])); want += state_text(e[1])
    got = open(fout).read().split("\n")[:-1]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)


def test_host_program_rejects_a_malformed_vocabulary_and_times_a_pass(program, tmp_path):
    v = G.vocab("k2L1"); fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.txt")
    write_cases(fin, v, [(0, G.features("k2L1", 65, 1))], [], 1, 0, [])
    r = subprocess.run([program, fin, fout, "2"], check=True, capture_output=True, text=True)
    assert r.stdout.startswith("query_seconds") and r.stdout.split("\n")[1].startswith("seconds_per_pass transform ")
    raw = bytearray(open(fin, "rb").read()); raw[8:12] = struct.pack("<i", 1)       # scoring 1
    open(fin, "wb").write(bytes(raw))
    assert subprocess.run([program, fin, fout], capture_output=True).returncode == 3

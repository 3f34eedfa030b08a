"""GPU test: the adapter's corb::ORBVocabulary and corb::KeyFrameDatabase<KeyFrame, Frame> (corb-slam_amd/host/corb_adapter_orbslam.hpp), compiled with g++ -Wall
-Werror and driven by tests/host/kfdb_adapter_main.cpp on test doubles, give what the Python classes give on one scripted session (tests/bow_cases.py, 70 keyframes whose
BowVectors are computed once): the transform's sizes and self-score, every candidate list and the six fields of every keyframe after every query."""
import os
import struct
import subprocess
import numpy as np
import pytest
import bow_cases as G
from bow_cases import ints, state_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
CODES = {"set_bow": 0, "add": 1, "erase": 2, "clear": 3, "nb": 4, "query": 5}


def test_adapter_database_matches_the_python_classes(tmp_path, corb):
    exe = tmp_path / "kfdb_adapter_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "kfdb_adapter_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    n = 70
    ops = G.session(n, rebow=False)
    vtxt = tmp_path / "voc.txt"; vtxt.write_text(G.vocab(G.SESSION_VOCAB).to_text())
    blob = [struct.pack("<iii", n, 4, len(ops))]
    for op in ops:
        blob.append(struct.pack("<i", CODES[op[0]]))
        if op[0] == "set_bow":
            blob += [struct.pack("<ii", op[1], len(op[2])), np.ascontiguousarray(op[2], np.uint8).tobytes()]
        elif op[0] in ("add", "erase"):
            blob.append(struct.pack("<i", op[1]))
        elif op[0] == "nb":
            blob += [struct.pack("<i", op[1]), np.asarray(op[2], "<i4").tobytes()]
        elif op[0] == "query":
            blob += [struct.pack("<iiQfi", op[1], op[2], op[3], op[5], len(op[4])), np.asarray(op[4], "<i4").tobytes()]
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    got = subprocess.check_output([str(exe), str(vtxt), str(tmp_path / "in.bin")]).decode().split("\n")[:-1]

    voc = corb.Vocabulary.from_text(str(vtxt)); db = corb.KeyFrameDatabase(voc, n, 128)
    want = []; n_cand = 0
    for op in ops:
        if op[0] == "set_bow":
            t = voc.transform(op[2], 4); db.set_bow(op[1], t[0], t[1])
            want.append("B %d %d %d %016x" % (len(t[0]), len(t[2]), len(t[4]), int(db.score(op[1], [op[1]]).view(np.uint64)[0])))
        elif op[0] == "add":
            db.add(op[1])
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "clear":
            db.clear()
        elif op[0] == "nb":
            db.set_neighbours(op[1], op[2])
        else:
            c = db.detect(op[1], op[2], op[3], op[4], op[5])
            want.append(ints("Q %d" % len(c), c)); want += state_text(db.state()); n_cand += len(c) > 0
    assert len(got) == len(want) and n_cand > 20
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)
    db.close(); voc.close()

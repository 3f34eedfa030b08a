"""GPU test: the adapter's corb::adapt::LoopDetectT (corb-slam_amd/host/corb_adapter_orbslam.hpp) over corb::LoopDetector (corb_host.hpp), compiled with g++ -Wall
-Werror and driven by tests/host/loopdetect_main.cpp on test doubles, walks a seeded world of tests/loopdetect_cases.py as LoopClosing::Run walks its queue: all forty
keyframes inserted, DetectLoop() in chunks of eight until a loop is detected, mLastLoopKFid set as CorrectLoop sets it, and on.  Every line it prints -- outcome,
minScore's bits, candidates, the enough list, mpCurrentKF, the queue's length, the groups -- is the definition's (tests/loopdetect_reference.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bow_cases as B
import covis_cases as C
import loopdetect_cases as G
import loopdetect_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MAX_QUEUE = 8


def expected_lines(w):
    """the program's output from the definition alone, and the operations that produce it"""
    lc, m, bow = w.reference()
    index = {kid: i for i, kid in enumerate(w.ids)}
    ops = [(4 if j in w.not_live else 0, index[j]) for j in w.old_ids] + [(1, index[c]) for c in w.cur_ids]
    lines, pending = [], list(w.cur_ids)
    while pending:
        ops.append((2, 0))
        ret = False
        while pending and not ret:
            chunk, done = pending[:MAX_QUEUE], 0
            for kid in chunk:
                a = lc.DetectLoop(kid); done += 1
                bits = 0 if a["minScore"] is None else int(np.float32(a["minScore"]).view(np.uint32))
                cs = [w.slot[k] for k in a["candidates"]]
                lines.append("D %d %08x |%s |%s" % (a["outcome"], bits, "".join(" %d" % s for s in cs), "".join(" %d" % cs[i] for i in a["enough"])))
                ret = a["outcome"] == R.DETECTED
                if ret:
                    break
            pending = pending[done:]
            lines.append("R %d %d %d |%s" % (ret, lc.mpCurrentKF, len(pending), "".join(" %d" % k for k in lc.mvpEnoughConsistentCandidates)))
            lines += ["G %d%s" % (c, "".join(" %d" % s for s in sorted(w.slot[k] for k in g))) for g, c in lc.groups()]
        if ret:
            lc.mLastLoopKFid = lc.mpCurrentKF; ops.append((3, index[lc.mpCurrentKF]))
    return ops, lines, m


def test_adapter_walks_the_queue_as_the_definition_does(tmp_path, corb):
    exe = tmp_path / "loopdetect_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "loopdetect_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    w = G.walk(G.WALK_SEEDS[0])
    ops, want, m = expected_lines(w)
    assert sum(l.startswith("R 1") for l in want) >= 3 and sum(l.startswith("D") for l in want) == 40
    vtxt = tmp_path / "voc.txt"; vtxt.write_text(B.vocab(B.SESSION_VOCAB).to_text())
    index = {kid: i for i, kid in enumerate(w.ids)}
    a = C.arrays(m, [], sorted(m.mps))
    blob = [struct.pack("<9i", G.N_SLOTS, 96, len(w.ids), len(m.mps), len(a["obs_kf"]), G.MAX_CONNECTIONS, G.TH, MAX_QUEUE, len(ops))]
    for kid in w.ids:
        kf = m.kfs[kid]; words, values = w.words[kid]; best = [index[i] for i in w.neighbour_ids(m, kid)]
        meta = np.zeros(1, corb.KF_META_DTYPE); meta["id"] = kid; meta["nlevels"] = 8; meta["flags"] = 1 if kid in w.bad else 0
        meta["Tcw"] = np.eye(4, dtype=np.float32).reshape(16); meta["TcwGBA"] = np.eye(4, dtype=np.float32).reshape(16)
        blob += [struct.pack("<4i", w.slot[kid], len(kf.mp_ids), len(words), len(best)), meta.tobytes(), np.asarray(kf.mp_ids, "<u8").tobytes(),
                 np.asarray(words, "<u4").tobytes(), np.asarray(values, "<f8").tobytes(), np.asarray(best, "<i4").tobytes()]
    rec = np.zeros(len(m.mps), corb.MP_RECORD_DTYPE); rec["id"] = a["mp_ids"]; rec["n_obs"] = np.diff(a["obs_off"]); rec["ref_kf_id"] = G.CR.NO_ID
    blob += [rec.tobytes(), a["obs_off"].astype("<i4").tobytes(), a["obs_kf"].astype("<u8").tobytes(), a["obs_idx"].astype("<u4").tobytes()]
    blob += [struct.pack("<2i", *op) for op in ops]
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    p = subprocess.run([str(exe), str(vtxt), str(tmp_path / "in.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    got = p.stdout.decode().split("\n")[:-1]
    for k, (g, x) in enumerate(zip(got, want)):
        assert g == x, (k, g, x)
    assert len(got) == len(want)

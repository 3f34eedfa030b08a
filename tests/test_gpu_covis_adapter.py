"""GPU test: the adapter's corb::Covisibility<KeyFrame, Db> (corb-slam_amd/host/corb_adapter_orbslam.hpp), compiled with g++ -Wall -Werror and driven by
tests/host/covis_adapter_main.cpp on test doubles, answers what tests/covis_reference.py answers on one scripted session over a seeded map: every UpdateConnections
with its first parent and the keyframes reported to the place-recognition database, the four queries, KeyFrameCulling and the local window."""
import os
import struct
import subprocess
import numpy as np
import pytest

import covis_reference as R
import covis_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def ints(tag, v):
    return "%s %d" % (tag, len(v)) + "".join(" %d" % x for x in v)


def test_adapter_graph_matches_the_reference_restatement(tmp_path, corb):
    exe = tmp_path / "covis_adapter_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "covis_adapter_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    m = G.random_map(**G.RANDOM_MAPS["k20_id0"])
    a = G.arrays(m)
    order = [int(i) for i in a["kf_ids"]]; slot = {k: s for s, k in enumerate(order)}; mp_slot = {int(p): s for s, p in enumerate(a["mp_ids"])}
    sl = lambda ids: [-1 if i is None else slot[i] for i in ids]
    ops, want = [], []
    for k in sorted(m.kfs):
        ops.append((0, slot[k], 0, 0))
        first = R.update_connections(m, k)
        want += ["U %d" % (-1 if first is None else slot[first]), ints("db", [slot[k]] + sl(R.get_vector_covisibles(m, k)))]
    bad = next(k for k in sorted(m.kfs)[5:] if m.kfs[k].weights)
    ops.append((1, slot[bad], 0, 0)); R.erase_connections(m, bad)
    for k in sorted(m.kfs)[::2]:
        other = sorted(m.kfs)[3]
        w = sorted(x for _, x in m.kfs[k].ordered)[len(m.kfs[k].ordered) // 2] if m.kfs[k].ordered else 1
        ops.append((2, slot[k], w, slot[other]))
        want += [ints("V", sl(R.get_vector_covisibles(m, k))), ints("B1", sl(R.get_best_covisibles(m, k, 1))), ints("B10", sl(R.get_best_covisibles(m, k, 10))),
                 ints("W", sl(R.get_covisibles_by_weight(m, k, w))), "w %d" % R.get_weight(m, k, other)]
        for mono in (0, 1):
            ops.append((3, slot[k], mono, 35))
            c = R.keyframe_culling(m, k, bool(mono), 35.0)
            want.append("C %d" % len(c) + "".join(" %d:%d:%d:%d" % (slot[i], n, r, int(d)) for i, n, r, d in c))
        ops.append((4, slot[k], 0, 0))
        local, fixed, points = R.local_window(m, k)
        want.append("L %d %d %d" % (len(local), len(fixed), len(points)) + "".join(" %d" % x for x in sl(local) + sl(fixed) + [mp_slot[p] for p in points]))
    blob = [struct.pack("<6i", len(order), int(np.diff(a["feat_off"]).max()), len(a["mp_ids"]), 12, 0, len(ops)),
            a["kf_ids"].tobytes(), a["kf_bad"].astype("<u4").tobytes(), a["feat_off"].tobytes(), a["octave"].tobytes(), a["u_right"].tobytes(), a["depth"].tobytes(),
            a["mp_id"].tobytes(), a["mp_ids"].tobytes(), a["mp_bad"].astype("<u4").tobytes(), a["obs_off"].tobytes(), a["obs_kf"].tobytes(), a["obs_idx"].tobytes()]
    blob += [struct.pack("<4i", *op) for op in ops]
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    got = subprocess.check_output([str(exe), str(tmp_path / "in.bin")]).decode().split("\n")[:-1]
    assert len(got) == len(want) and len(want) > 100
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)

"""GPU tests of include/corb_trajectory.h: the per-frame log, KeyFrame::mTcp, and the three trajectory dumps on records, byte for byte against the definition
(tests/traj_reference.py).  Every comparison is equality of bytes: there is no tolerance.  The cyclic parent chain is checked on the CPU only
(tests/test_traj_reference.py, tests/test_traj_math_host.py)."""
import os
import subprocess

import numpy as np
import pytest
import traj_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pose(rng, near_pi=False, spread=3.0):
    return R.pose(R.rot(rng.normal(0, 1, 3), rng.uniform(2.9, 3.14) if near_pi else rng.uniform(0.05, 3.0)), rng.normal(0, spread, 3))


class Scene:
    """keyframes in a store with their spanning tree, a Trajectory over them, and the same state as the definition sees it (store, Tcp, times, entries)"""

    def __init__(self, corb, n_slots, capacity, sensor=1):
        self.corb = corb
        self.KF = corb.KeyFrameStore(n_slots, 4); self.MP = corb.MapPointStore(4, 4)
        self.g = corb.Covisibility(self.KF, self.MP, 8)
        self.traj = corb.Trajectory(self.g, capacity, sensor)
        self.store = [None] * n_slots
        self.Tcp = np.tile(np.eye(4, dtype=np.float32), (n_slots, 1, 1)); self.times = np.zeros(n_slots); self.entries = []

    def put(self, slot, kid, Tcw, parent=R.NO_ID, when=None):
        meta = np.zeros(1, self.corb.KF_META_DTYPE); meta["id"] = kid; meta["nlevels"] = 8; meta["Tcw"] = np.asarray(Tcw, np.float32).reshape(16)
        self.KF.put_batch(slot, meta, np.array([0, 1], np.int32), np.zeros(1, self.corb.KP_DTYPE))
        self.store[slot] = dict(id=kid, n=1, flags=0, Tcw=np.asarray(Tcw, np.float32).reshape(4, 4).copy(), parent=parent)
        self.g.SetTree(slot, parent, False, [])
        if when is not None:
            self.traj.set_keyframe_time(slot, when); self.times[slot] = when

    def set_parent(self, slot, parent):
        self.g.SetTree(slot, parent, False, []); self.store[slot]["parent"] = parent

    def cull(self, slot):
        """KeyFrame::SetBadFlag's end: mTcp, then mbBad"""
        self.traj.set_bad_pose(slot); self.Tcp[slot] = R.bad_pose(self.store, slot)
        self.KF.set_meta(slot, flags=R.KF_BAD); self.store[slot]["flags"] = R.KF_BAD

    def move(self, slot, Tcw):
        self.KF.set_meta(slot, Tcw=np.asarray(Tcw, np.float32).reshape(16)); self.store[slot]["Tcw"] = np.asarray(Tcw, np.float32).reshape(4, 4).copy()

    def append(self, ref_slot, Tcr, when, lost):
        self.traj.append(None, 0, ref_slot, Tcr, when, lost); R.append(self.entries, self.store, ref_slot, Tcr, when, lost)

    def append_copy(self, lost):
        self.traj.append(None, -1, 0, None, 0.0, lost); R.append_copy(self.entries, lost)

    def check_frames(self, origin, fmt, want_stats=None):
        rows, times, idx, st = self.traj.frames(origin, fmt)
        wr, wt, wi, ws = R.frames(self.entries, self.store, self.Tcp, origin, fmt)
        got = {k: getattr(st, k) for k in ws}
        assert got == ws, (got, ws)
        assert rows.shape == wr.shape and rows.tobytes() == wr.tobytes() and times.tobytes() == wt.tobytes() and idx.tolist() == wi.tolist()
        if want_stats is not None:
            assert {k: ws[k] for k in want_stats} == want_stats, ws
        return rows, times, idx, ws

    def check_tables(self):
        for s in range(len(self.store)):
            assert self.traj.get_tcp(s).tobytes() == self.Tcp[s].tobytes(), s
            assert self.traj.get_keyframe_time(s) == self.times[s]
        e = self.traj.get_entries()
        assert e.tobytes() == (np.array(self.entries, R.ENTRY_DTYPE).tobytes() if self.entries else b"")

    def close(self):
        self.traj.close(); self.g.close(); self.KF.close(); self.MP.close()


def _hand_case(corb, seed=5, capacity=8):
    """keyframes 1..4 in slots 3, 0, 2, 1, the tree 1 <- 2 <- 3 <- 4; 2 and 3 culled; six entries: references 1, 2, 3, 4, a lost one with a pose, a cur_slot = -1 copy"""
    rng = np.random.default_rng(seed)
    A = Scene(corb, 4, capacity)
    slot_of = {1: 3, 2: 0, 3: 2, 4: 1}
    for kid in (1, 2, 3, 4):
        A.put(slot_of[kid], kid, _pose(rng), parent=kid - 1 if kid > 1 else R.NO_ID, when=100.0 + kid / 3.0)
    A.cull(slot_of[3]); A.cull(slot_of[2])
    for kid in (1, 2, 3, 4):                                        # what a later optimisation leaves: Tcp keeps the poses of the culling
        A.move(slot_of[kid], _pose(rng))
    for k, kid in enumerate((1, 2, 3, 4)):
        A.append(slot_of[kid], _pose(rng, spread=0.2), 10.0 + 0.1 * k, False)
    A.append(slot_of[4], _pose(rng, spread=0.2), 10.5, True)
    A.append_copy(True)
    return A, slot_of


def test_hand_case(corb):
    A, slot_of = _hand_case(corb)
    assert not np.array_equal(A.store[slot_of[1]]["Tcw"], np.eye(4, dtype=np.float32))
    rows, _, idx, _ = A.check_frames(-1, R.KITTI, dict(n_entries=6, n_rows=6, n_lost_skipped=0, n_ref_gone=0, n_chain_broken=0, max_chain=2))
    assert idx.tolist() == [0, 1, 2, 3, 4, 5] and rows[5].tobytes() == rows[4].tobytes()
    _, times, idx, _ = A.check_frames(-1, R.TUM, dict(n_rows=4, n_lost_skipped=2, max_chain=2))
    assert idx.tolist() == [0, 1, 2, 3] and times.tolist() == [10.0, 10.1, 10.2, 10.3]
    A.check_frames(slot_of[1], R.KITTI); A.check_frames(slot_of[4], R.TUM)
    A.check_tables()
    assert not np.array_equal(A.Tcp[slot_of[2]], np.eye(4)) and np.array_equal(A.Tcp[slot_of[1]], np.eye(4)) and np.array_equal(A.Tcp[slot_of[4]], np.eye(4))
    A.close()


def test_append_parity_with_track_frame_finish(corb):
    """Tcr = NULL gives the entry the bytes corb_track_frame_finish(stage 1) returns for the same records, and so does an append with those bytes"""
    rng = np.random.default_rng(11)
    A = Scene(corb, 3, 4)
    A.put(1, 7, _pose(rng))
    rec = np.zeros(1, corb.MP_RECORD_DTYPE); rec["id"] = 100; rec["n_obs"] = 1
    A.MP.put(0, rec, np.array([0, 1], np.int32), np.array([7], np.uint64), np.array([0], np.uint32)); A.MP.build_index(0, 1)
    FR = corb.KeyFrameStore(2, 8)
    fm = np.zeros(1, corb.KF_META_DTYPE); fm["id"] = 900; fm["nlevels"] = 8; Tcw = _pose(rng); fm["Tcw"] = Tcw.reshape(16)
    FR.put_batch(1, fm, np.array([0, 3], np.int32), np.zeros(3, corb.KP_DTYPE), mp_id=np.full(3, corb.NO_MAP_POINT, np.uint64))
    Tcr = FR.TrackFrameFinish(1, A.KF, 1, A.MP, 1)
    assert Tcr.tobytes() == R.relative_pose(Tcw, A.store[1]["Tcw"]).tobytes()
    A.traj.append(FR, 1, 1, None, 2.5, False)
    A.traj.append(FR, 1, 1, Tcr, 2.5, False)
    A.traj.append(None, 0, 1, Tcr, 2.5, False)
    e = A.traj.get_entries()
    assert len(e) == 3 and e[0]["Tcr"].tobytes() == Tcr.tobytes() and e[0].tobytes() == e[1].tobytes() == e[2].tobytes()
    assert (int(e[0]["ref_id"]), int(e[0]["ref_slot"]), float(e[0]["timestamp"]), int(e[0]["lost"])) == (7, 1, 2.5, 0)
    with pytest.raises(corb.CorbError, match=r"\(-1\)"):
        A.traj.append(FR, 0, 1, None, 0.0, False)                 # an empty frame slot
    with pytest.raises(corb.CorbError, match=r"\(-1\)"):
        A.traj.append(FR, 1, 0, None, 0.0, False)                 # an empty reference slot
    assert len(A.traj.get_entries()) == 3
    FR.close(); A.close()


def test_quaternion_branches_on_the_device(corb):
    rng = np.random.default_rng(3)
    cases = R.branch_rotations()
    A = Scene(corb, 8, 2)
    ids = [50, 10, 40, 20, 30, 60]; slots = [4, 0, 6, 1, 7, 2]     # shuffled against each other; ids[5] is the bad one
    for k in range(6):
        axis, angle = cases[k % 5]
        A.put(slots[k], ids[k], R.pose(R.rot(axis, angle), rng.normal(0, 2, 3)), when=1000.0 + ids[k] * 0.125)
    A.KF.set_meta(slots[5], flags=R.KF_BAD); A.store[slots[5]]["flags"] = R.KF_BAD
    rows, times, kid = A.traj.keyframes()
    wr, wt, wi = R.keyframes(A.store, A.times)
    assert kid.tolist() == wi.tolist() == [10, 20, 30, 40, 50] and times.tobytes() == wt.tobytes() and rows.tobytes() == wr.tobytes()
    taken = set()
    for s in slots[:5]:
        M = A.store[s]["Tcw"][:3, :3].T
        taken.add(3 if float(M[0, 0]) + float(M[1, 1]) + float(M[2, 2]) > 0 else int(np.argmax(np.diag(M))))
    assert taken == {0, 1, 2, 3}
    with pytest.raises(corb.CorbError, match=r"\(-2\)"):
        A.traj.keyframes(cap=4)
    A.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_random(corb, seed):
    rng = np.random.default_rng(1000 + seed)
    n_kf, n_slots, n_entries = 64, 70, 500
    A = Scene(corb, n_slots, n_entries)
    slots = rng.permutation(n_slots)[:n_kf]; ids = np.sort(rng.choice(np.arange(1, 5000), n_kf, replace=False))
    for k in range(n_kf):                                           # each parent's id is below its child's
        A.put(int(slots[k]), int(ids[k]), _pose(rng, near_pi=k % 4 == 0), parent=int(ids[rng.integers(0, k)]) if k else R.NO_ID, when=float(rng.uniform(0, 1e9)))
    bad = [k for k in range(1, n_kf) if rng.uniform() < 0.4]
    for k in rng.permutation(bad):
        A.cull(int(slots[k]))
    for k in range(n_kf):                                           # as BA would perturb them
        T = A.store[int(slots[k])]["Tcw"].astype(np.float64) @ R.pose(R.rot(rng.normal(0, 1, 3), rng.normal(0, 0.01)), rng.normal(0, 0.02, 3)).astype(np.float64)
        A.move(int(slots[k]), T.astype(np.float32))
    for i in range(n_entries):
        if i and rng.uniform() < 0.05:
            A.append_copy(bool(rng.uniform() < 0.5))
        else:
            A.append(int(slots[rng.integers(0, n_kf)]), _pose(rng, near_pi=i % 7 == 0, spread=0.3), 1.4e9 + i / 30.0, bool(rng.uniform() < 0.10))
    live = [int(slots[k]) for k in range(1, n_kf) if k not in bad]
    for fmt in (R.KITTI, R.TUM):
        for origin in (-1, live[len(live) // 2]):
            ws = R.frames(A.entries, A.store, A.Tcp, origin, fmt)[3]
            assert ws["n_chain_broken"] == 0 and ws["n_ref_gone"] == 0 and ws["max_chain"] >= 1
            A.check_frames(origin, fmt)
    assert R.origin_slot(A.store) == int(slots[0])
    A.check_tables()
    rows, times, kid = A.traj.keyframes()
    wr, wt, wi = R.keyframes(A.store, A.times)
    assert kid.tolist() == wi.tolist() and len(kid) == n_kf - len(bad) and times.tobytes() == wt.tobytes() and rows.tobytes() == wr.tobytes()
    A.close()


def test_defined_failures_without_a_cycle(corb):
    rng = np.random.default_rng(21)
    for case in ("parent_none", "parent_slot_empty", "slot_overwritten"):
        A, slot_of = _hand_case(corb)
        base_rows, _, base_idx, _ = A.check_frames(-1, R.KITTI)
        if case == "parent_none":                                   # keyframe 2 (bad) loses its parent: entries 1 and 2 (references 2 and 3) walk into it
            A.set_parent(slot_of[2], R.NO_ID)
            rows, _, idx, _ = A.check_frames(-1, R.KITTI, dict(n_rows=4, n_chain_broken=2, n_ref_gone=0))
            gone = [1, 2]
        elif case == "parent_slot_empty":                           # keyframe 3 (bad) names a parent the store does not hold
            A.set_parent(slot_of[3], 999)
            rows, _, idx, _ = A.check_frames(-1, R.KITTI, dict(n_rows=5, n_chain_broken=1, n_ref_gone=0))
            gone = [2]
        else:                                                       # keyframe 4's slot receives another keyframe: entries 3, 4, 5 referred to it
            A.put(slot_of[4], 77, _pose(rng), parent=1)
            rows, _, idx, _ = A.check_frames(-1, R.KITTI, dict(n_rows=3, n_chain_broken=0, n_ref_gone=3))
            gone = [3, 4, 5]
        keep = [i for i in range(6) if i not in gone]
        assert idx.tolist() == keep and rows.tobytes() == base_rows[keep].tobytes()
        A.check_frames(-1, R.TUM)
        A.close()


def test_errors_leave_nothing_behind(corb):
    A, slot_of = _hand_case(corb, capacity=6)
    L = corb.load()
    before = A.traj.get_entries().tobytes()
    with pytest.raises(corb.CorbError, match=r"\(-2\)"):            # a full log
        A.traj.append(None, 0, slot_of[1], np.eye(4, dtype=np.float32), 1.0, False)
    with pytest.raises(corb.CorbError, match=r"\(-2\)"):
        A.traj.append(None, -1, 0, None, 0.0, True)
    assert A.traj.get_entries().tobytes() == before
    # an export with cap one short: *n is set and the arrays are untouched
    import ctypes as C
    for fmt, w, n_rows in ((R.KITTI, 12, 6), (R.TUM, 7, 4)):
        rows = np.full((8, w), 7.5, np.float32); times = np.full(8, -3.0); idx = np.full(8, -9, np.int32); n = C.c_int(-1); st = corb.TrajStats()
        rc = L.corb_traj_frames(A.traj.h, -1, fmt, rows.ctypes.data_as(C.c_void_p), times.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), n_rows - 1, C.byref(n), C.byref(st))
        assert rc == -2 and n.value == n_rows and st.n_rows == n_rows
        assert (rows == 7.5).all() and (times == -3.0).all() and (idx == -9).all()
    rows = np.full((4, 7), 7.5, np.float32); times = np.full(4, -3.0); ids = np.full(4, 5, np.uint64); n = C.c_int(-1)
    assert L.corb_traj_keyframes(A.traj.h, rows.ctypes.data_as(C.c_void_p), times.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), 1, C.byref(n)) == -2
    assert n.value == 2 and (rows == 7.5).all() and (times == -3.0).all() and (ids == 5).all()
    # set_bad_pose without a parent, and with a parent the store does not hold: Tcp stays
    marker = _pose(np.random.default_rng(1))
    A.traj.set_tcp(slot_of[1], marker); A.Tcp[slot_of[1]] = marker
    with pytest.raises(corb.CorbError, match=r"\(-1\)"):
        A.traj.set_bad_pose(slot_of[1])
    A.set_parent(slot_of[4], 999)
    with pytest.raises(corb.CorbError, match=r"\(-1\)"):
        A.traj.set_bad_pose(slot_of[4])
    A.set_parent(slot_of[4], 3)
    with pytest.raises(corb.CorbError, match=r"\(-1\)"):
        A.traj.frames(-1, 2)
    A.check_tables()
    # reset: the lists clear, the tables stay
    A.traj.reset(); A.entries = []
    assert len(A.traj.get_entries()) == 0
    rows, times, idx, st = A.traj.frames(-1, R.KITTI)
    assert len(rows) == 0 and (st.n_entries, st.n_rows) == (0, 0)
    with pytest.raises(corb.CorbError, match=r"\(-1\)"):            # cur_slot = -1 on an empty log
        A.traj.append(None, -1, 0, None, 0.0, True)
    assert len(A.traj.get_entries()) == 0
    A.check_tables()
    assert A.traj.get_keyframe_time(slot_of[2]) == 100.0 + 2 / 3.0 and not np.array_equal(A.traj.get_tcp(slot_of[2]), np.eye(4))
    A.append(slot_of[3], marker, 1.0, False)
    A.check_frames(-1, R.TUM, dict(n_rows=1, max_chain=2))
    A.close()


def test_files(corb, tmp_path):
    A, slot_of = _hand_case(corb)
    want = {}
    for kind, fmt in ((R.KITTI, R.KITTI), (R.TUM, R.TUM)):
        wr, wt, _, _ = R.frames(A.entries, A.store, A.Tcp, -1, fmt)
        want[kind] = R.format_rows(kind, wr, wt)
    wr, wt, _ = R.keyframes(A.store, A.times)
    want[R.KEYFRAME_TUM] = R.format_rows(R.KEYFRAME_TUM, wr, wt)
    assert want[R.KITTI].count(b"\n") == 6 and want[R.TUM].count(b"\n") == 4 and want[R.KEYFRAME_TUM].count(b"\n") == 2
    for again in range(2):
        paths = [str(tmp_path / ("%s_%d.txt" % (name, again))) for name in ("CameraTrajectory", "FrameTrajectory", "KeyFrameTrajectory")]
        A.traj.SaveTrajectoryKITTI(paths[0]); A.traj.SaveTrajectoryTUM(paths[1]); A.traj.SaveKeyFrameTrajectoryTUM(paths[2])
        for kind, p in zip((R.KITTI, R.TUM, R.KEYFRAME_TUM), paths):
            assert open(p, "rb").read() == want[kind], p
    with pytest.raises(corb.CorbError, match=r"\(-1\)"):
        A.traj.save(R.KITTI, str(tmp_path / "no_such_directory" / "x.txt"))
    A.close()


def test_the_mirror_program_writes_the_same_files(corb, tmp_path):
    """tests/host/traj_main.cpp: corb::Trajectory with the reference's three method names in a child process, on a scene handed over in a file"""
    exe = tmp_path / "traj_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "traj_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(77)
    ids = {1: 3, 2: 0, 3: 2, 4: 1}
    store = [None] * 5; times = np.zeros(5); blob = [np.array([5, 4, 2, 6, 1, -1], np.int32)]
    for kid, s in ids.items():
        meta = np.zeros(1, corb.KF_META_DTYPE); meta["id"] = kid; meta["nlevels"] = 8; T = _pose(rng); meta["Tcw"] = T.reshape(16)
        parent = kid - 1 if kid > 1 else R.NO_ID
        store[s] = dict(id=kid, n=1, flags=0, Tcw=T, parent=parent); times[s] = 5.0 + kid
        blob += [np.array([s, 0], np.int32), meta, np.array([parent], np.uint64), np.array([times[s]])]
    Tcp = np.tile(np.eye(4, dtype=np.float32), (5, 1, 1))
    for kid in (3, 2):
        s = ids[kid]; Tcp[s] = R.bad_pose(store, s); after = _pose(rng)
        store[s]["flags"] = R.KF_BAD; store[s]["Tcw"] = after
        blob += [np.array([s, 0], np.int32), after.reshape(16)]
    entries = []
    for k, kid in enumerate((1, 2, 3, 4, 4)):
        Tcr = _pose(rng, spread=0.2); lost = k == 4
        R.append(entries, store, ids[kid], Tcr, 20.0 + k, lost)
        blob += [np.array([ids[kid], lost], np.int32), Tcr.reshape(16), np.array([20.0 + k])]
    R.append_copy(entries, True)
    blob += [np.array([-1, 1], np.int32), np.zeros(16, np.float32), np.array([0.0])]
    path = tmp_path / "scene.bin"
    path.write_bytes(b"".join(np.ascontiguousarray(b).tobytes() for b in blob))
    out = [str(tmp_path / n) for n in ("k.txt", "t.txt", "f.txt")]
    p = subprocess.run([str(exe), str(path)] + out, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    want = []
    for fmt in (R.KITTI, R.TUM):
        wr, wt, _, ws = R.frames(entries, store, Tcp, -1, fmt)
        want.append(R.format_rows(fmt, wr, wt))
        assert "%c %d %d %d %d %d %d %d" % ("KT"[fmt], len(wr), ws["n_entries"], ws["n_rows"], ws["n_lost_skipped"], ws["n_ref_gone"], ws["n_chain_broken"], ws["max_chain"]) in p.stdout.decode().splitlines()
    wr, wt, _ = R.keyframes(store, times)
    want.append(R.format_rows(R.KEYFRAME_TUM, wr, wt))
    assert p.stdout.decode().splitlines()[2:] == ["F 2", "S 1 1 %d" % len(want[2])]
    for w, o in zip(want, out):
        assert open(o, "rb").read() == w, o

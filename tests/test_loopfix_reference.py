"""tests/loopfix_reference.py is the definition the device route of the map update after a global bundle adjustment is held against; here its readings are pinned by
cases small enough to work out by hand, its arithmetic is checked against plain 4x4 matrices on poses whose products are exact, and the seeded generators of
tests/loopfix_cases.py are checked to reach every event those readings are about.  CPU only."""
import copy
import itertools

import numpy as np
import pytest

import covis_reference as R
import localmap_reference as LR
import loopfix_cases as C
import loopfix_reference as XR

F32 = np.float32
L = C.LOOP_KF


def exact_pose(k):
    """a pose whose products with its like are exact in float32: a rotation that permutes the axes and a translation in eighths"""
    perms = list(itertools.permutations(range(3)))
    p = perms[k % 6]; T = np.zeros((4, 4), F32); T[3, 3] = 1
    for r in range(3):
        T[r, p[r]] = -1.0 if (k >> r) & 1 else 1.0
    if np.linalg.det(T[:3, :3].astype(np.float64)) < 0:           # a rotation, not a reflection
        T[2] = -T[2]
    T[:3, 3] = [(k * 3 % 17 - 8) / 8.0, (k * 5 % 23 - 11) / 8.0, (k * 7 % 13 - 6) / 8.0]
    return T


def tiny(children, marked, points=None):
    """children: {id: [child ids]}; marked: the ids that carry the mark; every keyframe gets exact poses numbered by its id"""
    m = R.Map()
    for k in children:
        kf = XR.pose(R.KeyFrame(k, [XR.NO_ID])); kf.Tcw = exact_pose(k); kf.TcwGBA = exact_pose(k + 31); kf.ba_global = L if k in marked else 0
        m.kfs[k] = kf
    for k, ch in children.items():
        LR.set_tree(m, k, None, False, ch)
    for pid, (ref, ba, bad) in (points or {}).items():
        mp = XR.point(R.MapPoint(pid, {}, bad=bad)); mp.pos = np.array([0.5, -1.25, 2.0], F32); mp.pos_gba = np.array([7.0, 8.0, 9.0], F32); mp.ba_global = ba; mp.ref_kf = ref
        m.mps[pid] = mp
    return m


def inv64(T):
    return np.linalg.inv(np.asarray(T, np.float64))


def test_the_convention_is_left_to_right_in_double_with_one_rounding():
    a = np.array([[1.0, 2.0 ** -30, -1.0, 0.0]] * 4, F32); b = np.array([[1.0] * 4] * 4, F32)
    assert XR.fmul(a, b)[0, 0] == F32(2.0 ** -30)               # float32 sums would lose the small term, double keeps it
    a = np.array([[1.0, 2.0 ** -60, -1.0, 0.0]] * 4, F32)
    assert XR.fmul(a, b)[0, 0] == 0.0                           # ... and left to right in double loses this one: (1 + 2^-60) - 1
    T = exact_pose(5); W = XR.pose_inverse(T)
    assert np.array_equal(W.astype(np.float64), inv64(T)) and np.array_equal(W[3], [0, 0, 0, 1])


def test_an_unmarked_chain_of_three_below_a_marked_keyframe():
    m = tiny({1: [2], 2: [3], 3: [4], 4: []}, marked={1})
    old = {k: kf.Tcw.copy() for k, kf in m.kfs.items()}; g1 = m.kfs[1].TcwGBA.copy()
    n = XR.gba_propagate(m, [1], L, 100)
    assert n["n_propagated"] == 3 and n["n_popped"] == 4 and n["n_reached"] == 4 and n["n_revisited"] == 0 and m.stats["unmarked_chain_of_three"] == 1
    want = g1.astype(np.float64)
    for k in (2, 3, 4):                                         # TcwGBA(child) = Tchild * inv(Tparent) * TcwGBA(parent), with the parent's pose before its pop
        want = old[k].astype(np.float64) @ inv64(old[k - 1]) @ want
        assert np.abs(m.kfs[k].TcwGBA - want).max() <= 1e-9 and m.kfs[k].ba_global == L
        assert np.array_equal(m.kfs[k].Tcw, m.kfs[k].TcwGBA) and np.array_equal(m.kfs[k].TcwBef, old[k])
    assert np.array_equal(m.kfs[1].Tcw, g1) and np.array_equal(m.kfs[1].TcwBef, old[1])


def test_a_child_listed_twice_is_popped_twice_and_ends_with_bef_equal_to_gba():
    m = tiny({1: [2, 3], 2: [4], 3: [4], 4: []}, marked={1, 2, 3, 4})          # ChangeParent(4: 2 -> 3) left the stale entry in the set of 2
    n = XR.gba_propagate(m, [1], L, 100)
    assert n["n_popped"] == 5 and n["n_reached"] == 4 and n["n_revisited"] == 1 and n["n_propagated"] == 0
    assert np.array_equal(m.kfs[4].TcwBef, m.kfs[4].TcwGBA) and np.array_equal(m.kfs[4].Tcw, m.kfs[4].TcwGBA)
    assert not np.array_equal(m.kfs[2].TcwBef, m.kfs[2].TcwGBA)


def test_of_two_listers_in_one_generation_the_earlier_queue_position_computes_the_pose():
    m = tiny({1: [5, 3], 3: [4], 5: [4], 4: []}, marked={1, 3, 5})             # children ascend: the queue is 1, 3, 5 -- 3 pops before 5
    t4 = m.kfs[4].Tcw.copy(); t3 = m.kfs[3].Tcw.copy(); g3 = m.kfs[3].TcwGBA.copy()
    n = XR.gba_propagate(m, [1], L, 100)
    assert n["n_propagated"] == 1 and n["n_popped"] == 5 and m.stats["same_generation_listers"] == 1
    want = t4.astype(np.float64) @ inv64(t3) @ g3.astype(np.float64)
    assert np.abs(m.kfs[4].TcwGBA - want).max() <= 1e-9
    assert np.array_equal(m.kfs[4].TcwBef, m.kfs[4].TcwGBA)     # popped twice


def test_an_unreached_subtree_keeps_its_poses_and_an_unmarked_origin_is_set_to_its_stale_gba():
    m = tiny({1: [2], 2: [], 7: [8], 8: []}, marked={2, 7})
    bef7 = exact_pose(70); m.kfs[7].TcwBef = bef7.copy()
    t7 = m.kfs[7].Tcw.copy(); t8 = m.kfs[8].Tcw.copy(); g8 = m.kfs[8].TcwGBA.copy(); g1 = m.kfs[1].TcwGBA.copy()
    n = XR.gba_propagate(m, [1], L, 100)
    assert n["n_popped"] == 2 and n["n_propagated"] == 0 and m.stats["unmarked_origin_pop"] == 1
    assert np.array_equal(m.kfs[1].Tcw, g1) and m.kfs[1].ba_global == 0         # SetPose with whatever mTcwGBA held; the mark is not given
    assert np.array_equal(m.kfs[7].Tcw, t7) and np.array_equal(m.kfs[7].TcwBef, bef7)
    assert np.array_equal(m.kfs[8].Tcw, t8) and np.array_equal(m.kfs[8].TcwGBA, g8) and m.kfs[8].ba_global == 0
    assert np.array_equal(m.kfs[8].TcwBef, np.eye(4, dtype=F32))                # the identity a fresh graph holds


def test_a_child_the_store_does_not_hold_is_skipped():
    m = tiny({1: [2], 2: []}, marked={1, 2})
    m.kfs[1].children.add(999)
    n = XR.gba_propagate(m, [1], L, 100)
    assert n["n_popped"] == 2 and m.stats["child_not_held"] == 1


def test_every_point_branch_once():
    pts = {10: (2, 0, True),        # bad: passed over
           11: (2, L, False),       # optimised by the global BA
           12: (None, 0, False),    # no reference keyframe
           13: (999, 0, False),     # a reference keyframe the store does not hold
           14: (8, 0, False),       # a reference keyframe without the mark
           15: (2, 0, False),       # moved with a reached keyframe
           16: (7, 0, False)}       # moved with a keyframe the walk never reached: its stored mTcwBefGBA
    m = tiny({1: [2], 2: [], 7: [], 8: []}, marked={1, 2, 7}, points=pts)
    m.kfs[7].TcwBef = exact_pose(70)
    t2 = m.kfs[2].Tcw.copy(); g2 = m.kfs[2].TcwGBA.copy(); t7 = m.kfs[7].Tcw.copy()
    p0 = np.array([0.5, -1.25, 2.0, 1.0])
    n = XR.gba_propagate(m, [1], L, 100)
    assert (n["n_points_set"], n["n_points_moved"], n["n_points_skipped"]) == (1, 2, 3)
    for k in ("point_bad", "point_set", "point_ref_not_held", "point_ref_unmarked", "point_moved", "point_ref_never_reached"):
        assert m.stats[k] >= 1, k
    for pid in (10, 12, 13, 14):
        assert np.array_equal(m.mps[pid].pos, p0[:3].astype(F32))
    assert np.array_equal(m.mps[11].pos, [7, 8, 9])
    assert np.abs(m.mps[15].pos - (inv64(g2) @ t2.astype(np.float64) @ p0)[:3]).max() <= 1e-9      # inv(Tcw after) * Tcw before * p
    assert np.abs(m.mps[16].pos - (inv64(t7) @ exact_pose(70).astype(np.float64) @ p0)[:3]).max() <= 1e-9


def snapshot(m):
    return ([(k, kf.Tcw.tobytes(), kf.TcwGBA.tobytes(), kf.TcwBef.tobytes(), kf.ba_global) for k, kf in sorted(m.kfs.items())],
            [(p, mp.pos.tobytes()) for p, mp in sorted(m.mps.items())])


def test_a_cyclic_child_set_is_a_capacity_error_with_nothing_changed():
    m = tiny({1: [2], 2: [3], 3: [1]}, marked={1}, points={10: (2, 0, False)})
    before = snapshot(m)
    with pytest.raises(XR.CapacityError):
        XR.gba_propagate(m, [1], L, XR.default_queue_cap(3))
    assert snapshot(m) == before
    m2, origins, _ = C.tree_map(**C.CYCLIC_CASE)
    before = snapshot(m2)
    with pytest.raises(XR.CapacityError):
        XR.gba_propagate(m2, origins, L, XR.default_queue_cap(len(m2.kfs) + 1))
    assert snapshot(m2) == before


def test_the_queue_cap_counts_every_entry():
    m = tiny({1: [2, 3], 2: [], 3: []}, marked={1, 2, 3})
    with pytest.raises(XR.CapacityError):
        XR.gba_propagate(copy.deepcopy(m), [1], L, 2)
    assert XR.gba_propagate(m, [1], L, 3)["n_popped"] == 3


def test_the_generators_reach_every_event():
    want = {"chain70": ("propagated", "unmarked_chain_of_three", "point_ref_never_reached"),
            "star300": ("propagated",),
            "random400": ("propagated", "unmarked_chain_of_three", "revisited", "same_generation_listers", "child_not_held", "point_ref_never_reached"),
            "two_origins": ("propagated", "revisited"),
            "unmarked_origin": ("unmarked_origin_pop", "propagated", "revisited")}
    every = ("point_bad", "point_set", "point_moved", "point_ref_not_held", "point_ref_unmarked")
    for name, kw in C.GBA_CASES.items():
        m, origins, order = C.tree_map(**kw)
        n = XR.gba_propagate(m, origins, L, 50000)
        for k in want[name] + every:
            assert m.stats[k] > 0, (name, k, dict(m.stats))
        assert n["n_popped"] == n["n_reached"] + n["n_revisited"] and sorted(order) == sorted(m.kfs)
    m, origins, _ = C.tree_map(**C.GBA_CASES["unmarked_origin"])
    assert m.kfs[origins[0]].ba_global != L and origins[0] in m.kfs[origins[1]].children


# ---- CorrectLoop's propagation ----------------------------------------------------------------------------------------------------------------------------------
def loop_tiny(kfs, points, cur, bad_points=(), exact=True):
    """kfs: {id: [point ids]}; points: {id: [observer ids]}; every other keyframe is covisible with `cur`.  Poses are exact ones numbered by the id."""
    m = R.Map()
    for k, ids in kfs.items():
        kf = XR.pose(R.KeyFrame(k, ids, octave=[1] * len(ids))); kf.Tcw = exact_pose(k % 1000) if exact else C.random_pose(np.random.default_rng(k)); kf.nlevels = 8
        m.kfs[k] = kf
    for p, obs in points.items():
        mp = XR.loop_point(R.MapPoint(p, {o: (kfs[o].index(p) if o in kfs and p in kfs[o] else 0) for o in obs}, bad=p in bad_points))
        mp.pos = np.array([0.5, -1.25, 2.0], F32); mp.ref_kf = min(obs) if obs else None
        m.mps[p] = mp
    for k in kfs:
        if k != cur:
            R.add_connection(m, m.kfs[cur], k, 20 + k % 7); R.add_connection(m, m.kfs[k], cur, 20 + k % 7)
    return m


def scw_of(T, s=1.0):
    T = np.asarray(T, np.float64)
    return np.concatenate([XR.quat_from_R(T[:3, :3]), T[:3, 3] * s, [s]])


def test_every_branch_of_the_quaternion_from_a_matrix():
    for q in ([0.1, 0.2, 0.3, 0.9], [0.9, 0.1, 0.2, 0.05], [0.1, 0.9, 0.2, -0.05], [0.2, 0.1, 0.9, 0.05]):      # trace > 0, then the x, y and z diagonal branches
        q = np.array(q) / np.linalg.norm(q)
        Rm = XR.quat_to_R(q)
        assert (Rm[0, 0] + Rm[1, 1] + Rm[2, 2] > 0) == (abs(q[3]) > 0.5)
        q2 = XR.quat_from_R(Rm)
        assert np.abs(q2 * np.sign(q2 @ q) - q).max() < 1e-15 and np.abs(XR.quat_to_R(q2) - Rm).max() < 1e-15
        v = np.array([0.3, -1.0, 2.0])
        assert np.abs(XR.quat_rot(q, v) - Rm @ v).max() < 1e-15
        assert np.abs(XR.quat_to_R(XR.quat_mul(q, q2)) - Rm @ XR.quat_to_R(q2)).max() < 1e-15


def test_a_point_held_by_three_members_is_corrected_by_the_smallest_id_not_by_the_current_keyframe():
    m = loop_tiny({7: [100], 3: [100], 5: [100, 101], 9: []}, {100: [3, 5, 7], 101: [5]}, cur=5)
    walk, co, nc, n = XR.correct_loop(m, 5, scw_of(exact_pose(40)))
    assert walk == [3, 5, 7, 9] and n == 2
    assert (m.mps[100].corrected_by, m.mps[100].corrected_ref) == (5, 3) and (m.mps[101].corrected_by, m.mps[101].corrected_ref) == (5, 5)
    assert m.stats["held_by_a_later_member"] == 2 and co.shape == (4, 8) and nc.shape == (4, 8)


def test_the_walk_is_in_ascending_id_wherever_the_current_keyframe_stands():
    for cur, ids in ((1000004, [3, 8, 1000004]), (2, [2, 1000001, 1000007])):
        m = loop_tiny({k: [100] for k in ids}, {100: ids}, cur=cur)
        walk, co, nc, n = XR.correct_loop(m, cur, scw_of(exact_pose(40)))
        assert walk == sorted(ids) and m.mps[100].corrected_ref == min(ids) and n == 1
        assert np.array_equal(co[walk.index(cur)], scw_of(exact_pose(40)))          # CorrectedSim3[mpCurrentKF] = mg2oScw itself
    m = loop_tiny({k: [100] for k in (1, 2, 3)}, {100: [1, 2, 3]}, cur=2)
    with pytest.raises(XR.CapacityError):
        XR.correct_loop(m, 2, scw_of(exact_pose(40)), cap=2)
    assert m.mps[100].corrected_by == 0 and np.array_equal(m.kfs[1].Tcw, exact_pose(1))


def test_already_corrected_bad_and_unresolved_points_are_passed_over():
    m = loop_tiny({4: [100, 101, 102, 777, XR.NO_ID]}, {100: [4], 101: [4], 102: [4]}, cur=4, bad_points={101})
    m.mps[100].corrected_by = 4; m.mps[100].corrected_ref = 55
    p = m.mps[100].pos.copy()
    walk, co, nc, n = XR.correct_loop(m, 4, scw_of(exact_pose(40)))
    assert n == 1 and m.mps[102].corrected_by == 4 and m.stats["already_corrected"] == 1
    assert np.array_equal(m.mps[100].pos, p) and m.mps[100].corrected_ref == 55 and np.array_equal(m.mps[101].pos, p) and m.mps[101].corrected_by == 0


def test_with_scale_one_the_correction_is_the_plain_matrix_one_and_the_pose_is_the_corrected_sim3():
    m = loop_tiny({3: [100], 5: [101], 8: [102]}, {100: [3], 101: [5], 102: [8]}, cur=5)
    old = {k: kf.Tcw.astype(np.float64) for k, kf in m.kfs.items()}
    Scw = exact_pose(40).astype(np.float64)
    walk, co, nc, n = XR.correct_loop(m, 5, scw_of(Scw))
    p0 = np.array([0.5, -1.25, 2.0, 1.0])
    for k, pid in ((3, 100), (5, 101), (8, 102)):
        Tnew = Scw if k == 5 else old[k] @ inv64(old[5]) @ Scw                     # Tic * Scw
        assert np.abs(m.kfs[k].Tcw - Tnew).max() <= 1e-9
        assert np.abs(m.mps[pid].pos - (inv64(Tnew) @ old[k] @ p0)[:3]).max() <= 1e-9
        assert np.abs(XR.quat_to_R(nc[walk.index(k)][:4]) - old[k][:3, :3]).max() <= 1e-12 and np.array_equal(nc[walk.index(k)][4:], list(old[k][:3, 3]) + [1.0])


def test_the_pose_is_R_and_t_over_s():
    m = loop_tiny({5: []}, {}, cur=5, exact=False)
    S = C.loop_scw(m, 5, 9, 0.8)
    XR.correct_loop(m, 5, S)
    assert np.abs(m.kfs[5].Tcw[:3, :3] - XR.quat_to_R(S[:4])).max() < 1e-7 and np.abs(m.kfs[5].Tcw[:3, 3] - S[4:7] / 0.8).max() < 1e-6
    assert np.array_equal(m.kfs[5].Tcw[3], [0, 0, 0, 1])


def test_update_normal_and_depth_meets_the_poses_of_the_middle_of_the_walk():
    """100: its observer 3 precedes the corrector 5 (3 is a member that no longer holds it); 101: its observer 8 follows the corrector 5; 102: the observer is the corrector"""
    from oracle import pyorc
    kfs = {3: [XR.NO_ID], 5: [100, 101, 102], 8: [101], 9: [XR.NO_ID]}
    m = loop_tiny(kfs, {100: [3, 5], 101: [5, 8], 102: [5]}, cur=9, exact=False)
    for p in (100, 101, 102):
        m.mps[p].ref_kf = 5
    old = {k: kf.Tcw.copy() for k, kf in m.kfs.items()}
    S = C.loop_scw(m, 9, 3, 1.25)
    XR.correct_loop(m, 9, S, scale_factor=1.2)
    assert m.stats["observer_before"] == 1 and m.stats["observer_after"] == 1 and m.stats["observer_is_corrector"] >= 3
    new = {k: kf.Tcw for k, kf in m.kfs.items()}
    for pid, poses in ((100, {3: new[3], 5: old[5]}), (101, {5: old[5], 8: old[8]}), (102, {5: old[5]})):
        mp = m.mps[pid]
        keys = np.zeros(3, [("octave", "<i4")]); keys["octave"] = 1
        d = dict(bad=False, obs=dict(mp.obs), ref=5, pos=mp.pos)
        pyorc.map_point_update_normal_and_depth(d, {k: dict(T=T, keys=keys, nlevels=8) for k, T in poses.items()}, 1.2)
        assert np.array_equal(mp.normal, d["normal"]) and mp.max_distance == d["max_distance"] and mp.min_distance == d["min_distance"]
    assert not np.array_equal(new[3], old[3])
    m2 = loop_tiny(kfs, {100: [3, 5], 101: [5, 8], 102: [5]}, cur=9, exact=False)
    XR.correct_loop(m2, 9, S, scale_factor=0.0)
    assert np.array_equal(m2.mps[100].normal, np.zeros(3)) and np.array_equal(m2.mps[100].pos, m.mps[100].pos)      # scale_factor 0: the three fields are left alone


def test_the_loop_generators_reach_every_event():
    seen = set(); sizes = []
    for i, seed in enumerate(C.LOOP_SEEDS):
        m, cur = C.loop_map(seed, cur=C.LOOP_CURS[i % 3])
        walk, co, nc, n = XR.correct_loop(m, cur, C.loop_scw(m, cur, seed, C.LOOP_SCALES[i % 3]), 1.2)
        for k in ("corrected_by_a_neighbour", "held_by_a_later_member", "already_corrected", "observer_before", "observer_after", "observer_is_corrector", "bad_point"):
            assert m.stats[k] > 0, (seed, k)
        sizes.append(len(walk) - 1); seen.add(walk.index(cur) == 0); seen.add(walk.index(cur) == len(walk) - 1)
        assert 5 <= len(walk) - 1 <= 8 and 70 <= len(m.mps) <= 130 and max(len(p.obs) for p in m.mps.values()) <= 6
    assert len(seen) == 2 and max(sizes) >= 6


def test_the_calls_are_declared_exported_and_the_abi_version_stays_6():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "corb_accel.h")).read()
    assert re.search(r"#define CORB_ABI_VERSION 6\b", hdr)                   # no existing structure changed
    assert re.search(r"\bint corb_loop_correct_store\(CorbCovis\* g, int cur_slot, const double\* Scw", hdr)
    assert re.search(r"\bint corb_gba_propagate_store\(CorbCovis\* g, const int32_t\* origin_slots, int n_origins, uint64_t loop_kf, int queue_cap, CorbGbaPropagation\* out\);", hdr)
    fields = re.search(r"typedef struct CorbGbaPropagation \{(.*?)\} CorbGbaPropagation;", hdr, re.S).group(1)
    names = [n.strip() for n in fields.replace("int32_t", "").replace(";", "").split(",")]
    import corbload
    corb = corbload.load_pkg()
    assert names == [k for k, _ in corb.GbaPropagation._fields_] == list(XR.gba_propagate(R.Map(), [], 1, 8))
    for name in ("corb_loop_correct_store", "corb_fuse_sim3_store", "corb_gba_propagate_store", "corb_covis_set_pose_before_gba", "corb_covis_get_pose_before_gba"):
        assert name in corb.EXPORTS and re.search(r"\bint %s\(" % name, hdr)
    lib = os.path.join(root, "corb-slam_amd", "libcorb_accel.so")
    if os.path.exists(lib):
        import ctypes
        assert all(hasattr(ctypes.CDLL(lib), name) for name in corb.EXPORTS[-5:])


# ---- Fuse with Scw: the action layer ------------------------------------------------------------------------------------------------------------------------------
def test_two_points_compete_for_an_empty_feature_and_a_bad_point_in_a_feature_is_counted_and_left():
    NONE = XR.NO_ID
    held = [NONE, 900, 901, 999, NONE]                           # feature 1 holds a good point, 2 a bad one, 3 an id without a record
    ids = [10, 11, 12, 13, 14, 15]
    slot_of = {10: 0, 11: 1, 12: 2, 13: 3, 14: 4, 15: 5, 900: 6, 901: 7}
    best = [0, 0, 1, 2, 3, -1]
    h, act, rep, lists = XR.fuse_sim3_actions(best, held, ids, slot_of, {901}, [[(3, i)] for i in range(6)], 7)
    assert act.tolist() == [1, 2, 2, 4, 2, 0] and rep.tolist() == [-1, 0, 6, -1, -1, -1]          # the second point meets the first one in the feature: Replace pending
    assert [int(x) for x in h] == [10, 900, 901, 999, NONE] and lists[0] == [(3, 0), (7, 0)] and lists[1] == [(3, 1)]
    assert XR.fuse_sim3_takes_part([10, 900, 11], [False, False, True], held).tolist() == [True, False, False]

"""Definition, in plain Python / numpy, of what the calls of include/corb_trajectory.h compute: the entry Tracking::Track appends (corbslam_client/src/Tracking.cc:485-504),
KeyFrame::mTcp (KeyFrame.cc:666), the loops of System::SaveTrajectoryTUM (System.cc:281-306), SaveTrajectoryKITTI (:376-400) and SaveKeyFrameTrajectoryTUM (:326-341),
and the text their streams write.

The rules: a product of CV_32F matrices is cv::gemm (tests/trackframe_reference.py: a double sum over k ascending, one rounding, all sixteen elements the product's),
the product with the identity at the start of the walk included; GetPoseInverse and the camera centre as there; Converter::toQuaternion is Eigen::Quaterniond(Matrix3d)
on the floats widened to double, every operation one IEEE double operation, each component rounded to float once, no normalisation.

A store is a list over slots of None (never filled) or a dict(id, n, flags, Tcw [4][4] float32, parent: an id or NO_ID).  A slot with n <= 0 is not a keyframe; an id
is resolved to the lowest slot that holds it.  Where the reference dereferences NULL or never returns, the entry gives no row and is counted (the three cases below)."""
import numpy as np

from trackframe_reference import camera_centre, gemm4, pose_inverse, relative_pose  # noqa: F401

NO_ID = 0xFFFFFFFFFFFFFFFF
KF_BAD = 1
KITTI, TUM, KEYFRAME_TUM = 0, 1, 2
CHAIN_BROKEN = -1
ENTRY_DTYPE = np.dtype([("Tcr", np.float32, 16), ("ref_id", np.uint64), ("timestamp", np.float64), ("ref_slot", np.int32), ("lost", np.int32)])


def quaternion(M):
    """Converter::toQuaternion(M) (Converter.cc:137-149) -> x y z w as float32"""
    m = np.asarray(M, np.float32).reshape(3, 3).astype(np.float64)
    q = np.zeros(4, np.float64)
    t = (m[0, 0] + m[1, 1]) + m[2, 2]
    if t > 0:
        t = np.sqrt(t + np.float64(1.0)); q[3] = np.float64(0.5) * t; t = np.float64(0.5) / t
        q[0] = (m[2, 1] - m[1, 2]) * t; q[1] = (m[0, 2] - m[2, 0]) * t; q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(((m[i, i] - m[j, j]) - m[k, k]) + np.float64(1.0)); q[i] = np.float64(0.5) * t; t = np.float64(0.5) / t
        q[3] = (m[k, j] - m[j, k]) * t; q[j] = (m[j, i] + m[i, j]) * t; q[k] = (m[k, i] + m[i, k]) * t
    return q.astype(np.float32)


def walk(slot, flags, parent_slot, Tcp, Tcw, n_slots, Two):
    """(steps, Trw): Trw = I; while(pKF->isBad()) { Trw = Trw*pKF->mTcp; pKF = pKF->GetParent(); } Trw = Trw*pKF->GetPose()*Two, as a for loop bounded by the slot
    count.  (CHAIN_BROKEN, None): a bad keyframe without a held parent, or more steps than the store has slots (a cyclic parent chain)"""
    A = np.eye(4, dtype=np.float32); s = int(slot); steps = 0
    for it in range(n_slots + 1):
        if not (int(flags[s]) & KF_BAD):
            return steps, gemm4(gemm4(A, Tcw[s]), Two)
        if it == n_slots:
            break
        A = gemm4(A, Tcp[s]); s = int(parent_slot[s]); steps += 1
        if s < 0 or s >= n_slots:
            return CHAIN_BROKEN, None
    return CHAIN_BROKEN, None


def row_kitti(Tcr, Trw):
    Tcw = gemm4(Tcr, Trw)
    row = np.zeros((3, 4), np.float32); row[:, :3] = Tcw[:3, :3].T; row[:, 3] = camera_centre(Tcw)      # twc = -Rwc*tcw: negation commutes with the one rounding
    return row.reshape(12)


def row_tum(Tcr, Trw):
    return row_keyframe(gemm4(Tcr, Trw))


def row_keyframe(Tcw):
    Tcw = np.asarray(Tcw, np.float32).reshape(4, 4)
    return np.concatenate([camera_centre(Tcw), quaternion(Tcw[:3, :3].T)]).astype(np.float32)


# ---- the store as plain arrays ----
def held(rec):
    return rec is not None and rec["n"] > 0


def slot_of(store, kid):
    if kid == NO_ID:
        return -1
    for s, r in enumerate(store):
        if held(r) and int(r["id"]) == int(kid):
            return s
    return -1


def arrays(store):
    """flags, parent_slot (-1: none, or not held), Tcw [S][4][4] of a store"""
    S = len(store)
    flags = np.zeros(S, np.uint32); ps = np.full(S, -1, np.int32); Tcw = np.zeros((S, 4, 4), np.float32)
    for s, r in enumerate(store):
        if r is None:
            continue
        flags[s] = r["flags"]; Tcw[s] = np.asarray(r["Tcw"], np.float32).reshape(4, 4)
        if held(r):
            ps[s] = slot_of(store, r["parent"])
    return flags, ps, Tcw


def origin_slot(store):
    """vpKFs[0] after sort(KeyFrame::lId): the held record of the smallest id without KF_BAD (ties: the lowest slot); -1 if none"""
    best = -1
    for s, r in enumerate(store):
        if held(r) and not (r["flags"] & KF_BAD) and (best < 0 or int(r["id"]) < int(store[best]["id"])):
            best = s
    return best


def bad_pose(store, slot):
    """mTcp = Tcw*mpParent->GetPoseInverse() (KeyFrame.cc:666); None where the call answers CORB_ERR_ARG"""
    r = store[slot]
    if not held(r):
        return None
    p = slot_of(store, r["parent"])
    if p < 0:
        return None
    return gemm4(r["Tcw"], pose_inverse(store[p]["Tcw"]))


def append(entries, store, ref_slot, Tcr, timestamp, lost):
    """the `if` branch of Tracking.cc:485-504 onto a list of entries"""
    e = np.zeros((), ENTRY_DTYPE)
    e["Tcr"] = np.asarray(Tcr, np.float32).reshape(16); e["ref_id"] = store[ref_slot]["id"]; e["timestamp"] = timestamp; e["ref_slot"] = ref_slot; e["lost"] = 1 if lost else 0
    entries.append(e)


def append_copy(entries, lost):
    """the `else` branch: the last entry again with the new lost flag"""
    e = entries[-1].copy(); e["lost"] = 1 if lost else 0
    entries.append(e)


def frames(entries, store, Tcp, origin, fmt):
    """corb_traj_frames: (rows [n][12 | 7] float32, times [n], entry_index [n], stats dict)"""
    S = len(store)
    flags, ps, Tcw = arrays(store)
    o = origin_slot(store) if origin < 0 else origin
    st = dict(n_entries=len(entries), n_rows=0, n_lost_skipped=0, n_ref_gone=0, n_chain_broken=0, max_chain=0)
    rows, times, idx = [], [], []
    if len(entries) == 0:
        return np.zeros((0, 12 if fmt == KITTI else 7), np.float32), np.zeros(0), np.zeros(0, np.int32), st
    assert o >= 0 and held(store[o]), "no origin"
    Two = pose_inverse(Tcw[o])
    cache = {}
    for i, e in enumerate(entries):
        if fmt == TUM and e["lost"]:
            st["n_lost_skipped"] += 1; continue
        s = int(e["ref_slot"])
        if s < 0 or s >= S or not held(store[s]) or int(store[s]["id"]) != int(e["ref_id"]):
            st["n_ref_gone"] += 1; continue
        if s not in cache:
            cache[s] = walk(s, flags, ps, Tcp, Tcw, S, Two)
        steps, Trw = cache[s]
        if steps < 0:
            st["n_chain_broken"] += 1; continue
        st["max_chain"] = max(st["max_chain"], steps)
        rows.append(row_kitti(e["Tcr"], Trw) if fmt == KITTI else row_tum(e["Tcr"], Trw)); times.append(float(e["timestamp"])); idx.append(i)
    st["n_rows"] = len(rows)
    w = 12 if fmt == KITTI else 7
    return np.array(rows, np.float32).reshape(-1, w), np.array(times, np.float64), np.array(idx, np.int32), st


def keyframes(store, kf_times):
    """corb_traj_keyframes: (rows [n][7], times [n], ids [n]) over the held records without KF_BAD in ascending (id, slot)"""
    live = sorted((int(r["id"]), s) for s, r in enumerate(store) if held(r) and not (r["flags"] & KF_BAD))
    rows = np.array([row_keyframe(store[s]["Tcw"]) for _, s in live], np.float32).reshape(-1, 7)
    return rows, np.array([kf_times[s] for _, s in live], np.float64), np.array([k for k, _ in live], np.uint64)


# ---- the text: `f << fixed << setprecision(p) << float` is %.pf of the value widened to double ----
def format_rows(kind, rows, times=None):
    w = 12 if kind == KITTI else 7; p = 7 if kind == KEYFRAME_TUM else 9
    rows = np.asarray(rows, np.float32).reshape(-1, w)
    out = []
    for r in range(len(rows)):
        vals = ["%.*f" % (p, float(v)) for v in rows[r]]
        if kind != KITTI:
            vals.insert(0, "%.6f" % float(times[r]))
        out.append(" ".join(vals) + "\n")
    return "".join(out).encode()


# ---- rotations for the tests ----
def rot(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def quaternion_closed_form(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    return np.concatenate([a * np.sin(angle / 2), [np.cos(angle / 2)]])


def pose(R, t):
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return T.astype(np.float32)


def branch_rotations():
    """(axis, angle) of the five quaternion cases: the identity, 170 degrees about x, y, z (one per non-trace branch), and a trace just above 0 (trace = 1 + 2 cos)"""
    d = np.deg2rad
    return [((0, 0, 1), 0.0), ((1, 0, 0), d(170.0)), ((0, 1, 0), d(170.0)), ((0, 0, 1), d(170.0)), ((1, 2, 3), np.arccos(-0.5 + 1e-4))]

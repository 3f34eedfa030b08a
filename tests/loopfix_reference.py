"""The map update that follows a global bundle adjustment (RunGlobalBundleAdjustment, corbslam_server/src/GlobalOptimize.cpp:463-532 = corbslam_client/src/
LoopClosing.cc:684-753), restated as the definition the device route (corb_gba_propagate_store) is compared with bit for bit.  It works on the containers of
tests/covis_reference.py / tests/localmap_reference.py, with these attributes added (pose() / point() below give them their defaults):

  kf.Tcw, kf.TcwGBA, kf.TcwBef   4x4 float32: GetPose(), mTcwGBA, mTcwBefGBA.  mTcwBefGBA starts as the identity (the reference leaves it uninitialised, KeyFrame.cc:62)
  kf.ba_global                   mnBAGlobalForKF
  mp.pos, mp.pos_gba             float32[3]: mWorldPos, mPosGBA;  mp.ba_global: mnBAGlobalForKF;  mp.ref_kf: mpRefKF's id or None

Arithmetic convention (csrc/loopfix_internal.h states it for the kernels): every product of float matrices and vectors the reference makes on cv::Mat is computed per
entry as the exact products summed in float64, left to right, and rounded to float32 once; `A*x + b` is that product followed by one float32 add; SetPose's
Rwc = Rcw^T, Ow = -(Rwc*tcw) follow the same rule.  A product of two float32 is exact in float64, so numpy's `s + a*b` rounds as the device's fused form does.

Map.stats counts the events the seeded generators of tests/loopfix_cases.py must reach (tests/test_loopfix_reference.py asserts them)."""
import numpy as np

import localmap_reference as LR

NO_ID = LR.NO_ID
F32 = np.float32


class CapacityError(Exception):
    """the walk needs more queue entries than queue_cap: nothing was changed"""


def fmul(A, B):
    """A * B in the convention: float32 in, float64 left-to-right sums, one rounding"""
    A = np.asarray(A, F32).astype(np.float64); B = np.asarray(B, F32).astype(np.float64)
    vec = B.ndim == 1
    if vec:
        B = B[:, None]
    s = A[:, 0:1] * B[0:1, :]
    for k in range(1, A.shape[1]):
        s = s + A[:, k:k + 1] * B[k:k + 1, :]
    s = s.astype(F32)
    return s[:, 0] if vec else s


def affine(R, t, x):
    """R*x + t: the product, then one float32 add"""
    return (fmul(R, x) + np.asarray(t, F32)).astype(F32)


def pose_inverse(T):
    """Twc as KeyFrame::SetPose leaves it (KeyFrame.cc:78-94)"""
    T = np.asarray(T, F32)
    W = np.eye(4, dtype=F32)
    W[:3, :3] = T[:3, :3].T
    W[:3, 3] = -fmul(W[:3, :3], T[:3, 3])
    return W


def pose(kf):
    LR.tree(kf)
    if not hasattr(kf, "Tcw"):
        kf.Tcw = np.eye(4, dtype=F32); kf.TcwGBA = np.eye(4, dtype=F32); kf.ba_global = 0
    if not hasattr(kf, "TcwBef"):
        kf.TcwBef = np.eye(4, dtype=F32)
    return kf


def point(mp):
    if not hasattr(mp, "pos"):
        mp.pos = np.zeros(3, F32); mp.pos_gba = np.zeros(3, F32); mp.ba_global = 0; mp.ref_kf = None
    return mp


def default_queue_cap(n_slots):
    return 4 * n_slots + 64


def gba_propagate(m, origins, loop_kf, queue_cap, point_ids=None):
    """:463-532.  origins: ids of held keyframes (mvpKeyFrameOrigins); point_ids: the points GetAllMapPointsFromMap() returns (default: all of m.mps).  Returns the
    counts of CorbGbaPropagation as a dict.  Raises CapacityError, with the map untouched, when the queue would hold more than queue_cap entries in all."""
    # the reference never ends on a cyclic child set, so the walk is first made on the marks and the sets alone
    for kf in m.kfs.values():
        pose(kf)
    queue = list(origins)
    if len(queue) > queue_cap:
        raise CapacityError
    front = 0
    while front < len(queue):
        kf = m.kfs[queue[front]]
        for cid in sorted(kf.children):
            if cid not in m.kfs:
                continue
            if len(queue) >= queue_cap:
                raise CapacityError
            queue.append(cid)
        front += 1
    # the walk itself (:464-488)
    n = dict(n_popped=0, n_reached=0, n_propagated=0, n_revisited=0, n_points_set=0, n_points_moved=0, n_points_skipped=0)
    popped = set()
    queue = list(origins); front = 0
    gen = [0] * len(queue)                                      # generation of every queue entry (the device walks generation by generation)
    lister = {}; depth = {}
    while front < len(queue):
        kid = queue[front]; kf = m.kfs[kid]
        if kf.ba_global != loop_kf:
            m.stats["unmarked_origin_pop"] += 1                 # only an origin is ever popped without the mark
        Twc = pose_inverse(kf.Tcw)                              # :470
        for cid in sorted(kf.children):                         # :471: std::set<KeyFrame*> in the reference, ascending id here
            if cid not in m.kfs:                                # GetChilds() drops what the cache does not hold (KeyFrame.cc:523-532)
                m.stats["child_not_held"] += 1
                continue
            ch = pose(m.kfs[cid])
            if ch.ba_global != loop_kf:                         # :474
                ch.TcwGBA = fmul(fmul(ch.Tcw, Twc), kf.TcwGBA)  # :476-477
                ch.ba_global = loop_kf                          # :478
                n["n_propagated"] += 1
                lister[cid] = (gen[front], kid); depth[cid] = depth.get(kid, 0) + 1
                m.stats["propagated"] += 1
                if depth[cid] >= 3:
                    m.stats["unmarked_chain_of_three"] += 1
            elif cid in lister and lister[cid] != (gen[front], kid) and lister[cid][0] == gen[front]:
                m.stats["same_generation_listers"] += 1
            queue.append(cid); gen.append(gen[front] + 1)       # :481, marked or not
        kf.TcwBef = kf.Tcw.copy()                               # :484
        kf.Tcw = kf.TcwGBA.copy()                               # :485
        if kid in popped:
            n["n_revisited"] += 1; m.stats["revisited"] += 1
        popped.add(kid)
        front += 1
    n["n_popped"] = len(queue); n["n_reached"] = len(popped)
    # the points (:492-532)
    for pid in (sorted(m.mps) if point_ids is None else point_ids):
        mp = point(m.mps[pid])
        if mp.bad:                                              # :498
            m.stats["point_bad"] += 1
            continue
        if mp.ba_global == loop_kf:                             # :501-506
            mp.pos = mp.pos_gba.copy(); n["n_points_set"] += 1; m.stats["point_set"] += 1
            continue
        ref = m.kfs.get(mp.ref_kf) if mp.ref_kf is not None else None      # :510-512
        if ref is None:
            m.stats["point_ref_not_held"] += 1; n["n_points_skipped"] += 1
            continue
        if pose(ref).ba_global != loop_kf:                      # :514
            m.stats["point_ref_unmarked"] += 1; n["n_points_skipped"] += 1
            continue
        if mp.ref_kf not in popped:
            m.stats["point_ref_never_reached"] += 1             # its stored mTcwBefGBA is used as it is
        Xc = affine(ref.TcwBef[:3, :3], ref.TcwBef[:3, 3], mp.pos)         # :518-520
        Twc = pose_inverse(ref.Tcw)                             # :523
        mp.pos = affine(Twc[:3, :3], Twc[:3, 3], Xc)            # :527
        n["n_points_moved"] += 1; m.stats["point_moved"] += 1
    return n


# ---- CorrectLoop's propagation (GlobalOptimize.cpp:253-338 = LoopClosing.cc:436-522) -------------------------------------------------------------------------------
# The g2o::Sim3 parts are float64 in the operation order of G/types/sim3.h and Eigen (csrc/sim3_math.h, csrc/ba_math.h); a Sim3 is (q = x y z w, t, s).
# Added attributes: mp.corrected_by, mp.corrected_ref (mnCorrectedByKF, mnCorrectedReference), mp.normal, mp.min_distance, mp.max_distance; kf.nlevels (8).

def quat_from_R(R):
    """Eigen::Quaterniond(Matrix3d): the trace branch, or the branch of the largest diagonal entry"""
    R = np.asarray(R, np.float64); q = np.zeros(4)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t
        q[0] = (R[2, 1] - R[1, 2]) * t; q[1] = (R[0, 2] - R[2, 0]) * t; q[2] = (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t; t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t; q[j] = (R[j, i] + R[i, j]) * t; q[k] = (R[k, i] + R[i, k]) * t
    return q


def quat_rot(q, v):
    """Eigen's q * v: uv = q.vec x v; uv += uv; v + w * uv + q.vec x uv"""
    uv = np.array([q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]])
    uv = uv + uv
    return np.array([v[0] + q[3] * uv[0] + (q[1] * uv[2] - q[2] * uv[1]),
                     v[1] + q[3] * uv[1] + (q[2] * uv[0] - q[0] * uv[2]),
                     v[2] + q[3] * uv[2] + (q[0] * uv[1] - q[1] * uv[0])])


def quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def quat_to_R(q):
    """Eigen's toRotationMatrix"""
    tx, ty, tz = 2 * q[0], 2 * q[1], 2 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def sim3_from_pose(T):
    """g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0)"""
    T = np.asarray(T, F32).astype(np.float64)
    return quat_from_R(T[:3, :3]), T[:3, 3].copy(), 1.0


def sim3_mul(a, b):
    return quat_mul(a[0], b[0]), a[2] * quat_rot(a[0], b[1]) + a[1], a[2] * b[2]


def sim3_inv(a):
    qc = np.array([-a[0][0], -a[0][1], -a[0][2], a[0][3]])
    return qc, quat_rot(qc, (-1. / a[2]) * a[1]), 1. / a[2]


def sim3_map(a, x):
    return a[2] * quat_rot(a[0], x) + a[1]


def sim3_vec(a):
    return np.concatenate([a[0], a[1], [a[2]]])


def sim3_load(v):
    v = np.asarray(v, np.float64)
    return v[:4].copy(), v[4:7].copy(), float(v[7])


def loop_point(mp):
    point(mp)
    if not hasattr(mp, "corrected_by"):
        mp.corrected_by = 0; mp.corrected_ref = 0
    if not hasattr(mp, "normal"):
        mp.normal = np.zeros(3, F32); mp.min_distance = F32(0); mp.max_distance = F32(0)
    return mp


def update_normal_and_depth(m, mp, pose_of, scale_factor):
    """MapPoint::UpdateNormalAndDepth through the oracle's restatement (oracle/pyorc.py), over the keyframes the cache holds with the poses pose_of(id) gives"""
    from oracle import pyorc
    kfs = {}
    for k, kf in m.kfs.items():
        if k in mp.obs or k == mp.ref_kf:
            keys = np.zeros(len(kf.octave), [("octave", "<i4")]); keys["octave"] = kf.octave
            kfs[k] = dict(T=pose_of(k), keys=keys, nlevels=getattr(kf, "nlevels", 8))
    d = dict(bad=mp.bad, obs=dict(mp.obs), ref=mp.ref_kf, pos=mp.pos, normal=mp.normal, min_distance=mp.min_distance, max_distance=mp.max_distance)
    pyorc.map_point_update_normal_and_depth(d, kfs, scale_factor)
    mp.normal = np.asarray(d["normal"], F32); mp.min_distance = F32(d["min_distance"]); mp.max_distance = F32(d["max_distance"])


def correct_loop(m, cur_id, Scw, scale_factor=0.0, cap=None):
    """:253-338.  Returns (set in walk order, CorrectedSim3 [n, 8], NonCorrectedSim3 [n, 8], points corrected).  The set is GetVectorCovisibleKeyFrames() of the current
    keyframe plus the keyframe itself, walked in ASCENDING KEYFRAME ID (the reference's maps are pointer-keyed).  More than cap members: CapacityError, nothing changed."""
    import covis_reference as R
    cur = pose(m.kfs[cur_id])
    walk = sorted(R.get_vector_covisibles(m, cur_id) + [cur_id])             # :254-255
    if cap is not None and len(walk) > cap:
        raise CapacityError
    scw = sim3_load(Scw)
    Twc = pose_inverse(cur.Tcw)                                             # :259
    corrected, non = {}, {}
    for kid in walk:                                                        # :265-287
        Tiw = pose(m.kfs[kid]).Tcw
        if kid != cur_id:
            corrected[kid] = sim3_mul(sim3_from_pose(fmul(Tiw, Twc)), scw)  # :273-279
        else:
            corrected[kid] = scw                                            # :258
        non[kid] = sim3_from_pose(Tiw)                                      # :282-286
    n_points = 0; done = set()
    for w, kid in enumerate(walk):                                          # :290
        kf = m.kfs[kid]
        swi = sim3_inv(corrected[kid])                                      # :294
        for pid in kf.mp_ids:                                               # :298-321
            mp = m.good_point(pid)
            if mp is None:
                continue
            loop_point(mp)
            if mp.corrected_by == cur_id:                                   # :306
                m.stats["held_by_a_later_member" if pid in done else "already_corrected"] += 1
                continue
            mp.pos = sim3_map(swi, sim3_map(non[kid], mp.pos.astype(np.float64))).astype(F32)       # :310-315
            mp.corrected_by = cur_id; mp.corrected_ref = kid; done.add(pid)                         # :318-319
            n_points += 1
            if kid != cur_id:
                m.stats["corrected_by_a_neighbour"] += 1
            if scale_factor > 0:                                            # :320: the poses as they stand in the middle of the walk
                for o in list(mp.obs) + [mp.ref_kf]:
                    if o in corrected and o in m.kfs:
                        m.stats["observer_before" if o < kid else ("observer_is_corrector" if o == kid else "observer_after")] += 1
                update_normal_and_depth(m, mp, lambda k: m.kfs[k].Tcw, scale_factor)
        Rm = quat_to_R(corrected[kid][0]); t = corrected[kid][1] * (1. / corrected[kid][2])         # :324-330
        T = np.eye(4, dtype=F32); T[:3, :3] = Rm.astype(F32); T[:3, 3] = t.astype(F32)
        kf.Tcw = T                                                          # :332
    return walk, np.stack([sim3_vec(corrected[k]) for k in walk]), np.stack([sim3_vec(non[k]) for k in walk]), n_points


# ---- Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:1118-1241): the action layer over the search -------------------------------------------------------
# The search itself is the oracle's (pyorc.fuse(..., sim3=1)); fuse_sim3_takes_part says which points enter it, fuse_sim3_actions what :1206-1237 do with its answer.

def fuse_sim3_takes_part(ids, bad, held):
    """a point takes part unless it is bad or the keyframe holds its id at some feature (spAlreadyFound = pKF->GetMapPoints(), :1131, :1143)"""
    inside = {int(x) for x in held if int(x) != NO_ID}
    return np.array([not b and int(i) not in inside for i, b in zip(ids, bad)], bool)


def fuse_sim3_actions(best_idx, held, ids, slot_of, bad_ids, obs_lists, kf_id):
    """The reference's walk over the points in list order.  held: the keyframe's per-feature ids before the call; ids: the points' ids; slot_of: id -> slot of every
    record of the map's index; bad_ids: the ids of bad records; obs_lists[i]: [(keyframe id, feature)] of point i.  Returns (held after, action, replace_slot, lists
    after): 1 = entered an empty feature (AddObservation + AddMapPoint), 2 = the feature holds a non-bad point -> vpReplacePoint (replace_slot; -1 for an id without
    a record, which corb_fuse_store reports as 2 as well), 4 = the feature holds a bad point (counted, nothing done)."""
    held = np.array(held, np.uint64).copy(); lists = [list(l) for l in obs_lists]
    action = np.zeros(len(best_idx), np.uint8); replace = np.full(len(best_idx), -1, np.int32)
    for i, f in enumerate(best_idx):
        if f < 0:
            continue
        cur = int(held[f])
        if cur != NO_ID:                                        # :1208-1213
            if cur not in slot_of:
                action[i] = 2
            elif cur in bad_ids:
                action[i] = 4
            else:
                action[i] = 2; replace[i] = slot_of[cur]
        else:                                                   # :1214-1218
            action[i] = 1
            if kf_id not in [k for k, _ in lists[i]]:            # AddObservation returns at once for a keyframe the list holds already (MapPoint.cc:146-148)
                lists[i] = sorted(lists[i] + [(kf_id, int(f))])
            held[f] = ids[i]
    return held, action, replace, lists

"""Optimizer::OptimizeEssentialGraph (corbslam_client/src/Optimizer.cc:840-1117) on the map model of tests/covis_cases.py: the flattening of the graph into vertices,
edges and measurements (plan) and the write-back of poses and points (commit), restated as the definition include/corb_essential_graph.h cites and the device route
(corb_essential_graph_plan / corb_essential_graph_store) is compared with.  The Sim3 algebra is tests/loopfix_reference.py's (float64 in the operation order of
G/types/sim3.h and Eigen); a Sim3 travels as 8 doubles (quaternion x y z w, t, s).

Attributes on top of covis_reference / localmap_reference / loopfix_reference (node() / loop_point() give them their defaults):
  kf.fixed        getFixed() (CORB_KF_FIXED)
  kf.loop_edges   mspLoopEdges: a set of ids (std::set<LightKeyFrame>: ascending id); GetLoopEdges() returns the ones the cache holds (KeyFrame.cc:552-561)
  mp.fixed        getFixed() (CORB_MP_FIXED)

Readings.  "Held": the id is in m.kfs.  Every walk the reference makes over a pointer-keyed container is in ASCENDING KEYFRAME ID (the choice correct_loop made).
Where the reference would hand g2o a null vertex the edge is DROPPED and counted, never emitted and never entered into sInsertedEdges:
  a loop connection whose key or member is not held (GetWeight on NULL) or, once past the weight test, is bad;
  a tree edge to a held parent that is bad, a loop edge to a held keyframe that is bad;
  any edge of the second loop whose own keyframe is bad (:943 walks bad keyframes too, :872 gave them no vertex).
A parent that is not held gives no tree edge at all (GetParent() is NULL, :961).

Map.stats counts what the seeded cases of tests/essgraph_cases.py must reach (tests/test_essgraph_reference.py asserts them)."""
import numpy as np

import covis_reference as R
import localmap_reference as LR
import loopfix_reference as XR

F32 = np.float32
NO_ID = XR.NO_ID
KINDS = ("loop_connection", "tree", "loop_edge", "covisibility")
SUPPRESSED = ("parent", "child", "loop_edge", "bad", "not_smaller", "inserted")


class CapacityError(Exception):
    pass


def node(kf):
    XR.pose(kf)
    if not hasattr(kf, "fixed"):
        kf.fixed = False
    if not hasattr(kf, "loop_edges"):
        kf.loop_edges = set()
    return kf


def add_loop_edge(m, kid, other_id, cap=32):
    """KeyFrame::AddLoopEdge (KeyFrame.cc:545-550); a full set: CapacityError, nothing changes"""
    kf = node(m.kfs[kid])
    if other_id in kf.loop_edges:
        return
    if len(kf.loop_edges) >= cap:
        raise CapacityError
    kf.loop_edges.add(other_id)


def measure(Siw, Sjw):
    """Sji = Sjw * Swi (:918, :927)"""
    return XR.sim3_vec(XR.sim3_mul(XR.sim3_load(Sjw), XR.sim3_inv(XR.sim3_load(Siw))))


def plan(m, loop_id, cur_id, corrected, non_corrected, loop_connections, min_weight=100):
    """corrected / non_corrected: {id: 8 doubles}; loop_connections: {id: iterable of ids}.  Returns dict(v_ids, S [K, 8], fixed [K], snc [K, 8], vi, vj, kind [E],
    meas [E, 8], counts) with counts = dict(n_vertices, n_edges, n_kind [4], n_dropped, n_lc_below_weight, n_suppressed [6])."""
    for kf in m.kfs.values():
        node(kf)
    v_ids = [k for k in sorted(m.kfs) if not m.kfs[k].bad]                       # :869-873
    rank = {k: r for r, k in enumerate(v_ids)}
    S, snc, fixed = [], [], []
    for k in v_ids:
        kf = m.kfs[k]
        s = np.asarray(corrected[k], np.float64) if k in corrected else XR.sim3_vec(XR.sim3_from_pose(kf.Tcw))      # :878-892
        S.append(s); snc.append(np.asarray(non_corrected[k], np.float64) if k in non_corrected else s)
        fixed.append(k == loop_id or kf.fixed)                                  # :894
    vi, vj, kind, meas = [], [], [], []
    n_kind = [0, 0, 0, 0]; sup = [0] * 6; dropped = 0; below = 0
    inserted = set()
    for i in sorted(loop_connections):                                          # :912-940
        for j in sorted(loop_connections[i]):
            if i not in m.kfs or j not in m.kfs:
                dropped += 1; m.stats["dropped_lc_not_held"] += 1
                continue
            if (i != cur_id or j != loop_id) and R.get_weight(m, i, j) < min_weight:     # :923
                below += 1; m.stats["lc_below_weight"] += 1
                continue
            if i == cur_id and j == loop_id and R.get_weight(m, i, j) < min_weight:
                m.stats["lc_kept_by_exemption"] += 1
            if i not in rank or j not in rank:
                dropped += 1; m.stats["dropped_lc_bad"] += 1
                continue
            vi.append(rank[i]); vj.append(rank[j]); kind.append(0); meas.append(measure(S[rank[i]], S[rank[j]])); n_kind[0] += 1
            inserted.add((min(i, j), max(i, j)))                                # :938
    for i in sorted(m.kfs):                                                     # :943
        kf = m.kfs[i]; LR.tree(kf)
        me = rank.get(i)

        def emit(j, k):
            nonlocal dropped
            if me is None or j not in rank:
                dropped += 1; m.stats["dropped_own_bad" if me is None else "dropped_other_bad"] += 1
                return
            vi.append(me); vj.append(rank[j]); kind.append(k); meas.append(measure(snc[me], snc[rank[j]])); n_kind[k] += 1
        parent = kf.parent if kf.parent is not None and kf.parent in m.kfs else None     # :958
        if parent is not None:
            emit(parent, 1)
        loops = sorted(l for l in kf.loop_edges if l in m.kfs)                  # :986
        for l in loops:
            if l < i:                                                           # :990
                emit(l, 2)
        for n in R.get_covisibles_by_weight(m, i, min_weight):                  # :1012
            if n is None:                                                       # :1016 pKFn
                continue
            if n == parent:
                sup[0] += 1
            elif n in kf.children:
                sup[1] += 1
            elif n in loops:
                sup[2] += 1
            elif m.kfs[n].bad:                                                  # :1018
                sup[3] += 1
            elif not n < i:
                sup[4] += 1
            elif (min(i, n), max(i, n)) in inserted:                            # :1020
                sup[5] += 1
            else:
                emit(n, 3)
    for k, name in enumerate(KINDS):
        m.stats["kind_" + name] += n_kind[k]
    for k, name in enumerate(SUPPRESSED):
        m.stats["suppressed_" + name] += sup[k]
    K, E = len(v_ids), len(vi)
    return dict(v_ids=v_ids, S=np.array(S, np.float64).reshape(K, 8), fixed=np.array(fixed, np.uint8), snc=np.array(snc, np.float64).reshape(K, 8),
                vi=np.array(vi, np.int32), vj=np.array(vj, np.int32), kind=np.array(kind, np.uint8), meas=np.array(meas, np.float64).reshape(E, 8),
                counts=dict(n_vertices=K, n_edges=E, n_kind=n_kind, n_dropped=dropped, n_lc_below_weight=below, n_suppressed=sup))


def pose_from_sim3(s):
    """[R | t * (1/s)] rounded to float32 once (:1064-1072)"""
    q, t, sc = XR.sim3_load(s)
    T = np.eye(4, dtype=F32); T[:3, :3] = XR.quat_to_R(q).astype(F32); T[:3, 3] = (t * (1. / sc)).astype(F32)
    return T


def commit(m, p, S_final, cur_id, scale_factor=0.0):
    """:1053-1115 with the final estimates S_final [K, 8] of the vertices of plan p.  Returns dict(n_poses_set, n_points_moved, n_points_kept, n_points_skipped,
    n_points_fixed_ref) and the set of moved point ids.  The one deviation from the reference (include/corb_essential_graph.h): a point whose reference keyframe is
    fixed is mapped with that vertex's final estimate, as every other point."""
    rank = {k: r for r, k in enumerate(p["v_ids"])}
    n = dict(n_poses_set=0, n_points_moved=0, n_points_kept=0, n_points_skipped=0, n_points_fixed_ref=0)
    for k, r in rank.items():                                                   # :1053-1076
        if m.kfs[k].fixed:                                                      # :1057
            continue
        m.kfs[k].Tcw = pose_from_sim3(S_final[r]); n["n_poses_set"] += 1
    moved = set()
    for pid in sorted(m.mps):                                                   # :1079-1115
        mp = XR.loop_point(m.mps[pid])
        if mp.bad or getattr(mp, "fixed", False):                               # :1084
            continue
        if mp.corrected_by == cur_id:                                           # :1088-1091
            idr = mp.corrected_ref; m.stats["point_corrected_reference"] += 1
        else:
            if mp.ref_kf is None:                                               # :1095
                n["n_points_skipped"] += 1; m.stats["point_no_reference"] += 1
                continue
            idr = mp.ref_kf
        if idr not in rank:
            n["n_points_kept"] += 1; m.stats["point_without_vertex"] += 1
            continue
        r = rank[idr]
        srw = XR.sim3_load(p["S"][r]); swr = XR.sim3_inv(XR.sim3_load(S_final[r]))      # :1101-1102
        mp.pos = XR.sim3_map(swr, XR.sim3_map(srw, mp.pos.astype(np.float64))).astype(F32)      # :1106
        n["n_points_moved"] += 1; moved.add(pid)
        if m.kfs[idr].fixed:
            n["n_points_fixed_ref"] += 1; m.stats["point_fixed_reference"] += 1
    if scale_factor > 0:                                                        # :1112, with the committed poses
        for pid in sorted(moved):
            XR.update_normal_and_depth(m, m.mps[pid], lambda k: m.kfs[k].Tcw, scale_factor)
    return n, moved

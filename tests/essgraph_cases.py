"""Seeded cases for Optimizer::OptimizeEssentialGraph on records: the maps of loopfix_cases.loop_map (12 keyframes, F = 24, connections at th = 3) after CorrectLoop's
propagation, with everything the second half of a loop event meets added on top: loop edges of earlier loops, a bad and a fixed keyframe, LoopConnections with pairs
above and below the weight, the exempt (cur, loop) pair, members that are bad or not held, fixed points, points without a reference and points whose reference has no
vertex.  tests/test_essgraph_reference.py asserts that the seeds together reach every event; the GPU tests compare the device route with essgraph_reference on
exactly these cases.  Also the hub map (one keyframe covisible with more than 64 others) and a 5-keyframe map whose edge list is written out by hand."""
import numpy as np

import covis_reference as R
import localmap_reference as LR
import loopfix_cases as C
import loopfix_reference as XR
import essgraph_reference as ER

F32 = np.float32
NO_ID = XR.NO_ID
UNHELD_KF = 770000001            # an id no store holds: a loop-connection member, a reference keyframe
SEEDS = (71, 72, 73, 74, 75, 76)


class Case:
    """m: the map; loop_id, cur_id; corrected, non_corrected: {id: 8 doubles}; loop_connections: {id: set of ids}"""

    def inputs(self, min_weight):
        return dict(loop_id=self.loop_id, cur_id=self.cur_id, corrected=self.corrected, non_corrected=self.non_corrected, loop_connections=self.loop_connections,
                    min_weight=min_weight)


def seeded(seed):
    i = SEEDS.index(seed) if seed in SEEDS else seed
    rng = np.random.default_rng(seed + 5000)
    m, cur_id = C.loop_map(seed, cur=C.LOOP_CURS[i % 3])
    for kf in m.kfs.values():
        ER.node(kf)
    ids = sorted(m.kfs)
    walk, co, nc, _ = XR.correct_loop(m, cur_id, C.loop_scw(m, cur_id, seed, C.LOOP_SCALES[i % 3]), 0.0)
    c = Case(); c.m = m; c.cur_id = cur_id
    c.corrected = {k: co[w].copy() for w, k in enumerate(walk)}; c.non_corrected = {k: nc[w].copy() for w, k in enumerate(walk)}
    outside = [k for k in ids if k not in walk]
    c.loop_id = outside[0] if outside else [k for k in ids if k != cur_id][0]
    others = [k for k in ids if k not in (cur_id, c.loop_id)]
    # loop edges of earlier loops: a pair of covisible keyframes (the covisibility edge between them is suppressed) and a far pair
    near = [(a, b) for a in others for b, w in m.kfs[a].ordered if b in m.kfs and b < a and w >= 3 and b != m.kfs[a].parent and b not in m.kfs[a].children and a not in m.kfs[b].children]
    pairs = [near[int(rng.integers(len(near)))]] if near else []
    pairs.append((ids[-1], ids[0]))
    for a, b in pairs:
        ER.add_loop_edge(m, a, b); ER.add_loop_edge(m, b, a)
    # one bad keyframe (it stays in its neighbours' lists, as in the reference until SetBadFlag's erasure) and one fixed one
    bad_id = others[int(rng.integers(len(others)))]
    m.kfs[bad_id].bad = True
    fixed_id = [k for k in others if k != bad_id][int(rng.integers(len(others) - 1))]
    m.kfs[fixed_id].fixed = True
    if i % 2 == 0:
        ER.add_loop_edge(m, ids[-1], bad_id) if bad_id < ids[-1] else ER.add_loop_edge(m, bad_id, ids[0])      # a loop edge that is dropped
    # LoopConnections: the exempt pair; per chosen member of the walk a covisible keyframe (weight >= 3: emitted at min_weight 3 and then in sInsertedEdges),
    # a far one (weight 0), the bad keyframe, an id the store does not hold
    lc = {cur_id: {c.loop_id}}
    for k in [w for w in walk if w != bad_id][:3]:
        s = lc.setdefault(k, set())
        cov = [b for b, w in m.kfs[k].ordered if b in m.kfs and w >= 3 and b != bad_id]
        if cov:
            s.add(cov[int(rng.integers(len(cov)))])
        far = [b for b in ids if b != k and R.get_weight(m, k, b) == 0]
        if far:
            s.add(far[int(rng.integers(len(far)))])
    members = [w for w in walk if w != bad_id]
    lc.setdefault(members[0], set()).add(bad_id)
    lc.setdefault(members[-1], set()).add(UNHELD_KF)
    c.loop_connections = lc
    # points: a few fixed, a few hanging on the fixed keyframe, on the bad one, on an id the store does not hold, on nothing
    pids = sorted(m.mps)
    for n, pid in enumerate(pids):
        mp = m.mps[pid]; mp.fixed = bool(rng.random() < 0.05)
        if mp.corrected_by == cur_id:
            continue
        u = rng.random()
        if u < 0.06:
            mp.ref_kf = fixed_id
        elif u < 0.10:
            mp.ref_kf = bad_id
        elif u < 0.13:
            mp.ref_kf = UNHELD_KF
        elif u < 0.16:
            mp.ref_kf = None
    return c


def hub(n_kf=70):
    """n_kf keyframes and three points seen by all of them (every weight among them is 3), the tree a chain: at min_weight 3 the newest keyframe emits more than
    64 covisibility edges, so the wave compaction of the fill crosses a 64-lane round.  GetCovisiblesByWeight answers NOTHING for a list whose every weight reaches
    the threshold (KeyFrame.cc:252-255), so one more keyframe, the oldest, sees one of the three points: every list ends in a weight of 1."""
    rng = np.random.default_rng(9)
    m = R.Map()
    ids = [10 + 2 * k for k in range(n_kf)]
    chain = [2] + ids
    for k in chain:
        m.kfs[k] = R.KeyFrame(k, [NO_ID] * 4)
    for p in range(3):
        pid = 5000 + p
        obs = {k: p for k in (chain if p == 0 else ids)}
        m.mps[pid] = R.MapPoint(pid, obs)
        for k in obs:
            m.kfs[k].mp_ids[obs[k]] = pid
    for k in chain:
        R.update_connections(m, k, th=1)
    for a, k in enumerate(chain):
        LR.set_tree(m, k, None if a == 0 else chain[a - 1], a == 0, chain[a + 1: a + 2])
    for k, kf in m.kfs.items():
        ER.node(kf); kf.Tcw = C.random_pose(rng); kf.nlevels = 8
    for mp in m.mps.values():
        XR.loop_point(mp); mp.pos = (rng.normal(size=3) * 4).astype(F32); mp.ref_kf = ids[0]; mp.fixed = False
        mp.normal = rng.normal(size=3).astype(F32); mp.min_distance = F32(1.5); mp.max_distance = F32(30.0)
    c = Case(); c.m = m; c.cur_id = ids[-1]; c.loop_id = ids[0]
    c.corrected = {}; c.non_corrected = {}; c.loop_connections = {c.cur_id: {c.loop_id}}
    return c


HAND_MIN_WEIGHT = 10
# the edge list of hand_map() at min_weight 10, written out by hand: (vi, vj, kind) over the vertices 1, 2, 4, 5 (keyframe 3 is bad)
HAND_EDGES = [(3, 0, 0),     # loop connection (5, 1): weight 3, kept by the (cur, loop) exemption alone
              (3, 1, 0),     # loop connection (5, 2): weight 30
              (1, 0, 2),     # keyframe 2: its loop edge to 1 (its parent 77 is not held: no tree edge)
              (2, 0, 1),     # keyframe 4: the tree edge to 1
              (2, 1, 3),     #             the covisibility edge to 2
              (3, 2, 1)]     # keyframe 5: the tree edge to 4
HAND_COUNTS = dict(n_vertices=4, n_edges=6, n_kind=[2, 2, 1, 1],
                   n_dropped=1,                  # the tree edge of the bad keyframe 3
                   n_lc_below_weight=1,          # (1, 3): weight 9
                   n_suppressed=[1,              # parent:      5 -> 4
                                 1,              # child:       4 -> 5
                                 2,              # loop edge:   1 -> 2, 2 -> 1
                                 2,              # bad:         4 -> 3, 5 -> 3
                                 4,              # not smaller: 2 -> 4, 2 -> 5, 3 -> 5, 3 -> 4
                                 1])             # inserted:    5 -> 2, a loop connection


def hand_map():
    """Five keyframes 1 .. 5, keyframe 3 bad, keyframe 2 fixed, loop = 1, cur = 5.  Tree: 4 -> 1, 5 -> 4, 3 -> 2, 2 -> 77 (not held).  Loop edges 1 <-> 2.  Weights:
    (5,4) 50, (5,3) 40, (5,2) 30, (5,1) 3, (4,2) 45, (4,3) 25, (4,1) 8, (2,3) 7, (2,1) 11, (3,1) 9, each as that many shared points; every list ends below the
    threshold of 10 (a list whose every weight reaches it answers nothing).  LoopConnections {5: {1, 2}, 1: {3}}; Corrected / NonCorrected hold keyframes 4 and 5."""
    rng = np.random.default_rng(4)
    m = R.Map()
    w = {(5, 4): 50, (5, 3): 40, (5, 2): 30, (5, 1): 3, (4, 2): 45, (4, 3): 25, (4, 1): 8, (2, 3): 7, (2, 1): 11, (3, 1): 9}
    held = {k: [] for k in (1, 2, 3, 4, 5)}
    pid = 7000
    for (a, b), x in w.items():                                                 # a weight of x: x points the two keyframes share
        for _ in range(x):
            mp = XR.loop_point(R.MapPoint(pid, {a: len(held[a]), b: len(held[b])}))
            mp.pos = (rng.normal(size=3) * 4).astype(F32); mp.ref_kf = a; mp.fixed = False
            m.mps[pid] = mp; held[a].append(pid); held[b].append(pid); pid += 1
    for k in (1, 2, 3, 4, 5):
        kf = ER.node(R.KeyFrame(k, held[k])); kf.Tcw = C.random_pose(rng); kf.nlevels = 8
        m.kfs[k] = kf
    for k in (1, 2, 3, 4, 5):
        R.update_connections(m, k, th=1)
    LR.set_tree(m, 1, None, False, [4]); LR.set_tree(m, 2, 77, False, [3]); LR.set_tree(m, 3, 2, False, []); LR.set_tree(m, 4, 1, False, [5]); LR.set_tree(m, 5, 4, False, [])
    m.kfs[3].bad = True; m.kfs[2].fixed = True
    ER.add_loop_edge(m, 1, 2); ER.add_loop_edge(m, 2, 1)
    c = Case(); c.m = m; c.cur_id = 5; c.loop_id = 1
    c.corrected = {k: XR.sim3_vec(XR.sim3_from_pose(C.random_pose(rng))) * np.array([1, 1, 1, 1, 1.1, 1.1, 1.1, 1.1]) for k in (4, 5)}
    c.non_corrected = {k: XR.sim3_vec(XR.sim3_from_pose(m.kfs[k].Tcw)) for k in (4, 5)}
    c.loop_connections = {5: {1, 2}, 1: {3}}
    return c

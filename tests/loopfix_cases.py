"""Seeded cases for the tests of the map update after a global bundle adjustment: spanning trees of a given shape with poses, marks, stored mTcwBefGBA and map points
spread over every branch of GlobalOptimize.cpp:498-531.  tests/test_loopfix_reference.py checks that these generators reach every event the readings are about
(loopfix_reference's Map.stats); the GPU tests then compare the device route with loopfix_reference on exactly these cases."""
import numpy as np

import covis_cases as G
import covis_reference as R
import localmap_reference as LR
import loopfix_reference as XR

NO_ID = XR.NO_ID
F32 = np.float32
LOOP_KF = 4242                   # nLoopKF of the cases; an unmarked keyframe or point carries 0 or the id of an older loop
OLD_LOOP_KF = 977


def random_pose(rng, spread=3.0):
    """a rigid pose as float32: a rotation orthonormal to float rounding, a translation of a few units"""
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    x, y, z, w = q
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    T = np.eye(4); T[:3, :3] = Rm; T[:3, 3] = rng.normal(size=3) * spread
    return T.astype(F32)


def add_keyframe(m, rng, kid, marked, stored_bef=False):
    kf = XR.pose(R.KeyFrame(kid, [NO_ID]))                      # one feature: a slot without features is not a keyframe of the store
    kf.Tcw = random_pose(rng); kf.TcwGBA = random_pose(rng)
    kf.ba_global = LOOP_KF if marked else (0 if rng.random() < 0.5 else OLD_LOOP_KF)
    if stored_bef:
        kf.TcwBef = random_pose(rng)
    m.kfs[kid] = kf
    return kf


def add_points(m, rng, n, ref_ids, first_id=500000, p_bad=0.1, p_gba=0.4, p_no_ref=0.08, sure=()):
    """n points over the branches of :498-531: bad, optimised by the global BA, or hanging on a reference keyframe (held or not, marked or not, reached or not).
    sure: keyframes that each get one good, unoptimised point whatever the draws say"""
    for i in range(n):
        mp = XR.point(R.MapPoint(first_id + 7 * i, {}, bad=bool(rng.random() < p_bad)))
        mp.pos = (rng.normal(size=3) * 4).astype(F32); mp.pos_gba = (rng.normal(size=3) * 4).astype(F32)
        mp.ba_global = LOOP_KF if rng.random() < p_gba else (0 if rng.random() < 0.5 else OLD_LOOP_KF)
        u = rng.random()
        mp.ref_kf = None if u < p_no_ref / 2 else (880000000 + i if u < p_no_ref else ref_ids[int(rng.integers(len(ref_ids)))])
        if i < len(sure):
            mp.bad = False; mp.ba_global = 0; mp.ref_kf = sure[i]
        m.mps[mp.id] = mp


def tree_map(seed, shape, n, n_points=0, id0=1, id_step=3, unmarked=0.0, twice=0.0, unheld_children=0.0, n_origins=1, unmarked_origin=False, unreached=0, cyclic=False):
    """A map of n keyframes (ids id0, id0 + id_step, ...) whose child sets form `shape`: "chain", "star" (every keyframe a child of the first) or "random" (the parent of
    keyframe i drawn from the ones before it).  unmarked: share of keyframes that start chains of up to 4 unmarked keyframes down the tree; twice: share of keyframes
    listed in a second set as well (ChangeParent's stale entry) -- half of them in a set of their parent's generation; unheld_children: share of sets that list an id
    the store does not hold; unmarked_origin: the first origin starts unmarked and the second origin lists it; n_origins: the first keyframes of the list are origins (a further origin heads a tree of its own: the keyframes are dealt out in turn);
    unreached: further keyframes, marked, with a stored mTcwBefGBA, in a tree no origin reaches; cyclic: the last keyframe lists the first origin.
    Returns (map, origins, slot order of the keyframes)."""
    rng = np.random.default_rng(seed)
    m = R.Map()
    ids = [id0 + id_step * i for i in range(n)]
    parent = [None] * n; depth = [0] * n
    for i in range(n_origins, n):
        if shape == "chain":
            parent[i] = i - n_origins
        elif shape == "star":
            parent[i] = i % n_origins
        else:
            lo = max(0, i - 12) if rng.random() < 0.7 else 0
            parent[i] = int(rng.integers(lo, i))
        depth[i] = depth[parent[i]] + 1
    kids = [[] for _ in range(n)]
    for i in range(n_origins, n):
        kids[parent[i]].append(i)
    marked = [True] * n
    for i in range(n_origins, n):
        if rng.random() < unmarked:
            j = i
            for _ in range(int(rng.integers(1, 5))):
                marked[j] = False
                if not kids[j]:
                    break
                j = kids[j][int(rng.integers(len(kids[j])))]
    if unmarked_origin:
        marked[0] = False
    for i in range(n):
        add_keyframe(m, rng, ids[i], marked[i], stored_bef=rng.random() < 0.2)
    for i in range(n):
        LR.set_tree(m, ids[i], None if parent[i] is None else ids[parent[i]], False, [ids[c] for c in kids[i]])
    for i in range(n_origins, n):
        if rng.random() < twice:
            same = [j for j in range(i) if depth[j] == depth[parent[i]] and j != parent[i]]
            j = same[int(rng.integers(len(same)))] if same and rng.random() < 0.5 else int(rng.integers(0, i))
            m.kfs[ids[j]].children.add(ids[i])                  # a lister before it in the list: the sets stay acyclic
    for i in range(n):
        if rng.random() < unheld_children:
            m.kfs[ids[i]].children.add(990000000 + i)
    far = [ids[-1] + 1000 + 5 * i for i in range(unreached)]
    for a, k in enumerate(far):
        add_keyframe(m, rng, k, marked=a % 3 != 2, stored_bef=True)
        LR.set_tree(m, k, far[a - 1] if a else None, False, far[a + 1: a + 2])
    if unmarked_origin and n_origins > 1:
        m.kfs[ids[1]].children.add(ids[0])                      # popped unmarked first, then composed by the second origin from the pose that pop left
    if cyclic:
        m.kfs[ids[-1]].children.add(ids[0])
    add_points(m, rng, n_points, ids + far, sure=far)
    order = [int(k) for k in rng.permutation(len(m.kfs))]
    all_ids = list(m.kfs)
    return m, ids[:n_origins], [all_ids[i] for i in order]


# name -> arguments of tree_map: the shapes the GPU test walks
GBA_CASES = {
    "chain70": dict(seed=51, shape="chain", n=70, n_points=300, unmarked=0.1, unreached=4),
    "star300": dict(seed=52, shape="star", n=301, n_points=300, unmarked=0.3, unreached=3),
    "random400": dict(seed=53, shape="random", n=400, n_points=2000, unmarked=0.1, twice=0.05, unheld_children=0.05, unreached=6, id0=1000001),
    "two_origins": dict(seed=54, shape="random", n=60, n_points=200, unmarked=0.15, twice=0.1, n_origins=2, unreached=3),
    "unmarked_origin": dict(seed=55, shape="random", n=40, n_points=150, unmarked=0.15, twice=0.1, n_origins=2, unmarked_origin=True, unreached=3),
}
CYCLIC_CASE = dict(seed=56, shape="chain", n=9, n_points=40, unmarked=0.2, cyclic=True)


# ---- CorrectLoop's propagation ----
def loop_map(seed, n_kf=12, F=24, cur="middle", p_already=0.08, p_stale=0.15):
    """A random map (tests/covis_cases.py: a point is seen by a run of up to 6 neighbouring keyframes, some points bad, some ids dangling, some observers not held)
    whose keyframes were all connected once (th = 3, so that the middle keyframe is covisible with 6 to 8 others), with poses, positions, reference keyframes (mostly
    the first held observer) and, for p_already of the points, mnCorrectedByKF already equal to the current keyframe's id.  p_stale of the points with two held observers are no longer held by the first of them (the
    feature was given away, the observation stayed): such an observer can precede the point's corrector in the walk.  The current keyframe is the middle one of
    the run; cur = "largest": it carries the id of another client (1 000 000 + k), the largest of its set; "smallest": every OTHER keyframe does; "middle": neither.
    Returns (map, id of the current keyframe)."""
    rng = np.random.default_rng(seed)
    ids = [int(i) for i in np.sort(rng.choice(np.arange(1, 1 + 6 * n_kf), n_kf, replace=False))]
    c = n_kf // 2
    if cur == "largest":
        ids[c] += 1000000
    elif cur == "smallest":
        ids = [k if j == c else k + 1000000 for j, k in enumerate(ids)]
    m = G.random_map(seed=seed, n_kf=n_kf, F=F, span=5, max_obs=6, p_bad_kf=0.0, ids=ids)
    for p, mp in m.mps.items():
        held = [o for o in sorted(mp.obs) if o in m.kfs]
        if len(held) >= 2 and rng.random() < p_stale:
            for i, q in enumerate(m.kfs[held[0]].mp_ids):
                if q == p:
                    m.kfs[held[0]].mp_ids[i] = NO_ID
    for k in sorted(m.kfs):
        LR.update_connections(m, k, th=3)
    cur_id = ids[c]
    for k, kf in m.kfs.items():
        XR.pose(kf); kf.Tcw = random_pose(rng); kf.nlevels = 8
    for p, mp in m.mps.items():
        XR.loop_point(mp)
        mp.pos = (rng.normal(size=3) * 4).astype(F32)
        held = [o for o in sorted(mp.obs) if o in m.kfs]
        mp.ref_kf = held[int(rng.integers(len(held)))] if held and rng.random() < 0.9 else (min(mp.obs) if mp.obs else None)
        mp.normal = rng.normal(size=3).astype(F32); mp.min_distance = F32(1.5); mp.max_distance = F32(30.0)
        if rng.random() < p_already:
            mp.corrected_by = cur_id; mp.corrected_ref = 5
    return m, cur_id


def loop_scw(m, cur_id, seed, scale):
    """mg2oScw as 8 doubles (quaternion x y z w, t, s): the current keyframe's pose turned and shifted a little, with the given scale"""
    rng = np.random.default_rng(seed)
    T = m.kfs[cur_id].Tcw.astype(np.float64)
    d = random_pose(rng, spread=0.3).astype(np.float64)
    d[:3, :3] = np.eye(3) * 0.97 + d[:3, :3] * 0.03                            # a small turn (made orthonormal below)
    u, _, vt = np.linalg.svd(d[:3, :3]); d[:3, :3] = u @ vt
    S = d @ T
    return np.concatenate([XR.quat_from_R(S[:3, :3]), S[:3, 3] * scale, [scale]])


LOOP_SEEDS = (61, 62, 63, 64, 65, 66)
LOOP_CURS = ("middle", "largest", "smallest")
LOOP_SCALES = (1.0, 0.8, 1.25)

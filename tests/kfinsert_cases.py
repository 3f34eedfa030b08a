"""Seeded scenes for keyframe insertion (tests/kfinsert_reference.py is the definition), shared by the CPU and GPU tests.  Each generator returns the scene with the
call's arguments; counts() applies the definition and returns how often every kind / decision occurs, so tests/test_kfinsert_reference.py can hold the cases to
reaching every branch without a GPU."""
import collections

import numpy as np

import kfinsert_reference as R

f32 = np.float32
F, O = 320, 6                        # features per keyframe record, observations per map-point record of the scenes
TH_DEPTH = 35.0
SCALE = np.cumprod([1.0] + [1.2] * 7).astype(f32)
for _l in range(1, 8):               # mvScaleFactor[i] = mvScaleFactor[i-1] * scaleFactor in float (ORBextractor.cc:418-424)
    SCALE[_l] = f32(SCALE[_l - 1] * f32(1.2))
CAM = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, bf=386.1448, mb=0.5371657, scale=SCALE)


def _pose(rng):
    a = rng.uniform(-0.2, 0.2, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
    Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
    Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
    T = np.eye(4); T[:3, :3] = Rx @ Ry @ Rz; T[:3, 3] = rng.uniform(-2, 2, 3)
    return T.astype(f32)


def keyframe(rng, kid, n, depth=None):
    kp = np.zeros(n, R.KP_DTYPE)
    kp["x"] = rng.uniform(0, 1241, n).astype(f32); kp["y"] = rng.uniform(0, 376, n).astype(f32); kp["octave"] = rng.integers(0, 8, n); kp["size"] = 31; kp["angle"] = rng.uniform(0, 360, n)
    ur = np.where(rng.random(n) < 0.6, kp["x"] - 3, -1).astype(f32)
    d = rng.uniform(2, 30, n).astype(f32) if depth is None else np.asarray(depth, f32)
    return dict(id=kid, Tcw=_pose(rng), nlevels=8, kf_flags=0, kp=kp, desc=rng.integers(0, 256, (n, 32)).astype(np.uint8), u_right=ur, depth=d,
                flags=np.zeros(n, np.uint8), mp_id=np.full(n, R.NO_MAP_POINT, np.uint64))


def point(rng, pid, obs, ref=None, bad=False, found=1, visible=1, first_kf=None):
    p = R.blank_point()
    p["id"] = pid; p["obs"] = sorted(obs); p["ref_kf_id"] = (obs[0][0] if obs else 0) if ref is None else ref; p["flags"] = R.MP_BAD if bad else 0
    p["descriptor"] = rng.integers(0, 256, 32).astype(np.uint8); p["world_pos"] = rng.uniform(-5, 20, 3).astype(f32); p["client_id"] = 1
    p["normal"] = rng.uniform(-1, 1, 3).astype(f32); p["min_distance"] = f32(1.5); p["max_distance"] = f32(40)
    p["n_found"] = found; p["n_visible"] = visible
    if first_kf is not None:
        p["scratch"] = dict(first_kf_id=first_kf)
    return p


def _scene(kfs, mps, cap):
    return dict(kfs=kfs, mps=mps + [None] * (cap - len(mps)), cam=CAM, F=F, O=O, index={})


# ---------------------------------------------------------------- call 1
# name -> (seed, features, features with depth, of which not beyond th_depth (None: all), mode)
POINTS = {
    "n0": (1, 0, 0, None, 1), "n1_nodepth": (2, 1, 0, None, 1), "n1": (3, 1, 1, None, 1), "n63_allfar": (4, 63, 63, 0, 1), "n64": (5, 64, 64, None, 1),
    "n65_allfar": (6, 65, 60, 0, 1), "d99_allfar": (7, 120, 99, 0, 1), "d100_far99": (8, 130, 100, 99, 1), "d101_far100": (9, 130, 101, 100, 1),
    "d102_far101": (10, 140, 102, 101, 1), "d102_far100": (11, 140, 102, 100, 1), "d257": (12, 257, 257, None, 1), "d257_far99": (13, 257, 257, 99, 1),
    "d257_far0": (14, 300, 257, 0, 1), "full_far150": (15, F, 300, 150, 1), "init": (16, 257, 200, 50, 0), "init_n65": (17, 65, 64, None, 0), "last_frame": (18, 257, 230, 101, 2),
    "last_frame_far0": (19, 130, 120, 0, 2),
}
N_OLD = 40                           # records the map holds before the call: slots 0 .. 39, ids 500 ..


def points_case(name):
    seed, n, n_depth, n_near, mode = POINTS[name]
    rng = np.random.default_rng(1000 + seed)
    depth = rng.choice(np.array([0.0, -1.0, np.nan], f32), n)
    cand = rng.permutation(n)[:n_depth]
    near = n_depth if n_near is None else n_near
    z = np.concatenate([np.round(rng.uniform(1, TH_DEPTH - 1, near) * 4) / 4,          # quarter steps: equal depths occur
                        rng.uniform(TH_DEPTH + 0.5, 90, n_depth - near)]).astype(f32)
    if near >= 2:
        z[1] = f32(TH_DEPTH)                                                             # exactly the threshold is not beyond it
    depth[cand] = z
    kf = keyframe(rng, 17, n, depth)
    mirror = keyframe(rng, 0, n, depth)
    olds = [point(rng, 500 + k, [(10, k)] if k % 3 else []) for k in range(N_OLD)]      # every third one has lost its observations
    held = rng.random(n)
    for i in range(n):
        if held[i] < 0.45:
            continue
        kf["mp_id"][i] = 9000 + i if held[i] > 0.85 else 500 + int(rng.integers(0, N_OLD))
        kf["flags"][i] = R.HAS_MP if held[i] < 0.8 else 0
    mirror["mp_id"][:] = kf["mp_id"]
    sc = _scene([kf, mirror], olds, N_OLD + n + 4)
    R.build_index(sc, 0, N_OLD)
    return sc, dict(slot=0, th_depth=TH_DEPTH, mode=mode, first_mp_slot=N_OLD + 2, first_mp_id=70000, client_id=3, frame_id=4242, mirror=1)


# ---------------------------------------------------------------- calls 2 and 3: a small map of six keyframes, the new one in slot 5
KF_IDS = [10, 13, 16, 19, 22]        # slots 0 .. 4; slot 0 lies outside the named range [1, 6), id 7777 is in no slot
ASSOC = {"n0": (1, 0, 30), "n1": (2, 1, 30), "n63": (3, 63, 17), "n64": (4, 64, 30), "n65": (5, 65, 17), "n257": (6, 257, 30), "full": (7, F, 17), "list_full": (8, 65, 17)}


def assoc_case(name):
    seed, n, new_id = ASSOC[name]
    rng = np.random.default_rng(2000 + seed)
    kfs = [keyframe(rng, kid, 50) for kid in KF_IDS] + [keyframe(rng, new_id, n)]
    kfs[3]["kf_flags"] = R.KF_BAD
    new = kfs[5]; mps = []

    def obs_list(length, with_new, feature=0):
        ids = list(rng.permutation(KF_IDS + [7777])[: length - (1 if with_new else 0)])
        return sorted([(int(k), int(rng.integers(0, 50))) for k in ids] + ([(new_id, feature)] if with_new else []))

    i = 0
    while i < n:
        r = rng.random(); pid = 500 + len(mps); slot = len(mps)
        if r < 0.12:
            i += 1                                                                       # no id
        elif r < 0.22:
            new["mp_id"][i] = 9000 + i; i += 1                                           # unresolved
        elif r < 0.34:
            mps.append(point(rng, pid, obs_list(2, False), bad=True)); new["mp_id"][i] = pid; i += 1
        elif r < 0.5:
            length = int(rng.choice([1, 2, O - 1, O]))                                   # observes the keyframe already
            mps.append(point(rng, pid, obs_list(length, True, i))); new["mp_id"][i] = pid; i += 1
        else:
            length = int(rng.choice([1, 2, O - 1]))                                      # to be added; now and then held by up to three features
            if name == "list_full" and i > n // 2 and not any(len(m["obs"]) == O and new_id not in [k for k, _ in m["obs"]] for m in mps):
                length = O
            ob = obs_list(length, False)
            mps.append(point(rng, pid, ob, ref=ob[int(rng.integers(0, len(ob)))][0]))
            for _ in range(int(rng.choice([1, 1, 1, 2, 3]))):
                if i < n:
                    new["mp_id"][i] = pid; i += 1
    perm = rng.permutation(n)                                                            # duplicates are not neighbours
    new["mp_id"] = new["mp_id"][perm]
    for m in mps:
        m["obs"] = [(k, int(np.where(perm == f)[0][0]) if k == new_id else f) for k, f in m["obs"]]
    new["flags"][:] = np.where(new["mp_id"] != R.NO_MAP_POINT, R.HAS_MP, 0) | np.where(rng.random(n) < 0.2, R.OUTLIER, 0)
    sc = _scene(kfs, mps, len(mps) + 3)
    R.build_index(sc, 0, len(mps))
    return sc, dict(slot=5, kf_first=1, kf_n=5, scale_factor=1.2)


# ---------------------------------------------------------------- call 4
CULL = {"n0": (1, 0), "n1": (2, 1), "n64": (3, 64), "n65": (4, 65), "n300": (5, 300)}
CUR_KF = 22


def cull_case(name):
    seed, n = CULL[name]
    rng = np.random.default_rng(3000 + seed)
    kfs = [keyframe(rng, kid, 50) for kid in KF_IDS]
    n_mp = max(4, (3 * n) // 4)
    mps = []
    for s in range(n_mp):
        length = int(rng.integers(1, 5))
        ids = rng.permutation(KF_IDS + [7777])[:length]
        obs = []
        for k in ids:                                                                    # a feature is observed by one point
            f = s if s < 50 and int(k) != 7777 else int(rng.integers(0, 50))
            obs.append((int(k), f))
        found, visible = [(1, 1), (3, 4), (1, 4), (1, 5), (0, 0), (0, 3), (5, 5)][int(rng.integers(0, 7))]
        first = CUR_KF - int(rng.choice([0, 1, 2, 2, 3, 5]))
        mps.append(point(rng, 500 + s, obs, bad=rng.random() < 0.15, found=found, visible=visible, first_kf=first))
    for s, m in enumerate(mps):
        for k, f in m["obs"]:
            if k in KF_IDS and f == s and not m["flags"] & R.MP_BAD:
                kf = kfs[KF_IDS.index(k)]; kf["mp_id"][f] = m["id"]; kf["flags"][f] = R.HAS_MP
    recent = rng.integers(0, n_mp, n).astype(np.int32) if n else np.zeros(0, np.int32)   # with repeats
    sc = _scene(kfs, mps, n_mp + 2)
    R.build_index(sc, 0, n_mp)
    return sc, dict(recent_slots=recent, cur_kf_id=CUR_KF, th_obs=3, kf_first=1, kf_n=4)


def counts():
    """how often the definition reaches every kind / decision over all the cases"""
    c = {1: collections.Counter(), 3: collections.Counter(), 4: collections.Counter()}
    for name in POINTS:
        sc, a = points_case(name)
        if a["mode"] != 0:
            c[1].update(R.create_stereo_points(sc, apply=False, **a)[0]["kind"].tolist())
    for name in ASSOC:
        sc, a = assoc_case(name)
        c[3].update(R.process_new_keyframe(sc, apply=False, **a)[0]["kind"].tolist())
    for name in CULL:
        sc, a = cull_case(name)
        out = R.map_point_culling(sc, apply=True, **a)[0]
        first = {}
        for i, s in enumerate(a["recent_slots"]):
            if int(s) not in first:                                                      # each first-applicable branch, at a point's first occurrence
                first[int(s)] = i; c[4][int(out["decision"][i])] += 1
    return c

"""Seeded maps for the covisibility tests: covis_reference.Map objects, and the same maps as the flat arrays the stores take.  tests/test_covis_reference.py checks
that the generators reach the cases they exist for (ties, fallbacks, unknown ids, bad points, early returns, re-sorted rows, both culling answers); the GPU tests then
compare the device routes with covis_reference on exactly these maps."""
import numpy as np

import covis_reference as R

NO_ID = R.NO_ID
UNKNOWN_BASE = 9000000          # ids from here on belong to keyframes the store never holds


def random_map(seed, n_kf=20, F=80, fill=0.8, span=6, max_obs=8, p_bad=0.05, p_unknown=0.15, p_bad_kf=0.1, p_dangling=0.03, p_double=0.02, sparse=(), id0=False,
               ids=None, point_ids=None):
    """n_kf keyframes of F feature slots; a point is seen by a run of up to `span` keyframes next to each other (near neighbours share many points, far ones few or
    none) and, with p_unknown, by one or two keyframes the store does not hold.  sparse: indices of keyframes that take part in at most four points (no weight
    reaches 15: the fallback).  p_double: a keyframe holds the point at a second feature.  p_dangling: a feature holds an id without a record."""
    rng = np.random.default_rng(seed)
    if ids is None:
        ids = np.sort(rng.choice(np.arange(1, 1 + 6 * n_kf), n_kf, replace=False)).astype(np.uint64)
        if id0:
            ids[0] = 0
    ids = [int(i) for i in ids]
    m = R.Map()
    for kid in ids:
        n = F if rng.random() < 0.7 else int(rng.integers(max(1, F // 2), F + 1))
        ur = np.where(rng.random(n) < 0.6, rng.uniform(1, 600, n), -1.0).astype(np.float32)
        m.kfs[kid] = R.KeyFrame(kid, [NO_ID] * n, octave=rng.integers(0, 8, n).tolist(), depth=rng.uniform(-2, 60, n).astype(np.float32).tolist(), u_right=ur.tolist(),
                                bad=bool(rng.random() < p_bad_kf))
    free = {kid: list(rng.permutation(len(m.kfs[kid].mp_ids))) for kid in ids}
    quota = {kid: (4 if k in sparse else int(fill * len(m.kfs[kid].mp_ids))) for k, kid in enumerate(ids)}
    used = {kid: 0 for kid in ids}
    n_points = 0
    for _ in range(40 * n_kf * F):
        if all(used[k] >= quota[k] for k in ids):
            break
        c = int(rng.integers(n_kf)); width = int(rng.integers(1, span + 1))
        seen = [ids[k] for k in range(c, min(n_kf, c + width)) if used[ids[k]] < quota[ids[k]] and free[ids[k]]][:max_obs]
        if not seen:
            continue
        pid = int(point_ids[n_points]) if point_ids is not None else 1000 + 3 * n_points
        n_points += 1
        obs = {}
        for kid in seen:
            idx = int(free[kid].pop()); obs[kid] = idx; m.kfs[kid].mp_ids[idx] = pid; used[kid] += 1
            if rng.random() < p_double and free[kid]:
                m.kfs[kid].mp_ids[int(free[kid].pop())] = pid
        if rng.random() < p_unknown:
            for _u in range(int(rng.integers(1, 3))):
                if len(obs) < max_obs:
                    obs[UNKNOWN_BASE + int(rng.integers(0, 12))] = int(rng.integers(0, F))
        m.mps[pid] = R.MapPoint(pid, obs, bad=bool(rng.random() < p_bad))
    for kid in ids:
        for idx in free[kid]:
            if rng.random() < p_dangling:
                m.kfs[kid].mp_ids[int(idx)] = 500000000 + int(rng.integers(0, 1000))
    return m


def star_map(F, obs, distinct, n_in_store=6, main_id=100, weights=None):
    """One keyframe (id main_id) of F features, every feature holding its own point; a point is seen by the keyframe and obs - 1 others, handed out round-robin over
    `distinct` other ids of which the first n_in_store are keyframes of the store (one feature each) and the rest are not.  weights (optional): [(id, count)] instead --
    keyframe `id` sees the first `count` points not yet given to it.  F * (obs - 1) >= distinct makes every id appear."""
    m = R.Map()
    others = [200 + 5 * k for k in range(distinct)]
    m.kfs[main_id] = R.KeyFrame(main_id, [10000 + i for i in range(F)])
    for k, oid in enumerate(others[:n_in_store]):
        m.kfs[oid] = R.KeyFrame(oid, [NO_ID])
    r = 0
    for i in range(F):
        o = {main_id: i}
        if weights is None:
            for _ in range(min(obs - 1, distinct)):
                o[others[r % distinct]] = 0; r += 1
        m.mps[10000 + i] = R.MapPoint(10000 + i, o)
    if weights is not None:
        for oid, count in weights:
            if oid not in m.kfs:
                m.kfs[oid] = R.KeyFrame(oid, [NO_ID])
            for i in range(count):
                m.mps[10000 + i].obs[oid] = 0
    return m


def culling_map(seed, n_cov=3, F=40, id0=False, n_helpers=3):
    """A current keyframe (id 7) covisible with n_cov keyframes of F points each.  A point of a covisible keyframe is seen by that keyframe, the current one and 0 .. 3
    more keyframes of the store (`helpers`, themselves covisible with the current one) and perhaps one outside it, octaves and right coordinates at random: Observations() of exactly 3 and 4 and the octave + 1 / + 2 boundary both occur; the odd covisible
    keyframes see mostly well-observed points (cull), the even ones mostly not (keep)."""
    rng = np.random.default_rng(seed)
    m = R.Map()
    cov = [20 + 3 * k for k in range(n_cov)]
    if id0 and n_cov:
        cov[0] = 0
    helpers = [900, 903, 906][:n_helpers]
    cur_ids = []
    for h in helpers:
        m.kfs[h] = R.KeyFrame(h, [NO_ID] * (n_cov * F), octave=[0] * (n_cov * F), u_right=[-1.0] * (n_cov * F))
    for k, kid in enumerate(cov):
        kf = R.KeyFrame(kid, [NO_ID] * F, octave=rng.integers(1, 5, F).tolist(), depth=rng.uniform(-1, 50, F).astype(np.float32).tolist(),
                        u_right=np.where(rng.random(F) < 0.5, 10.0, -1.0).astype(np.float32).tolist())
        m.kfs[kid] = kf
        for i in range(F):
            pid = 50000 + k * F + i
            kf.mp_ids[i] = pid
            obs = {kid: i, 7: len(cur_ids)}
            cur_ids.append(pid)
            n_more = 3 if (k % 2 == 1 and rng.random() < 0.97) else int(rng.integers(0, 4))
            for h in helpers[:n_more]:
                j = k * F + i
                obs[h] = j; m.kfs[h].mp_ids[j] = pid
                m.kfs[h].octave[j] = kf.octave[i] + int(rng.integers(-1, 3)) if k % 2 == 0 else kf.octave[i] + int(rng.integers(-1, 2))
                m.kfs[h].u_right[j] = 5.0 if rng.random() < 0.3 else -1.0
            if rng.random() < 0.2:
                obs[UNKNOWN_BASE + int(rng.integers(0, 4))] = 0
            m.mps[pid] = R.MapPoint(pid, obs, bad=bool(rng.random() < 0.04))
    m.kfs[7] = R.KeyFrame(7, cur_ids, octave=[2] * len(cur_ids))
    return m


def arrays(m, kf_order=None, mp_order=None):
    """the map as plain arrays in slot order: dict(kf_ids, feat_off, mp_id, octave, depth, u_right, kf_bad, mp_ids, mp_bad, obs_off, obs_kf, obs_idx)"""
    kf_order = list(m.kfs) if kf_order is None else list(kf_order)
    mp_order = list(m.mps) if mp_order is None else list(mp_order)
    feat_off = np.concatenate([[0], np.cumsum([len(m.kfs[k].mp_ids) for k in kf_order])]).astype(np.int32)
    cat = lambda f, dt: np.concatenate([np.asarray(f(m.kfs[k]), dt) for k in kf_order]) if kf_order else np.zeros(0, dt)
    obs_kf, obs_idx, obs_off = [], [], [0]
    for p in mp_order:
        for oid in sorted(m.mps[p].obs):
            obs_kf.append(oid); obs_idx.append(m.mps[p].obs[oid])
        obs_off.append(len(obs_kf))
    return dict(kf_ids=np.array(kf_order, np.uint64), feat_off=feat_off, mp_id=cat(lambda k: k.mp_ids, np.uint64), octave=cat(lambda k: k.octave, np.int32),
                depth=cat(lambda k: k.depth, np.float32), u_right=cat(lambda k: k.u_right, np.float32), kf_bad=np.array([m.kfs[k].bad for k in kf_order], bool),
                mp_ids=np.array(mp_order, np.uint64), mp_bad=np.array([m.mps[p].bad for p in mp_order], bool), obs_off=np.array(obs_off, np.int32),
                obs_kf=np.array(obs_kf, np.uint64), obs_idx=np.array(obs_idx, np.uint32))


def rows(m, kf_order):
    """every row as corb_covis_get returns it: [((all ids, all weights), (ordered ids, ordered weights))] in slot order"""
    out = []
    for k in kf_order:
        kf = m.kfs[k]
        a = R.descending([(w, i) for i, w in kf.weights.items()])
        out.append((([i for i, _ in a], [w for _, w in a]), ([i for i, _ in kf.ordered], [w for _, w in kf.ordered])))
    return out


# the maps the GPU tests update in batches; tests/test_covis_reference.py asserts that each reaches every case of UpdateConnections
RANDOM_MAPS = {
    "k20": dict(seed=11, n_kf=20, F=80, sparse=(7, 19)),
    "k20_id0": dict(seed=12, n_kf=20, F=96, sparse=(0, 13), id0=True, p_unknown=0.3),
    "k40_wide": dict(seed=13, n_kf=40, F=130, span=12, max_obs=12, sparse=(5,)),
}
# the maps of the culling tests: (n_cov covisible keyframes + n_helpers) listed keyframes
CULLING_MAPS = {
    "c3": dict(seed=21, n_cov=3, F=40),
    "c3_id0": dict(seed=22, n_cov=4, F=40, id0=True),
    "c1": dict(seed=23, n_cov=1, F=40, n_helpers=0),
    "c64": dict(seed=24, n_cov=61, F=20),
    "c65": dict(seed=25, n_cov=62, F=20),
}

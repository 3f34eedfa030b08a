"""The seeded cases of test_gpu_sim3_ransac.py (built once; test_sim3solver_reference.py checks their conditioning on the CPU)."""
import functools
import numpy as np
import sim3solver_reference as R


def force(rv, it, triple, N):
    """make iteration `it` draw the ascending triple a < b < c < N - 2 (positions = values: no swapped entry is touched)"""
    a, b, c = triple
    assert a < b < c < N - 2
    rv[it] = [int((a + 0.5) / N * R.RAND_RANGE), int((b + 0.5) / (N - 1) * R.RAND_RANGE), int((c + 0.5) / (N - 2) * R.RAND_RANGE)]
    assert R.draw_triple(rv[it], N) == (a, b, c)


def _case(seed, Ns, shares, min_inliers=20, max_iterations=300, fix_scale=False, scales=None):
    prs = [R.scene(seed + 10 * k, n, sh, scale=1.0 if (fix_scale or scales is None) else scales[k])[0] for k, (n, sh) in enumerate(zip(Ns, shares))]
    return dict(problems=prs, rand=R.draws(seed, len(Ns), max_iterations), min_inliers=min_inliers, max_iterations=max_iterations, fix_scale=fix_scale)


@functools.lru_cache(maxsize=None)
def host_cases():
    c = {}
    Ns = [19, 20, 21, 63, 64, 65, 129]; sh = [0.0, 0.0, 0.0, 0.3, 0.7, 0.3, 0.0]
    c["seven"] = _case(100, Ns, sh, scales=[1.0, 1.3, 0.8, 1.0, 1.2, 0.9, 1.1])
    c["seven_fix_scale"] = _case(200, Ns, sh, fix_scale=True)
    c["three"] = _case(300, [40, 300, 129], [0.0, 0.3, 0.7], scales=[1.0, 1.25, 1.0])
    c["n3"] = _case(400, [3], [0.0], min_inliers=3)
    c["single_iteration"] = _case(500, [30], [0.0], max_iterations=1)
    # one candidate with the special correspondences: 0, 1, 2 have p1c == p2c (drawn together at iteration 0: the identity-rotation triple); 5 has z == 0 on side 1 and
    # 9 on side 2 -- outside a triple wherever the draws miss them, inside one at iterations 1 and 2
    one = _case(600, [300], [0.3], scales=[1.15])
    pr = one["problems"][0]; x1 = pr["x1"].copy(); x2 = pr["x2"].copy()
    x1[:3] = x2[:3]
    x1[5, 2] = 0.0; x2[9, 2] = 0.0
    one["problems"] = [R.problem(x1, x2, pr["sigma2_1"], pr["sigma2_2"], R.KITTI, R.KITTI)]
    force(one["rand"][0], 0, (0, 1, 2), 300); force(one["rand"][0], 1, (5, 6, 7), 300); force(one["rand"][0], 2, (8, 9, 10), 300)
    c["one_special"] = one
    return c


def _pose(rng):
    T = np.eye(4); T[:3, :3] = R._rot(rng, 0.3); T[:3, 3] = rng.uniform(-1, 1, 3)
    return T.astype(np.float32)


@functools.lru_cache(maxsize=None)
def record_scene(seed=700, n1=150, n_cand=3):
    """keyframe 1 and n_cand candidates as records: map points 1000 + i at KF1's features, 500000 + 1000 c + j at candidate c's; vpMatched12 pairs feature i1 of KF1 with a
    point of the candidate, 30 % of them unrelated.  The filter cases of the constructor sit at fixed features of KF1 (see `cases`)."""
    rng = np.random.default_rng(seed)
    scale = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    kf1 = dict(id=11, Tcw=_pose(rng), K=R.KITTI, octave=rng.integers(0, 8, n1).astype(np.int32), mp_id=(1000 + np.arange(n1)).astype(np.uint64))
    T1 = kf1["Tcw"].astype(np.float64)
    Xc1 = np.stack([rng.uniform(-6, 6, n1), rng.uniform(-2, 2, n1), rng.uniform(5, 30, n1)], axis=1)
    W1 = (Xc1 - T1[:3, 3]) @ T1[:3, :3]                                   # Rcw^T (Xc - tcw)
    points = {1000 + i: dict(pos=W1[i].astype(np.float32), bad=False, obs={11: i}) for i in range(n1)}
    cases = dict(bad1=3, bad2=7, unknown_id=12, no_mp1=18, not_matched=21, not_observing1=25, not_observing2=31, other_index=40)
    points[1000 + cases["bad1"]]["bad"] = True
    kf1["mp_id"][cases["no_mp1"]] = R.NO_MAP_POINT
    points[1000 + cases["not_observing1"]]["obs"] = {99: 0}
    j = cases["other_index"] + 1                                          # the point held at feature 40 observes KF1 at feature 41 (another octave)
    kf1["octave"][cases["other_index"]] = 0; kf1["octave"][j] = 3
    points[1000 + cases["other_index"]]["obs"] = {11: j}
    kfs2, matched = [], []
    for c in range(n_cand):
        n2 = n1 + 5 * c - 4
        k2 = dict(id=22 + c, Tcw=_pose(rng), K=(700.0 + 10 * c, 705.0, 600.0, 180.0 + c), octave=rng.integers(0, 8, n2).astype(np.int32),
                  mp_id=(500000 + 1000 * c + np.arange(n2)).astype(np.uint64))
        T2 = k2["Tcw"].astype(np.float64)
        Rs = R._rot(rng, 0.5); ts = rng.uniform(-0.5, 0.5, 3); s = [1.0, 1.2, 0.85][c % 3]
        perm = rng.permutation(n2)[:n1] if n2 >= n1 else np.concatenate([rng.permutation(n2), rng.integers(0, n2, n1 - n2)])
        Xc2 = np.stack([rng.uniform(-6, 6, n2), rng.uniform(-2, 2, n2), rng.uniform(5, 30, n2)], axis=1)
        good = rng.random(n1) >= 0.3
        Xc2[perm[good]] = ((Xc1[good] - ts) @ Rs) / s + rng.normal(scale=0.002, size=(int(good.sum()), 3))      # x1 = s R x2 + t
        W2 = (Xc2 - T2[:3, 3]) @ T2[:3, :3]
        for jj in range(n2):
            points[int(k2["mp_id"][jj])] = dict(pos=W2[jj].astype(np.float32), bad=False, obs={22 + c: jj, 5: 1})
        m = k2["mp_id"][perm].copy()
        points[int(m[cases["bad2"]])]["bad"] = True
        m[cases["unknown_id"]] = 77777777
        m[cases["not_matched"]] = R.NO_MAP_POINT
        points[int(m[cases["not_observing2"]])]["obs"] = {5: 1}
        kfs2.append(k2); matched.append(m)
    return dict(kf1=kf1, kfs2=kfs2, matched=np.array(matched, np.uint64), points=points, scale=scale, cases=cases, rand=R.draws(seed, n_cand, 300))

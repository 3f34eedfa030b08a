"""The seeded cases of test_gpu_pnp_ransac.py (built once; test_pnpsolver_reference.py checks on the CPU that they are what they claim to be)."""
import functools
import itertools
import numpy as np
import pnpsolver_reference as R

PARAMS = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991)       # Tracking::Relocalization / MapFusion


def force(rv, it, members, N):
    """make iteration `it` draw the ascending set `members`, all below N - len(members) (positions = values: no swapped entry is touched)"""
    members = list(members); k = len(members)
    assert all(a < b for a, b in zip(members, members[1:])) and members[-1] < N - k
    rv[it] = [int((a + 0.5) / (N - j) * R.RAND_RANGE) for j, a in enumerate(members)]
    assert R.draw_set(rv[it], k, N) == members


def _case(seed, Ns, shares, noises, tail=0, **kw):
    p = dict(PARAMS); p.update(kw)
    prs = [R.scene(seed + 10 * k, n, sh, nz)[0] for k, (n, sh, nz) in enumerate(zip(Ns, shares, noises))]
    return dict(problems=prs, rand=R.draws(seed, len(Ns), p["max_iterations"] + tail, p["min_set"]), tail=tail, params=p)


@functools.lru_cache(maxsize=None)
def special():
    """one problem of 40 correspondences whose first iterations are forced: (0) four coplanar world points, (1) a sample holding the same correspondence twice (rows 4 and
    5 are equal: a rank-deficient PW0tPW0), (2) a clean sample whose pose puts correspondence 20 on the camera plane -- Zc as close to 0 as a float position allows --
    and (3) four equal correspondences (rows 12-15): a non-finite pose.  Returns (problem, forced sets, rand_values [1, 300, 4])"""
    pr, truth = R.scene(900, 40, 1.0, 0.0)
    X = pr["p3dw"].astype(np.float64).copy(); uv = pr["p2d"].astype(np.float64).copy()
    Rt, tt = truth["R"], truth["t"]
    fx, fy, cx, cy = R.KITTI

    def reproject(i):
        Xc = Rt @ np.float64(np.float32(X[i])) + tt
        uv[i] = [fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy]
    # (0) rows 0-3: world z exactly 2
    for i in range(4):
        X[i, 2] = 2.0; reproject(i)
    # (1) rows 4 == 5
    X[5] = X[4]; uv[5] = uv[4]
    # (3) rows 12-15 equal
    for i in (13, 14, 15):
        X[i] = X[12]; uv[i] = uv[12]
    sets = [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]]
    pr = R.problem(X, uv, pr["sigma2"], R.KITTI)
    # (2) row 20 on the camera plane of the pose of sample 2
    h = R.compute_pose(*[x[None] for x in R.gather_sets(pr, sets[2])], pr["K"])
    R2, t2 = h["R"][0], h["t"][0]
    Xc = np.array([1.0, -0.5, 0.0])
    X[20] = R2.T @ (Xc - t2)
    pr = R.problem(X, uv, pr["sigma2"], R.KITTI)
    rv = R.draws(900, 1, 300)
    for it, s in enumerate(sets):
        force(rv[0], it, s, 40)
    return pr, sets, rv


@functools.lru_cache(maxsize=None)
def refine_scenes():
    """scenes whose first record has exactly 10, 64 and 65 inliers: that many noise-free correspondences, every other pixel unrelated, the first iteration forced onto four
    of the true ones; N = 20, 128, 129"""
    out = []
    for k, (n, n_in) in enumerate(((20, 10), (128, 64), (129, 65))):            # mRansacMinInliers = max(int(N * 0.5), 10) = 10, 64, 64
        pr, truth = R.scene(950 + k, n, n_inliers=n_in)
        rv = R.draws(950 + k, 1, 300)
        inl = np.flatnonzero(truth["inlier"])
        # four noise-free points do not always give the pose: take the first of 60 subsets of the true ones that does
        cand = np.array(list(itertools.islice(itertools.combinations([int(i) for i in inl[inl < n - 4]], 4), 60)), np.int64)
        h = R.compute_pose(*R.gather_sets(pr, cand), pr["K"])
        good = np.flatnonzero(R.check_inliers(pr, h["R"], h["t"]).sum(axis=1) == n_in)
        force(rv[0], 0, [int(i) for i in cand[good[0]]], n)
        out.append((pr, rv, n_in))
    return out


@functools.lru_cache(maxsize=None)
def host_cases():
    c = {}
    Ns = [9, 10, 11, 63, 64, 65, 129, 300]
    c["eight"] = _case(100, Ns, [1.0, 1.0, 0.9, 0.5, 0.9, 0.5, 0.0, 0.5], [0.0, 0.0, 0.5, 0.0, 0.5, 0.5, 0.0, 0.5])
    c["eight_tail"] = _case(200, Ns, [0.9, 0.9, 0.5, 0.9, 0.0, 0.9, 0.5, 0.9], [0.5, 0.5, 0.0, 0.5, 0.0, 0.0, 0.5, 0.0], tail=5)
    c["single_iteration"] = _case(300, [64, 30], [0.9, 0.5], [0.0, 0.5], max_iterations=1)
    c["min_set_6"] = _case(400, [65, 129], [0.9, 0.5], [0.5, 0.0], tail=5, min_set=6)
    c["epsilon_02"] = _case(500, [129, 300], [0.6, 0.6], [1.5, 1.5], epsilon=0.2)       # 1.5 px of noise: partial fits, so the running best improves four and five times
    pr, sets, rv = special()
    c["special"] = dict(problems=[pr], rand=rv, tail=0, params=dict(PARAMS))
    rs = refine_scenes()
    c["refine_sets"] = dict(problems=[r[0] for r in rs], rand=np.concatenate([r[1] for r in rs]), tail=0, params=dict(PARAMS))
    return c


@functools.lru_cache(maxsize=None)
def record_scene(seed=700, n=150, n_cand=3):
    """a frame record of n features and n_cand rows of vvpMapPointMatches: candidate c matches feature i with map point 1000 * (c + 1) + i, seen at the feature's pixel by
    the frame's true pose for 90 / 60 / 30 % of the features.  The filter cases of the constructor sit at fixed features (see `cases`)."""
    rng = np.random.default_rng(seed)
    scale = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    K = (700.0, 705.0, 600.0, 180.0)
    Rt = R._rot(rng, 0.4); tt = rng.uniform(-0.5, 0.5, 3)
    Xc = np.stack([rng.uniform(-6, 6, n), rng.uniform(-2, 2, n), rng.uniform(5, 30, n)], axis=1)
    kp = np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1).astype(np.float32)
    octave = rng.integers(0, 8, n).astype(np.int32)
    cases = dict(bad=3, unknown_id=12, no_mp=18)
    points, matched = {}, []
    for c in range(n_cand):
        W = (Xc - tt) @ Rt
        wrong = rng.random(n) >= (0.9, 0.6, 0.3)[c % 3]
        W[wrong] = rng.uniform(-8, 8, (int(wrong.sum()), 3))
        ids = (1000 * (c + 1) + np.arange(n)).astype(np.uint64)
        for i in range(n):
            points[int(ids[i])] = dict(pos=W[i].astype(np.float32), bad=False)
        points[int(ids[cases["bad"]])]["bad"] = True
        ids[cases["unknown_id"]] = 77777777
        ids[cases["no_mp"]] = R.NO_MAP_POINT
        matched.append(ids)
    return dict(kp=kp, octave=octave, K=K, points=points, matched=np.array(matched, np.uint64), scale=scale, cases=cases, rand=R.draws(seed, n_cand, 305), tail=5,
                params=dict(PARAMS))

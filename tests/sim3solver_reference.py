"""numpy restatement of Sim3Solver (C/src/Sim3Solver.cc): the constructor's arithmetic and filter (:37-112), the draw mapping (:163-177 with DUtils::Random::RandomInt),
SetRansacParameters' cap (:114-138), ComputeSim3 (:226-337), CheckInliers (:340-364) and the rule that turns per-hypothesis inlier counts into iterate()'s returns
(:158-201).  Every float expression keeps the C++ type of the source and is evaluated unfused; the readings of the OpenCV calls and the two choices the reference
cannot pin (cv::eigen -> cyclic Jacobi in float64; atan2 + cv::Rodrigues -> the algebraic rotation in float64) are those of DESIGN.md section 2, and this file is their
definition.  compute_sim3(..., q=...) evaluates everything downstream of a GIVEN quaternion: the GPU tests pass the device's."""
import math
import numpy as np
import ransac_reference

f32, f64 = np.float32, np.float64
NAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
NO_MAP_POINT = 0xFFFFFFFFFFFFFFFF
MP_BAD = 1
RAND_RANGE = 2 ** 31                          # RAND_MAX + 1


def thresholds(sigma2):
    """mvnMaxError: vector<size_t>::push_back(9.210 * sigmaSquare) -- double x float, truncated to an integer; compared as float (:87-88, :356)"""
    return np.floor(f64(9.210) * np.asarray(sigma2, f32).astype(f64)).astype(f32)


def gemm_rows(R, X, t=None):
    """rows of R * x (+ t) for every row x of X: cv::gemm on floats -- double accumulation left to right, one rounding"""
    R = np.asarray(R, f32).astype(f64); X = np.asarray(X, f32).reshape(-1, 3).astype(f64)
    out = np.empty((len(X), 3), f32)
    for i in range(3):
        s = R[i, 0] * X[:, 0]
        s = s + R[i, 1] * X[:, 1]
        s = s + R[i, 2] * X[:, 2]
        if t is not None:
            s = s + f64(f32(t[i]))
        out[:, i] = s.astype(f32)
    return out


def project(X, K):
    """FromCameraToImage / Project (:382-423): const float invz = 1 / z; K = (fx, fy, cx, cy)"""
    X = np.asarray(X, f32).reshape(-1, 3); fx, fy, cx, cy = [f32(k) for k in K]
    with np.errstate(all="ignore"):
        invz = f32(1) / X[:, 2]
        x = X[:, 0] * invz; y = X[:, 1] * invz
        return np.stack([fx * x + cx, fy * y + cy], axis=1).astype(f32)


def problem(p1c, p2c, sigma2_1, sigma2_2, K1, K2):
    """what the constructor leaves for N given correspondences"""
    p1c = np.ascontiguousarray(p1c, f32).reshape(-1, 3); p2c = np.ascontiguousarray(p2c, f32).reshape(-1, 3)
    return dict(n=len(p1c), x1=p1c, x2=p2c, p1c=p1c, p2c=p2c, p1=project(p1c, K1), p2=project(p2c, K2), th1=thresholds(sigma2_1), th2=thresholds(sigma2_2),
                sigma2_1=np.ascontiguousarray(sigma2_1, f32), sigma2_2=np.ascontiguousarray(sigma2_2, f32), K1=tuple(f32(k) for k in K1), K2=tuple(f32(k) for k in K2))


def draw_triple(r, N):
    """three picks without replacement from vAvailableIndices = 0 .. N-1 (:163-177): ransac_reference's draw rule for a set of 3"""
    return tuple(ransac_reference.draw_set(r, 3, N))


def draw_triple_literal(r, N):
    return tuple(ransac_reference.draw_set_literal(r, 3, N))


def ransac_cap(N, probability=0.99, min_inliers=20, max_iterations=300):
    """mRansacMaxIts (:125-135); 0 = iterate() sets bNoMore at once (:146-150)"""
    if N < min_inliers:
        return 0
    if min_inliers == N:
        nit = 1
    else:
        eps = f32(min_inliers) / f32(N)
        x = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(eps), 3.0)))
        nit = max_iterations if not x < max_iterations else (1 if x < 1 else int(x))
    return max(1, min(nit, max_iterations))


def _centroid(P):
    """ComputeCentroid (:215-224), P[k] = point k: cv::reduce sums in float left to right; C / P.cols multiplies by the double 1.0 / 3, one rounding"""
    s = (P[0] + P[1]) + P[2]
    C = (s.astype(f64) * (f64(1.0) / f64(3.0))).astype(f32)
    return P - C, C


def horn_N(P1, P2):
    """steps 1-3 (:231-265): returns (N float32 4x4, Pr1, Pr2, O1, O2); P[k] = column k of P3Dc*i"""
    P1 = np.asarray(P1, f32).reshape(3, 3); P2 = np.asarray(P2, f32).reshape(3, 3)
    Pr1, O1 = _centroid(P1); Pr2, O2 = _centroid(P2)
    M = np.empty((3, 3), f32)
    for i in range(3):
        for j in range(3):
            s = f64(Pr2[0, i]) * f64(Pr1[0, j])
            s = s + f64(Pr2[1, i]) * f64(Pr1[1, j])
            s = s + f64(Pr2[2, i]) * f64(Pr1[2, j])
            M[i, j] = f32(s)
    N = np.empty((4, 4), f32)                    # (:251-260) float expressions; the double variables receive float results
    N[0, 0] = (M[0, 0] + M[1, 1]) + M[2, 2]
    N[0, 1] = M[1, 2] - M[2, 1]
    N[0, 2] = M[2, 0] - M[0, 2]
    N[0, 3] = M[0, 1] - M[1, 0]
    N[1, 1] = (M[0, 0] - M[1, 1]) - M[2, 2]
    N[1, 2] = M[0, 1] + M[1, 0]
    N[1, 3] = M[2, 0] + M[0, 2]
    N[2, 2] = (-M[0, 0] + M[1, 1]) - M[2, 2]
    N[2, 3] = M[1, 2] + M[2, 1]
    N[3, 3] = (-M[0, 0] - M[1, 1]) + M[2, 2]
    for i in range(4):
        for j in range(i):
            N[i, j] = N[j, i]
    return N, Pr1, Pr2, O1, O2


def jacobi_top(N):
    """cv::eigen's first eigenvector: cyclic Jacobi on N in float64.  A pair (p, q) is rotated iff |a_pq| > 2^-60 max|N_ij|; sweeps end when one rotates no pair, at
    most 30; the column of the largest diagonal entry (lowest index on ties), rounded to float"""
    A = np.asarray(N, f32).astype(f64).copy(); V = np.eye(4, dtype=f64)
    with np.errstate(all="ignore"):
        scale = f64(0)
        for v in np.abs(A).ravel():
            if v > scale:
                scale = v
        tiny = scale * f64(2.0 ** -60)
        for sweep in range(30):
            rotated = False
            for p in range(3):
                for q in range(p + 1, 4):
                    apq = A[p, q]
                    if not abs(apq) > tiny:
                        continue
                    rotated = True
                    app, aqq = A[p, p], A[q, q]
                    theta = (aqq - app) / (f64(2.0) * apq)
                    t = (f64(1.0) if theta >= 0 else f64(-1.0)) / (abs(theta) + np.sqrt(theta * theta + f64(1.0)))
                    c = f64(1.0) / np.sqrt(t * t + f64(1.0)); s = t * c
                    A[p, p] = app - t * apq; A[q, q] = aqq + t * apq; A[p, q] = A[q, p] = 0.0
                    for k in range(4):
                        if k != p and k != q:
                            akp, akq = A[k, p], A[k, q]
                            A[k, p] = A[p, k] = c * akp - s * akq
                            A[k, q] = A[q, k] = s * akp + c * akq
                        vkp, vkq = V[k, p], V[k, q]
                        V[k, p] = c * vkp - s * vkq; V[k, q] = s * vkp + c * vkq
            if not rotated:
                break
    jb = 0
    for j in range(1, 4):
        if A[j, j] > A[jb, jb]:
            jb = j
    return V[:, jb].astype(f32)


def rotation(q):
    """atan2 + cv::Rodrigues (:278-284) written algebraically from the float quaternion, in double: R = I + (2 q0 [v]x + 2 [v]x^2) / |q|^2, each entry rounded once"""
    q0, v1, v2, v3 = [f64(f32(x)) for x in q]
    two, one = f64(2.0), f64(1.0)
    with np.errstate(all="ignore"):
        vv = v1 * v1; vv = vv + v2 * v2; vv = vv + v3 * v3
        n2 = q0 * q0 + vv; a = two * q0
        R = [[one + (two * (v1 * v1 - vv)) / n2, (a * (-v3) + two * (v1 * v2)) / n2, (a * v2 + two * (v1 * v3)) / n2],
             [(a * v3 + two * (v2 * v1)) / n2, one + (two * (v2 * v2 - vv)) / n2, (a * (-v1) + two * (v2 * v3)) / n2],
             [(a * (-v2) + two * (v3 * v1)) / n2, (a * v1 + two * (v3 * v2)) / n2, one + (two * (v3 * v3 - vv)) / n2]]
        return np.array(R, f64).astype(f32)


def compute_sim3(P1, P2, fix_scale=False, q=None):
    """ComputeSim3 (:226-337).  Returns dict(N, q, R, t, s, ok); not ok (R, t, s = NaN): the quaternion's vector part is zero, or R, t or s is not finite"""
    N, Pr1, Pr2, O1, O2 = horn_N(P1, P2)
    q = jacobi_top(N) if q is None else np.asarray(q, f32)
    R = rotation(q)
    with np.errstate(all="ignore"):
        s12 = f32(1.0)
        if not fix_scale:
            P3 = np.empty((3, 3), f32)               # P3 = mR12i * Pr2; P3[i, k] = row i, column (point) k
            for i in range(3):
                for k in range(3):
                    s = f64(R[i, 0]) * f64(Pr2[k, 0])
                    s = s + f64(R[i, 1]) * f64(Pr2[k, 1])
                    s = s + f64(R[i, 2]) * f64(Pr2[k, 2])
                    P3[i, k] = f32(s)
            nom = den = None                         # Mat::dot: a double sum in memory order; cv::pow(P3, 2) = the float product
            for i in range(3):
                for k in range(3):
                    pn = f64(Pr1[k, i]) * f64(P3[i, k]); pd = f64(f32(P3[i, k] * P3[i, k]))
                    nom = pn if nom is None else nom + pn
                    den = pd if den is None else den + pd
            s12 = f32(nom / den)
        t = np.empty(3, f32)                         # mt12i = O1 - ms12i * mR12i * O2: one gemm, alpha = -s, beta = 1
        for i in range(3):
            s = f64(R[i, 0]) * f64(O2[0])
            s = s + f64(R[i, 1]) * f64(O2[1])
            s = s + f64(R[i, 2]) * f64(O2[2])
            t[i] = f32(f64(O1[i]) - f64(s12) * s)
    ok = bool(q[1] != 0 or q[2] != 0 or q[3] != 0) and bool(np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s12))
    if not ok:
        R = np.full((3, 3), NAN32, f32); t = np.full(3, NAN32, f32); s12 = NAN32
    return dict(N=N, q=q, R=R, t=t, s=f32(s12), ok=ok)


def check_inliers(pr, h):
    """CheckInliers (:340-364) for hypothesis h = compute_sim3(...): bool per correspondence"""
    if not h["ok"]:
        return np.zeros(pr["n"], bool)
    R, t, s = h["R"], h["t"], h["s"]
    with np.errstate(all="ignore"):
        sR = (s * R).astype(f32)                                                 # ms12i * mR12i: a float product per entry
        alpha = f64(1.0) / f64(s)
        sRinv = (alpha * R.T.astype(f64)).astype(f32)                            # (1.0 / ms12i) * mR12i.t(): the double reciprocal times the entry, one rounding
        tinv = np.empty(3, f32)
        for i in range(3):
            a = f64(sRinv[i, 0]) * f64(t[0])
            a = a + f64(sRinv[i, 1]) * f64(t[1])
            a = a + f64(sRinv[i, 2]) * f64(t[2])
            tinv[i] = f32(-a)
        uv = project(gemm_rows(sR, pr["x2"], t), pr["K1"])
        d1 = pr["p1"] - uv
        err1 = (d1[:, 0].astype(f64) * d1[:, 0].astype(f64) + d1[:, 1].astype(f64) * d1[:, 1].astype(f64)).astype(f32)
        uv = project(gemm_rows(sRinv, pr["x1"], tinv), pr["K2"])
        d2 = uv - pr["p2"]
        err2 = (d2[:, 0].astype(f64) * d2[:, 0].astype(f64) + d2[:, 1].astype(f64) * d2[:, 1].astype(f64)).astype(f32)
        return (err1 < pr["th1"]) & (err2 < pr["th2"])


def events_of(counts, min_inliers):
    """iteration i (0-based) returns iff c_i > minInliers and c_i >= max_{j<i} c_j"""
    out = []; best = 0
    for i, c in enumerate(counts):
        if c >= best:
            best = c
            if c > min_inliers:
                out.append(i)
    return out


def iterate_literal(counts, cap, min_inliers, chunk):
    """a literal transcription of iterate(chunk) (:140-207) called until bNoMore, over given per-iteration counts: the 1-based mnIterations of every return"""
    st = dict(mnIterations=0, mnBestInliers=0)

    def iterate(nIterations):
        nCurrentIterations = 0
        while st["mnIterations"] < cap and nCurrentIterations < nIterations:
            nCurrentIterations += 1; st["mnIterations"] += 1
            mnInliersi = counts[st["mnIterations"] - 1]
            if mnInliersi >= st["mnBestInliers"]:
                st["mnBestInliers"] = mnInliersi
                if mnInliersi > min_inliers:
                    return True, False
        return False, st["mnIterations"] >= cap

    returns = []
    while True:
        found, bNoMore = iterate(chunk)
        if found:
            returns.append(st["mnIterations"])
        if bNoMore or st["mnIterations"] >= cap:
            return returns


def ransac(pr, rand_values, probability=0.99, min_inliers=20, max_iterations=300, fix_scale=False, q_dev=None):
    """everything a call returns for one problem: dict(cap, counts, q, events = [dict(iteration, n_inliers, R, t, s, flags)], N matrices); q_dev: per-iteration quaternions
    to evaluate downstream of (the device's)"""
    N = pr["n"]; cap = ransac_cap(N, probability, min_inliers, max_iterations)
    rv = np.asarray(rand_values).reshape(-1, 3)
    hyps, flags = [], []
    for it in range(cap):
        idx = draw_triple(rv[it], N)
        h = compute_sim3(pr["x1"][list(idx)], pr["x2"][list(idx)], fix_scale, None if q_dev is None else q_dev[it])
        hyps.append(h); flags.append(check_inliers(pr, h))
    counts = np.array([int(f.sum()) for f in flags], np.int32)
    ev = [dict(iteration=i + 1, n_inliers=int(counts[i]), R=hyps[i]["R"], t=hyps[i]["t"], s=hyps[i]["s"], flags=flags[i]) for i in events_of(counts, min_inliers)]
    return dict(cap=cap, counts=counts, q=np.array([h["q"] for h in hyps], f32).reshape(-1, 4), events=ev, N=[h["N"] for h in hyps], ok=[h["ok"] for h in hyps])


def eigen_gap(N):
    """(top eigenvector by float64 eigh, relative gap (l1 - l2) / max|l|) of the float matrix N"""
    w, v = np.linalg.eigh(np.asarray(N, f32).astype(f64))
    return v[:, 3], (w[3] - w[2]) / max(np.abs(w).max(), 1e-300)


# ---- scenes ----
KITTI = (718.856, 718.856, 607.1928, 185.2157)


def _rot(rng, max_angle):
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax); ang = rng.uniform(0.05, max_angle)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def scene(seed, n, outlier_share=0.3, noise=0.002, scale=1.0, max_angle=0.6):
    """n correspondences of a known similarity X1 = s R X2 + t in front of two KITTI-calibrated cameras; a share of them replaced by unrelated points.
    Returns (problem, truth dict(s, R, t))"""
    rng = np.random.default_rng(seed)
    R = _rot(rng, max_angle); t = rng.uniform(-0.5, 0.5, 3); s = float(scale)
    X2 = np.stack([rng.uniform(-6, 6, n), rng.uniform(-2, 2, n), rng.uniform(5, 30, n)], axis=1)
    X1 = s * X2 @ R.T + t + rng.normal(scale=noise, size=(n, 3))
    out = rng.random(n) < outlier_share
    X1[out] = np.stack([rng.uniform(-6, 6, out.sum()), rng.uniform(-2, 2, out.sum()), rng.uniform(5, 30, out.sum())], axis=1)
    sig = (np.float32(1.2) ** rng.integers(0, 4, (2, n)).astype(np.float32)) ** 2
    return problem(X1, X2, sig[0].astype(f32), sig[1].astype(f32), KITTI, KITTI), dict(s=s, R=R, t=t)


def draws(seed, n_problems, max_iterations):
    return np.random.RandomState(seed).randint(0, RAND_RANGE, (n_problems, max_iterations, 3)).astype(np.int32)


# ---- the constructor on records (:37-112) ----
def constructor(kf1, kf2, points, matched12, scale1, scale2):
    """kf = dict(id, Tcw 4x4, K, octave [n] (mvKeysUn[.].octave), mp_id [n] uint64); points = {id: dict(pos, bad, obs = {kf id: feature index})};
    matched12 = MapPoint id per feature of KF1 (NO_MAP_POINT = NULL); scale = mvScaleFactors.  Returns (problem, mvnIndices1)"""
    idx1, X1, X2, s1, s2 = [], [], [], [], []
    n1, n2 = len(kf1["mp_id"]), len(kf2["mp_id"])
    sc1 = np.asarray(scale1, f32); sc2 = np.asarray(scale2, f32)
    for i1 in range(n1):
        id2, id1 = int(matched12[i1]), int(kf1["mp_id"][i1])
        if id2 == NO_MAP_POINT or id1 == NO_MAP_POINT or id1 not in points or id2 not in points:
            continue
        m1, m2 = points[id1], points[id2]
        if m1["bad"] or m2["bad"]:
            continue
        k1 = m1["obs"].get(kf1["id"], -1); k2 = m2["obs"].get(kf2["id"], -1)
        if not (0 <= k1 < n1 and 0 <= k2 < n2):
            continue
        o1 = min(max(int(kf1["octave"][k1]), 0), len(sc1) - 1); o2 = min(max(int(kf2["octave"][k2]), 0), len(sc2) - 1)
        idx1.append(i1); X1.append(m1["pos"]); X2.append(m2["pos"]); s1.append(sc1[o1] * sc1[o1]); s2.append(sc2[o2] * sc2[o2])
    T1 = np.asarray(kf1["Tcw"], f32).reshape(4, 4); T2 = np.asarray(kf2["Tcw"], f32).reshape(4, 4)
    x1 = gemm_rows(T1[:3, :3], np.array(X1, f32).reshape(-1, 3), T1[:3, 3]); x2 = gemm_rows(T2[:3, :3], np.array(X2, f32).reshape(-1, 3), T2[:3, 3])
    return problem(x1, x2, np.array(s1, f32), np.array(s2, f32), kf1["K"], kf2["K"]), np.array(idx1, np.int32)

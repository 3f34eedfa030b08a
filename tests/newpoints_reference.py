"""numpy restatement of the triangulation loop of LocalMapping::CreateNewMapPoints (C/src/LocalMapping.cc:262-418), one float32 / float64 operation at a time, plus the
seeded scene generator the CPU and GPU tests share.  Conventions: the reference's float expressions with the C++ types of the source;
cv::Mat products = cv::gemm (double accumulation, one rounding), cv::norm / Mat::dot = double sums; the stereo parallax cos(2 atan2(mb / 2, depth)) =
(d*d - h*h) / (d*d + h*h) in double, rounded once; x3D = v[0:3] / v[3] in float with v the float-rounded null vector of the float 4x4 A."""
import numpy as np

f32, f64 = np.float32, np.float64
OK, NO_PARALLAX, W_ZERO, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, SCALE = range(8)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
NO_MAP_POINT = 0xFFFFFFFFFFFFFFFF
KITTI = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, bf=386.1448)


def _acc(a, b, c=None):
    """(float)(sum of (double)a[k] * (double)b[k] [+ (double)c]) accumulated in order"""
    s = f64(0)
    for x, y in zip(a, b):
        s = s + f64(x) * f64(y)
    if c is not None:
        s = s + f64(c)
    return s


def _norm(v):
    return np.sqrt(f64(v[0]) * f64(v[0]) + f64(v[1]) * f64(v[1]) + f64(v[2]) * f64(v[2]))


class _Cam:
    def __init__(self, k):
        self.T = np.asarray(k["Tcw"], f32).reshape(4, 4)
        self.fx, self.fy, self.cx, self.cy = (f32(k[n]) for n in ("fx", "fy", "cx", "cy"))
        self.invfx, self.invfy = f32(1) / self.fx, f32(1) / self.fy
        self.Ow = camera_centre(self.T)


def camera_centre(T):
    """Ow = -Rcw^T tcw: exact negation of the transposed rotation, then gemm"""
    T = np.asarray(T, f32).reshape(4, 4)
    return np.array([f32(_acc([-T[q, i] for q in range(3)], [T[q, 3] for q in range(3)])) for i in range(3)], f32)


def _xn(c, kp):
    return [(f32(kp["x"]) - c.cx) * c.invfx, (f32(kp["y"]) - c.cy) * c.invfy, f32(1)]


def matrix_A(kf1, kf2, idx1, idx2):
    """the float 4x4 system of :299-303"""
    c1, c2 = _Cam(kf1), _Cam(kf2)
    x1, x2 = _xn(c1, kf1["kp"][idx1]), _xn(c2, kf2["kp"][idx2])
    A = np.zeros((4, 4), f32)
    for k in range(4):
        A[0, k] = x1[0] * c1.T[2, k] - c1.T[0, k]; A[1, k] = x1[1] * c1.T[2, k] - c1.T[1, k]
        A[2, k] = x2[0] * c2.T[2, k] - c2.T[0, k]; A[3, k] = x2[1] * c2.T[2, k] - c2.T[1, k]
    return A


def svd_point(A):
    """right singular vector of the smallest singular value of the float32 A, by numpy's SVD in float64"""
    return np.linalg.svd(np.asarray(A, f32).astype(f64))[2][-1]


def _cos_stereo(mb, depth):
    h, d = f64(f32(mb) / f32(2)), f64(f32(depth))
    return f32((d * d - h * h) / (d * d + h * h))


def _unproject(c, kp, z):
    z = f32(z)
    x = (f32(kp["x"]) - c.cx) * z * c.invfx; y = (f32(kp["y"]) - c.cy) * z * c.invfy
    return np.array([f32(f64(c.T[0, i]) * f64(x) + f64(c.T[1, i]) * f64(y) + f64(c.T[2, i]) * f64(z) + f64(c.Ow[i])) for i in range(3)], f32)


def _reproj_ok(c, X, z, kp, ur, stereo, bf, sigma2):
    x = f32(_acc(c.T[0, :3], X, c.T[0, 3])); y = f32(_acc(c.T[1, :3], X, c.T[1, 3]))
    invz = f32(f64(1) / f64(z))
    u = c.fx * x * invz + c.cx; v = c.fy * y * invz + c.cy
    ex, ey = u - f32(kp["x"]), v - f32(kp["y"])
    if not stereo:
        return not (f64(ex * ex + ey * ey) > f64(5.991) * f64(sigma2))
    er = (u - f32(bf) * invz) - f32(ur)
    return not (f64(ex * ex + ey * ey + er * er) > f64(7.8) * f64(sigma2))


def decide_pair(kf1, kf2, idx1, idx2, x3d_svd=None, v_svd=None):
    """one pair of :268-398 -> (x3D float32[3], status, source).  x3d_svd: use this point for the SVD branch; v_svd: use this null vector (4) instead of computing it"""
    c1, c2 = _Cam(kf1), _Cam(kf2)
    k1, k2 = kf1["kp"][idx1], kf2["kp"][idx2]
    ur1, ur2 = f32(kf1["u_right"][idx1]), f32(kf2["u_right"][idx2])
    st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)
    Z = np.zeros(3, f32)
    x1, x2 = _xn(c1, k1), _xn(c2, k2)
    ray1 = [f32(_acc(c1.T[:3, i], x1)) for i in range(3)]; ray2 = [f32(_acc(c2.T[:3, i], x2)) for i in range(3)]
    cos_rays = f32(_acc(ray1, ray2) / (_norm(ray1) * _norm(ray2)))
    cos1 = cos_rays + f32(1); cos2 = cos1
    if st1:
        cos1 = _cos_stereo(kf1["mb"], kf1["depth"][idx1])
    elif st2:
        cos2 = _cos_stereo(kf2["mb"], kf2["depth"][idx2])
    cos_stereo = min(cos1, cos2)
    source = 0
    if cos_rays < cos_stereo and cos_rays > 0 and (st1 or st2 or f64(cos_rays) < f64(0.9998)):
        if x3d_svd is not None and v_svd is None:
            X = np.asarray(x3d_svd, f32).copy()
        else:
            v = (np.asarray(v_svd, f64) if v_svd is not None else svd_point(matrix_A(kf1, kf2, idx1, idx2))).astype(f32)
            if v[3] == 0:
                return Z, W_ZERO, 0
            X = np.array([v[0] / v[3], v[1] / v[3], v[2] / v[3]], f32)
    elif st1 and cos1 < cos2 and f32(kf1["depth"][idx1]) > 0:
        X = _unproject(c1, k1, kf1["depth"][idx1]); source = 1
    elif st2 and cos2 < cos1 and f32(kf2["depth"][idx2]) > 0:
        X = _unproject(c2, k2, kf2["depth"][idx2]); source = 2
    else:
        return Z, NO_PARALLAX, 0
    z1 = f32(_acc(c1.T[2, :3], X, c1.T[2, 3]))
    if z1 <= 0:
        return X, BEHIND_1, source
    z2 = f32(_acc(c2.T[2, :3], X, c2.T[2, 3]))
    if z2 <= 0:
        return X, BEHIND_2, source
    s1, s2 = np.asarray(kf1["scale"], f32), np.asarray(kf2["scale"], f32)
    sc1 = s1[min(max(int(k1["octave"]), 0), len(s1) - 1)]; sc2 = s2[min(max(int(k2["octave"]), 0), len(s2) - 1)]
    if not _reproj_ok(c1, X, z1, k1, ur1, st1, kf1["bf"], sc1 * sc1):
        return X, REPROJ_1, source
    if not _reproj_ok(c2, X, z2, k2, ur2, st2, kf1["bf"], sc2 * sc2):          # (:372: the CURRENT keyframe's mbf)
        return X, REPROJ_2, source
    d1 = f32(_norm(X - c1.Ow)); d2 = f32(_norm(X - c2.Ow))
    if d1 == 0 or d2 == 0:
        return X, SCALE, source
    ratio_dist = d2 / d1; ratio_factor = f32(1.5) * s1[1 if len(s1) > 1 else 0]; ratio_octave = sc1 / sc2
    if ratio_dist * ratio_factor < ratio_octave or ratio_dist > ratio_octave * ratio_factor:
        return X, SCALE, source
    return X, OK, source


def decide(kf1, kf2, pairs, x3d_svd=None):
    """:268-398 for every pair -> (x3D [n, 3] float32, status uint8, source uint8).  x3d_svd [n, 3]: the points to use where the SVD branch is taken."""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    X = np.zeros((len(pairs), 3), f32); st = np.zeros(len(pairs), np.uint8); src = np.zeros(len(pairs), np.uint8)
    for i, (a, b) in enumerate(pairs):
        X[i], st[i], src[i] = decide_pair(kf1, kf2, int(a), int(b), None if x3d_svd is None else x3d_svd[i])
    return X, st, src


def new_map_point(cur, nb, idx1, idx2, X, mp_id, client_id):
    """the record of `new MapPoint(x3D, mpCurrentKeyFrame)` + two AddObservation + ComputeDistinctiveDescriptors + UpdateNormalAndDepth (:401-411)"""
    obs = sorted([(int(cur["id"]), int(idx1), cur), (int(nb["id"]), int(idx2), nb)], key=lambda o: o[0])
    X = np.asarray(X, f32)
    normal = np.zeros(3, f32); norms = []
    for _, _, k in obs:
        v = X - camera_centre(k["Tcw"]); n = _norm(v); norms.append(n); inv = f64(1) / n
        normal = np.array([normal[a] + f32(f64(v[a]) * inv) for a in range(3)], f32)
    normal = np.array([f32(f64(normal[a]) * (f64(1) / f64(2))) for a in range(3)], f32)
    dist = f32(norms[0] if obs[0][2] is cur else norms[1])
    sc = np.asarray(cur["scale"], f32)
    level = min(max(int(cur["kp"]["octave"][idx1]), 0), len(sc) - 1)
    mx = dist * sc[level]
    return dict(id=int(mp_id), ref_kf_id=int(cur["id"]), client_id=int(client_id), world_pos=X.copy(), obs=[(o[0], o[1]) for o in obs],
                descriptor=np.asarray(obs[0][2]["desc"][obs[0][1]], np.uint8).copy(), normal=normal, min_distance=mx / sc[len(sc) - 1], max_distance=mx)


def create_new_map_points(pyorc, cur, nbs, F12, epipoles, only_stereo=False, x3d_svd=None, first_mp_id=0, client_id=0):
    """The neighbour loop (:219-419) as the reference runs it: SearchForTriangulation per neighbour against flags that evolve, the pairs triangulated in order.
    x3d_svd: {(j, idx1, idx2): x3D} to use where the SVD branch is taken.  Returns dict(pair_offset, pairs, x3d, status, source, n_new, records, flags, mp_ids)
    with flags / mp_ids the per-feature state of [cur] + nbs afterwards."""
    scale = np.asarray(cur["scale"], f32); sigma2 = scale * scale
    flags = [np.array(k["has_mp"], np.uint8, copy=True) for k in [cur] + list(nbs)]
    ids = [np.array(k.get("mp_id", np.full(len(k["kp"]), NO_MAP_POINT, np.uint64)), np.uint64, copy=True) for k in [cur] + list(nbs)]
    off = [0]; P = []; X = []; S = []; R = []; recs = []
    for j, nb in enumerate(nbs):
        pr, n = pyorc.search_for_triangulation(cur["desc"], cur["kp"], cur["u_right"], flags[0], pyorc.FeatVec(*cur["fv"]), nb["desc"], nb["kp"], nb["u_right"], flags[j + 1],
                                               pyorc.FeatVec(*nb["fv"]), np.asarray(F12[j], f32), float(epipoles[j][0]), float(epipoles[j][1]), scale, sigma2, only_stereo, False)
        pr = np.asarray(pr, np.int32).reshape(-1, 2)
        pr = pr[np.argsort(pr[:, 0], kind="stable")]
        for a, b in pr:
            x, st, src = decide_pair(cur, nb, int(a), int(b), None if x3d_svd is None else x3d_svd.get((j, int(a), int(b))))
            P.append((int(a), int(b))); X.append(x); S.append(st); R.append(src)
            if st == OK:
                mid = first_mp_id + len(recs)
                recs.append(new_map_point(cur, nb, a, b, x, mid, client_id))
                flags[0][a] = 1; ids[0][a] = mid; flags[j + 1][b] |= 1; ids[j + 1][b] = mid
        off.append(len(P))
    return dict(pair_offset=np.asarray(off, np.int32), pairs=np.asarray(P, np.int32).reshape(-1, 2), x3d=np.asarray(X, f32).reshape(-1, 3), status=np.asarray(S, np.uint8),
                source=np.asarray(R, np.uint8), n_new=len(recs), records=recs, flags=flags, mp_ids=ids)


# ---- the seeded scene: a current keyframe and neighbours ~1 m apart looking at points 5-40 m away ----
def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])


CENTRES = [(0.0, 0.0, 0.0), (0.45, 0.02, 0.9), (-0.5, 0.03, 0.85), (0.7, -0.04, -0.7)]        # camera centres: keyframe 0 = current


def compute_F12(k1, k2):
    """LocalMapping::ComputeF12 (C/src/LocalMapping.cc:587-606) in double, rounded to float, and the epipole of KF1's centre in KF2 (ORBmatcher.cc:803-808)"""
    T1, T2 = np.asarray(k1["Tcw"], f64).reshape(4, 4), np.asarray(k2["Tcw"], f64).reshape(4, 4)
    R12 = T1[:3, :3] @ T2[:3, :3].T; t12 = -R12 @ T2[:3, 3] + T1[:3, 3]
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    K1 = np.array([[k1["fx"], 0, k1["cx"]], [0, k1["fy"], k1["cy"]], [0, 0, 1]], f64); K2 = np.array([[k2["fx"], 0, k2["cx"]], [0, k2["fy"], k2["cy"]], [0, 0, 1]], f64)
    F = np.linalg.inv(K1).T @ tx @ R12 @ np.linalg.inv(K2)
    C2 = T2[:3, :3] @ (-T1[:3, :3].T @ T1[:3, 3]) + T2[:3, 3]
    return F.astype(f32), (f32(k2["fx"] * C2[0] / C2[2] + k2["cx"]), f32(k2["fy"] * C2[1] / C2[2] + k2["cy"]))


def scene(seed, n_points, n_nb=1, noise=0.5, stereo_frac=0.6, n_nodes=16, mismatch_frac=0.0, centres=None):
    """cur, nbs: keyframe dicts (id, Tcw, intrinsics, mb, scale, kp, u_right, depth, desc, has_mp, fv) observing the same n_points world points, every keyframe in its own
    feature order; truth[j][idx1] = feature of neighbour j that shows the same point; W = the world points.  mismatch_frac: that share of neighbour 0's features sits in octave 7 (the pair fails the
    scale test there and is met again at neighbour 1)."""
    rng = np.random.default_rng(seed)
    c = KITTI; mb = f32(f32(c["bf"]) / f32(c["fx"]))
    scale = np.ones(8, f32)
    for l in range(1, 8):
        scale[l] = scale[l - 1] * f32(1.2)
    W = np.stack([rng.uniform(-6, 6, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(5, 40, n_points)], 1)
    W[:, 0] *= W[:, 2] / 40 + 0.3
    base = rng.integers(0, 256, (n_points, 32), dtype=np.uint8); node = rng.integers(0, n_nodes, n_points)
    octave = rng.integers(0, 4, n_points)
    kfs = []
    for q in range(n_nb + 1):
        R = _rot(*(rng.normal(0, 0.01, 3) if q else np.zeros(3)))
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = -R @ np.asarray((centres or CENTRES)[q])
        T = T.astype(f32)
        perm = rng.permutation(n_points)
        Pc = (T[:3, :3].astype(f64) @ W[perm].T).T + T[:3, 3].astype(f64)
        kp = np.zeros(n_points, KP_DTYPE)
        kp["x"] = c["fx"] * Pc[:, 0] / Pc[:, 2] + c["cx"] + rng.normal(0, noise, n_points); kp["y"] = c["fy"] * Pc[:, 1] / Pc[:, 2] + c["cy"] + rng.normal(0, noise, n_points)
        kp["octave"] = octave[perm]; kp["size"] = 31; kp["angle"] = rng.uniform(0, 360, n_points)
        if q == 1 and mismatch_frac > 0:
            kp["octave"][rng.random(n_points) < mismatch_frac] = 7
        st = rng.random(n_points) < stereo_frac
        ur = np.where(st, kp["x"] - c["bf"] / Pc[:, 2] + rng.normal(0, noise, n_points), -1).astype(f32)
        depth = np.where(st, f32(c["bf"]) / np.maximum(kp["x"] - ur, f32(1e-3)), f32(-1)).astype(f32)
        bits = np.unpackbits(base[perm], axis=1) ^ (rng.random((n_points, 256)) < 0.03).astype(np.uint8)
        order = np.argsort(node[perm], kind="stable"); ids = np.unique(node[perm])
        off = np.concatenate([[0], np.cumsum([np.sum(node[perm] == i) for i in ids])]).astype(np.int32)
        kfs.append(dict(id=100 + 10 * q, Tcw=T, fx=f32(c["fx"]), fy=f32(c["fy"]), cx=f32(c["cx"]), cy=f32(c["cy"]), bf=f32(c["bf"]), mb=mb, scale=scale, kp=kp, u_right=ur, depth=depth,
                        desc=np.packbits(bits, axis=1), has_mp=np.zeros(n_points, np.uint8), fv=((ids * 7 + 3).astype(np.uint32), off, order.astype(np.uint32)), perm=perm))
    inv = [np.argsort(k["perm"]) for k in kfs]
    truth = [inv[j + 1][kfs[0]["perm"]] for j in range(n_nb)]
    return kfs[0], kfs[1:], truth, W


def exact_pair(n=40, seed=1):
    """two keyframes 1 m apart side by side (so that every point at 5-40 m has more than the 1.15 degrees of parallax a monocular pair needs), exact projections
    (float-rounded), all monocular; returns (kf1, kf2, pairs, world points per pair)"""
    cur, nbs, truth, W = scene(seed, n, 1, noise=0.0, stereo_frac=0.0, centres=[(0.0, 0.0, 0.0), (1.0, 0.02, 0.05)])
    return cur, nbs[0], np.stack([np.arange(n), truth[0]], 1).astype(np.int32), W[cur["perm"]]


def _project(k, P):
    T = np.asarray(k["Tcw"], f64).reshape(4, 4); Pc = T[:3, :3] @ np.asarray(P, f64) + T[:3, 3]
    return float(k["fx"]) * Pc[0] / Pc[2] + float(k["cx"]), float(k["fy"]) * Pc[1] / Pc[2] + float(k["cy"]), Pc[2]


def status_cases(cur=None, nb=None):
    """One pair per status / source from exact projections into two keyframes (default: the scene's first two, 1 m apart, mostly along the optical axis, so that a close
    stereo point near the axis has less ray parallax than stereo parallax): returns (kf1, kf2, pairs, names); the keyframes hold one feature per case."""
    if cur is None:
        cur, nbs, _, _ = scene(2, 4, 1, noise=0.0, stereo_frac=0.0); nb = nbs[0]
    cases = []        # (name, world point, stereo1, stereo2, octave1, octave2, tweak)
    cases.append(("ok_svd", (1.0, 0.3, 12.0), 0, 0, 1, 1, None))
    cases.append(("no_parallax", (40.0, 5.0, 3000.0), 0, 0, 0, 0, None))
    cases.append(("source1", (0.2, 0.1, 6.0), 1, 0, 0, 0, None))
    cases.append(("source2", (0.2, 0.1, 6.0), 0, 1, 0, 0, None))
    cases.append(("both_stereo", (0.2, 0.1, 6.0), 1, 1, 0, 0, None))
    cases.append(("behind_1", (1.0, 0.3, 12.0), 0, 0, 0, 0, "swap"))
    cases.append(("behind_2", (0.3, 0.1, 0.5), 1, 0, 0, 0, None))             # a stereo point between the two cameras: in front of the first, behind the second
    cases.append(("reproj_1", (1.0, 0.3, 12.0), 0, 0, 0, 0, "off1"))
    cases.append(("reproj_2", (0.2, 0.1, 6.0), 1, 0, 0, 0, "off2"))
    cases.append(("scale", (1.0, 0.3, 12.0), 0, 0, 0, 7, None))
    n = len(cases)
    out = []
    for k in (cur, nb):
        k = dict(k); k["kp"] = np.zeros(n, KP_DTYPE); k["u_right"] = np.full(n, -1, f32); k["depth"] = np.full(n, -1, f32); out.append(k)
    for i, (name, P, s1, s2, o1, o2, tweak) in enumerate(cases):
        obs = [_project(out[0], P), _project(out[1], P)]
        if tweak == "swap":
            obs = [obs[1], obs[0]]
        for k, (u, v, z), s, o in ((out[0], obs[0], s1, o1), (out[1], obs[1], s2, o2)):
            k["kp"]["x"][i], k["kp"]["y"][i], k["kp"]["octave"][i] = u, v, o
            if s:
                k["u_right"][i] = u - float(k["bf"]) / z; k["depth"][i] = z
        if tweak == "off1":
            out[0]["kp"]["y"][i] += 10
        if tweak == "off2":
            out[1]["kp"]["y"][i] += 10
    return out[0], out[1], np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32), [c[0] for c in cases]


def mixed_pairs(seed, n_pairs):
    """The scene with 0.5-px noise and about 60 % stereo features, the status cases appended to both keyframes, the pairs shuffled: (kf1, kf2, pairs [n_pairs, 2])"""
    cur, nbs, truth, _ = scene(seed, n_pairs - 10, 1); nb = nbs[0]
    c1, c2, cp, names = status_cases(cur, nb)
    n0 = len(cur["kp"])
    pairs = np.concatenate([np.stack([np.arange(n0), truth[0]], 1), cp + n0]).astype(np.int32)
    for k, c in ((cur, c1), (nb, c2)):
        for f in ("kp", "u_right", "depth"):
            k[f] = np.concatenate([k[f], c[f]])
    return cur, nb, pairs[np.random.default_rng(seed).permutation(len(pairs))]

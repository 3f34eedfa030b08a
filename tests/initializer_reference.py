"""numpy restatement of the monocular Initializer (C/src/Initializer.cc): Initialize (:44-121) with the set generation (:77-97), FindHomography, FindFundamental,
Normalize, ComputeH21, ComputeF21, CheckHomography, CheckFundamental, ReconstructF, ReconstructH, DecomposeE, CheckRT and Triangulate.  The source's float
expressions are non-fused IEEE operations in the types C++ gives them; sums over keys and over matches are float sums in ascending index order.  The readings of the
OpenCV calls the reference cannot pin are those of DESIGN.md section 2 and this file is their definition: cv::SVDecomp / cv::SVD::compute = the one-sided Jacobi
`hestenes` of pnpsolver_reference in float64 on the matrix taken into double, results rounded to float once; Mat::inv of a 3 x 3 = adjugate times 1 / det in double;
a float product = double accumulation in ascending k, one rounding.  The functions are vectorised over hypotheses or matches (leading axis)."""
import math
import numpy as np
from pnpsolver_reference import hestenes, _quiet, SV_DROP, RAND_RANGE
from ransac_reference import draw_set

f32, f64 = np.float32, np.float64
OK, NO_MODEL, H_DEGENERATE, AMBIGUOUS, FEW_POINTS, LOW_PARALLAX = range(6)
STATUS_NAMES = ("OK", "NO_MODEL", "H_DEGENERATE", "AMBIGUOUS", "FEW_POINTS", "LOW_PARALLAX")
RESULT_DTYPE = np.dtype([("status", "<i4"), ("model", "<i4"), ("n_matches", "<i4"), ("score_h", "<f4"), ("score_f", "<f4"), ("rh", "<f4"), ("best_it_h", "<i4"),
                         ("best_it_f", "<i4"), ("H21", "<f4", 9), ("F21", "<f4", 9), ("n_inliers", "<i4"), ("n_good", "<i4", 8), ("cos_parallax", "<f4", 8),
                         ("parallax", "<f4", 8), ("best_hypothesis", "<i4"), ("second_best_good", "<i4"), ("R21", "<f4", 9), ("t21", "<f4", 3),
                         ("n_triangulated", "<i4")])                                                                  # CorbInitResult


# ---- the draws (:82-97) ----
def draw_sets(rand_values, N):
    """mvSets: rand_values [its, 8] results of rand(), each consumed as RandomInt(0, size - 1) with the swap-with-back removal"""
    return np.array([draw_set(r, 8, N) for r in np.asarray(rand_values).reshape(-1, 8)], np.int64).reshape(-1, 8)


# ---- Normalize (:749-795) ----
def normalize(xy):
    """-> (meanX, meanY, sX, sY) as float32; sums in float in ascending index order"""
    xy = np.asarray(xy, f32); n = len(xy)
    with _quiet():
        mean = np.add.accumulate(xy, axis=0, dtype=f32)[-1] / f32(n)
        dev = np.add.accumulate(np.abs(xy - mean), axis=0, dtype=f32)[-1] / f32(n)
        s = (f64(1.0) / dev.astype(f64)).astype(f32)
    return np.array([mean[0], mean[1], s[0], s[1]], f32)


def T_of(nrm):
    T = np.zeros((3, 3), f32)
    T[0, 0] = nrm[2]; T[1, 1] = nrm[3]; T[0, 2] = -nrm[0] * nrm[2]; T[1, 2] = -nrm[1] * nrm[3]; T[2, 2] = 1
    return T


# ---- small matrices (leading axes are batch) ----
def mul3(A, B, alpha=None):
    """float product: entries accumulated in double in ascending k from 0.0 (times alpha in double), rounded once"""
    A = np.asarray(A, f32).astype(f64); B = np.asarray(B, f32).astype(f64)
    with _quiet():
        s = np.zeros(np.broadcast_shapes(A.shape[:-2], B.shape[:-2]) + (A.shape[-2], B.shape[-1]), f64)
        for k in range(A.shape[-1]):
            s = s + A[..., :, k, None] * B[..., None, k, :]
        if alpha is not None:
            s = np.asarray(alpha, f32).astype(f64)[..., None, None] * s
        return s.astype(f32)


def det3(M):
    M = np.asarray(M, f32).astype(f64)
    a, b, c, d, e, f, g, h, i = [M[..., k // 3, k % 3] for k in range(9)]
    with _quiet():
        return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)


def inv3(M):
    Md = np.asarray(M, f32).astype(f64)
    a, b, c, d, e, f, g, h, i = [Md[..., k // 3, k % 3] for k in range(9)]
    with _quiet():
        det = det3(M)
        r = f64(1.0) / det
        adj = [(e * i - f * h), (c * h - b * i), (b * f - c * e), (f * g - d * i), (a * i - c * g), (c * d - a * f), (d * h - e * g), (b * g - a * h), (a * e - b * d)]
        out = np.stack([(x * r).astype(f32) for x in adj], axis=-1).reshape(Md.shape)
    return np.where((det == 0)[..., None, None], f32(0), out)


def svd_null(A):
    """vt.row(last) of cv::SVDecomp of the float matrices A [H, m, n]: V's column of the smallest singular value (the last of the descending order), as float"""
    A = np.asarray(A, f32)
    UW, V, w, order = hestenes(A.astype(f64))
    return V[np.arange(len(A)), :, order[:, -1]].astype(f32)


def svd3(M):
    """cv::SVD::compute of float 3 x 3 matrices M [H, 3, 3] -> U [H, 3, 3], w [H, 3], Vt [H, 3, 3] as float, descending.  u_k = a_k / w_k; a smallest singular value not
    above 2^-51 sum_j w_j leaves the cross product of the other two columns, two such leave NaN"""
    M = np.asarray(M, f32); H = len(M); ar = np.arange(H)
    UW, V, w, order = hestenes(M.astype(f64))
    with _quiet():
        thr = SV_DROP * ((w[:, 0] + w[:, 1]) + w[:, 2])
        o0, o1, o2 = order[:, 0], order[:, 1], order[:, 2]
        w0, w1, w2 = w[ar, o0], w[ar, o1], w[ar, o2]
        u0 = UW[ar, :, o0] / w0[:, None]; u1 = UW[ar, :, o1] / w1[:, None]; u2 = UW[ar, :, o2] / w2[:, None]
        cross = np.stack([u0[:, 1] * u1[:, 2] - u0[:, 2] * u1[:, 1], u0[:, 2] * u1[:, 0] - u0[:, 0] * u1[:, 2], u0[:, 0] * u1[:, 1] - u0[:, 1] * u1[:, 0]], axis=1)
        u2 = np.where((w2 > thr)[:, None], u2, cross)
        U = np.stack([u0, u1, u2], axis=2)
        U = np.where((w1 > thr)[:, None, None], U, np.nan)
        Vt = np.stack([V[ar, :, o0], V[ar, :, o1], V[ar, :, o2]], axis=1)
    return U.astype(f32), np.stack([w0, w1, w2], axis=1).astype(f32), Vt.astype(f32)


# ---- ComputeH21 (:226-266), ComputeF21 (:268-303) on normalised points [H, 8, 2] ----
def compute_H21(p1, p2):
    p1 = np.asarray(p1, f32); p2 = np.asarray(p2, f32); H = len(p1)
    u1, v1, u2, v2 = p1[:, :, 0], p1[:, :, 1], p2[:, :, 0], p2[:, :, 1]
    A = np.zeros((H, 16, 9), f32); z = np.zeros_like(u1); o = np.ones_like(u1)
    A[:, 0::2] = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], axis=2)
    A[:, 1::2] = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], axis=2)
    return svd_null(A).reshape(H, 3, 3)


def compute_F21(p1, p2):
    p1 = np.asarray(p1, f32); p2 = np.asarray(p2, f32); H = len(p1)
    u1, v1, u2, v2 = p1[:, :, 0], p1[:, :, 1], p2[:, :, 0], p2[:, :, 1]
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], axis=2)
    Fpre = svd_null(A).reshape(H, 3, 3)
    U, w, Vt = svd3(Fpre)
    D = np.zeros((H, 3, 3), f32); D[:, 0, 0] = w[:, 0]; D[:, 1, 1] = w[:, 1]
    return mul3(mul3(U, D), Vt)


# ---- CheckHomography (:305-388), CheckFundamental (:390-468): M [H, 3, 3], m = (u1, v1, u2, v2) [N] each -> (score [H], inliers [H, N]) ----
def _ordered_score(t1, a1, t2, a2):
    H, N = t1.shape
    terms = np.empty((H, 2 * N + 1), f32); terms[:, 0] = 0
    terms[:, 1::2] = np.where(a1, t1, f32(0)); terms[:, 2::2] = np.where(a2, t2, f32(0))
    return np.add.accumulate(terms, axis=1, dtype=f32)[:, -1]


def _recip(x):
    return (f64(1.0) / x.astype(f64)).astype(f32)


def check_homography(H21, H12, m, sigma):
    u1, v1, u2, v2 = [np.asarray(x, f32)[None, :] for x in m]
    h = [np.asarray(H21, f32)[:, k // 3, k % 3, None] for k in range(9)]; hi = [np.asarray(H12, f32)[:, k // 3, k % 3, None] for k in range(9)]
    th = f32(5.991)
    with _quiet():
        inv_s2 = _recip(np.asarray(f32(sigma) * f32(sigma)))
        w = _recip(hi[6] * u2 + hi[7] * v2 + hi[8])
        a = (hi[0] * u2 + hi[1] * v2 + hi[2]) * w; b = (hi[3] * u2 + hi[4] * v2 + hi[5]) * w
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_s2
        w = _recip(h[6] * u1 + h[7] * v1 + h[8])
        a = (h[0] * u1 + h[1] * v1 + h[2]) * w; b = (h[3] * u1 + h[4] * v1 + h[5]) * w
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv_s2
        a1 = ~(chi1 > th); a2 = ~(chi2 > th)
        return _ordered_score(th - chi1, a1, th - chi2, a2), a1 & a2


def check_fundamental(F21, m, sigma):
    u1, v1, u2, v2 = [np.asarray(x, f32)[None, :] for x in m]
    f = [np.asarray(F21, f32)[:, k // 3, k % 3, None] for k in range(9)]
    th, th_score = f32(3.841), f32(5.991)
    with _quiet():
        inv_s2 = _recip(np.asarray(f32(sigma) * f32(sigma)))
        a2 = f[0] * u1 + f[1] * v1 + f[2]; b2 = f[3] * u1 + f[4] * v1 + f[5]; c2 = f[6] * u1 + f[7] * v1 + f[8]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2
        a1 = f[0] * u2 + f[3] * v2 + f[6]; b1 = f[1] * u2 + f[4] * v2 + f[7]; c1 = f[2] * u2 + f[5] * v2 + f[8]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2
        k1 = ~(chi1 > th); k2 = ~(chi2 > th)
        return _ordered_score(th_score - chi1, k1, th_score - chi2, k2), k1 & k2


def first_best(scores):
    """the iteration the loop of :148-171 keeps: the first maximum of the positive scores (strict >, NaN is never greater); -1 if none"""
    best, bi = f32(0), -1
    for i, s in enumerate(np.asarray(scores, f32)):
        if s > best:
            best, bi = s, i
    return best, bi


# ---- Triangulate (:734-747) for matches [n]: A rows in float, the null vector, x / w ----
def triangulate(m, P1, P2):
    u1, v1, u2, v2 = [np.asarray(x, f32)[:, None] for x in m]
    with _quiet():
        A = np.stack([u1 * P1[2] - P1[0], v1 * P1[2] - P1[1], u2 * P2[2] - P2[0], v2 * P2[2] - P2[1]], axis=1).astype(f32)
        v = svd_null(A) if len(A) else np.zeros((0, 4), f32)
        return (v[:, :3] / v[:, 3:4]).astype(f32)


def _norm3(v):
    v = v.astype(f64)
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def cos_before(a, ia, b, ib):
    """the rank order of vCosParallax: value, then position; NaN last"""
    na, nb = a != a, b != b
    if na or nb:
        return ia < ib if na == nb else nb
    return a < b or (a == b and ia < ib)


def order_statistic(cos):
    """vCosParallax[min(50, size - 1)] after the sort (:898-900), by rank"""
    want = min(50, len(cos) - 1)
    for i, ci in enumerate(cos):
        if sum(1 for j, cj in enumerate(cos) if cos_before(cj, j, ci, i)) == want:
            return f32(ci)
    raise AssertionError


def parallax_of(c):
    """:901 with acos in double and one rounding"""
    c = float(f32(c))
    return f32(math.acos(c) * 180 / 3.1415926535897932384626433832795) if -1.0 <= c <= 1.0 else f32(np.nan)


def check_rt(R, t, m, i1, inl, K4, n1, sigma):
    """CheckRT (:798-907) -> (nGood, cosine of the order statistic (1 when nGood == 0: parallax 0), vP3D [n1, 3], vbGood [n1], vCosParallax)"""
    fx, fy, cx, cy = [f32(x) for x in K4]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)
    R = np.asarray(R, f32).reshape(3, 3); t = np.asarray(t, f32).reshape(3)
    sigma = f32(sigma); th2 = f32(f64(4.0) * f64(sigma * sigma))
    P1 = np.concatenate([K, np.zeros((3, 1), f32)], axis=1)
    P2 = mul3(K, np.concatenate([R, t[:, None]], axis=1))
    O2 = mul3(-R.T, t[:, None])[:, 0]
    sel = np.nonzero(inl)[0]
    mm = [np.asarray(x, f32)[sel] for x in m]; u1, v1, u2, v2 = mm
    p3d = np.zeros((n1, 3), f32); good = np.zeros(n1, bool)
    with _quiet():
        X = triangulate(mm, P1, P2)
        fin = np.isfinite(X).all(axis=1)
        n2 = X - O2
        dist1 = _norm3(X).astype(f32); dist2 = _norm3(n2).astype(f32)
        Xd, nd = X.astype(f64), n2.astype(f64)
        dot = (Xd[:, 0] * nd[:, 0] + Xd[:, 1] * nd[:, 1]) + Xd[:, 2] * nd[:, 2]
        cosp = (dot / (dist1 * dist2).astype(f64)).astype(f32)
        low = cosp.astype(f64) < 0.99998
        X2 = np.zeros_like(X); Rd = R.astype(f64)                                # p3dC2 = R * p3dC1 + t: one product with the sum taken in double
        for a in range(3):
            s = np.zeros(len(X), f64)
            for k in range(3):
                s = s + Rd[a, k] * Xd[:, k]
            X2[:, a] = (s + f64(t[a])).astype(f32)
        keep = fin & ~((X[:, 2] <= 0) & low) & ~((X2[:, 2] <= 0) & low)
        invZ1 = _recip(X[:, 2])
        im1x = fx * X[:, 0] * invZ1 + cx; im1y = fy * X[:, 1] * invZ1 + cy
        keep &= ~(((im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1)) > th2)
        invZ2 = _recip(X2[:, 2])
        im2x = fx * X2[:, 0] * invZ2 + cx; im2y = fy * X2[:, 1] * invZ2 + cy
        keep &= ~(((im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2)) > th2)
    k1 = np.asarray(i1)[sel][keep]
    p3d[k1] = X[keep]; good[k1] = low[keep]
    cos = [f32(c) for c in cosp[keep]]
    return len(cos), (order_statistic(cos) if cos else f32(1)), p3d, good, cos


# ---- the motion hypotheses ----
def decompose_E(E):
    """DecomposeE (:909-929) and the order of :494-497 -> [(R, t)] * 4"""
    U, w, Vt = svd3(np.asarray(E, f32)[None]); U, Vt = U[0], Vt[0]
    with _quiet():
        t = U[:, 2]
        t = (t.astype(f64) / _norm3(t[None])[0]).astype(f32)
        W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f32)
        R1 = mul3(mul3(U, W), Vt); R2 = mul3(mul3(U, W.T.copy()), Vt)
        if det3(R1) < 0:
            R1 = -R1
        if det3(R2) < 0:
            R2 = -R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def faugeras(A):
    """the 8 hypotheses of :584-686 from A = invK * H21 * K; None where d1 / d2 or d2 / d3 is below 1.00001 (:597)"""
    U, w, Vt = svd3(np.asarray(A, f32)[None]); U, w, Vt = U[0], w[0], Vt[0]
    with _quiet():
        s = f32(det3(U) * det3(Vt))
        d1, d2, d3 = w
        if f64(d1 / d2) < 1.00001 or f64(d2 / d3) < 1.00001:
            return None
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)); aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1 = [aux1, aux1, -aux1, -aux1]; x3 = [aux3, -aux3, aux3, -aux3]
        aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2); ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        st = [aux_st, -aux_st, -aux_st, aux_st]
        aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2); cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        out = []
        for hy in range(8):
            i = hy & 3
            Rp = np.eye(3, dtype=f32)
            if hy < 4:
                Rp[0, 0] = ct; Rp[0, 2] = -st[i]; Rp[2, 0] = st[i]; Rp[2, 2] = ct
                tp = np.array([x1[i], 0, -x3[i]], f32) * f32(d1 - d3)
            else:
                Rp[0, 0] = cp; Rp[0, 2] = sp[i]; Rp[1, 1] = -1; Rp[2, 0] = sp[i]; Rp[2, 2] = -cp
                tp = np.array([x1[i], 0, x3[i]], f32) * f32(d1 + d3)
            R = mul3(mul3(U, Rp, alpha=s), Vt)
            t = mul3(U, tp[:, None])[:, 0]
            t = (t.astype(f64) / _norm3(t[None])[0]).astype(f32)
            out.append((R, t))
    return out


def decide(model, n_good, cosines, n_inliers, min_parallax, min_triangulated):
    """:499-569 (model 1) or :689-731 (model 0) -> (status, best_hypothesis, second_best_good).  Several failing tests are reported in the source's order: F: few
    points, ambiguous, parallax (the order of :517-525); H: parallax, ambiguous, few points"""
    best_good = second = 0; best = -1
    for i, g in enumerate(n_good):
        if g > best_good:
            second, best_good, best = best_good, g, i
        elif g > second:
            second = g
    mp = f32(min_parallax)
    if model == 1:
        best = max(best, 0)
        n_min = max(int(0.9 * n_inliers), min_triangulated)
        nsimilar = sum(1 for g in n_good if g > 0.7 * best_good)
        if best_good < n_min:
            return FEW_POINTS, best, second
        if nsimilar > 1:
            return AMBIGUOUS, best, second
        with _quiet():
            return (OK if parallax_of(cosines[best]) > mp else LOW_PARALLAX), best, second
    with _quiet():
        par = (f32(-1) >= mp) if best < 0 else (parallax_of(cosines[best]) >= mp)
    if not par:
        return LOW_PARALLAX, best, second
    if not second < 0.75 * best_good:
        return AMBIGUOUS, best, second
    if not (best_good > min_triangulated and best_good > 0.9 * n_inliers):
        return FEW_POINTS, best, second
    return OK, best, second


def reconstruct(model, M, inl, m, i1, K4, n1, sigma=1.0, min_parallax=1.0, min_triangulated=50):
    """ReconstructF (model 1, :470-570) or ReconstructH (model 0, :572-732) -> dict(status, n_good, cos_parallax, best_hypothesis, second_best_good, R21, t21, p3d,
    triangulated)"""
    fx, fy, cx, cy = [f32(x) for x in K4]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)
    out = dict(status=OK, n_good=np.zeros(8, np.int32), cos_parallax=np.zeros(8, f32), best_hypothesis=-1, second_best_good=0, R21=np.zeros(9, f32), t21=np.zeros(3, f32),
               p3d=np.zeros((n1, 3), f32), triangulated=np.zeros(n1, bool), n_inliers=int(np.sum(inl)))
    M = np.asarray(M, f32).reshape(3, 3)
    hyps = decompose_E(mul3(mul3(K.T.copy(), M), K)) if model == 1 else faugeras(mul3(mul3(inv3(K), M), K))
    if hyps is None:
        out["status"] = H_DEGENERATE
        return out
    cand = []
    for hy, (R, t) in enumerate(hyps):
        g, c, p3d, good, _ = check_rt(R, t, m, i1, inl, K4, n1, sigma)
        out["n_good"][hy] = g; out["cos_parallax"][hy] = c; cand.append((p3d, good))
    st, best, second = decide(model, [int(g) for g in out["n_good"][:len(hyps)]], out["cos_parallax"], out["n_inliers"], min_parallax, min_triangulated)
    out.update(status=st, best_hypothesis=best, second_best_good=second)
    if st == OK:
        out.update(R21=hyps[best][0].reshape(9).copy(), t21=hyps[best][1].copy(), p3d=cand[best][0], triangulated=cand[best][1])
    return out


# ---- Initialize (:44-121) ----
def pack_matches(keys1, keys2, matches12):
    keys1 = np.asarray(keys1, f32).reshape(-1, 2); keys2 = np.asarray(keys2, f32).reshape(-1, 2); matches12 = np.asarray(matches12, np.int64)
    i1 = np.nonzero(matches12 >= 0)[0]; i2 = matches12[i1]
    return (keys1[i1, 0], keys1[i1, 1], keys2[i2, 0], keys2[i2, 1]), i1, i2


def hypotheses(keys1, keys2, matches12, rand_values, sigma=1.0):
    """FindHomography and FindFundamental without their running best: -> (scores [its, 2], H21i [its, 3, 3], F21i [its, 3, 3], inliers H [its, N], inliers F)"""
    keys1 = np.asarray(keys1, f32).reshape(-1, 2); keys2 = np.asarray(keys2, f32).reshape(-1, 2)
    m, i1, i2 = pack_matches(keys1, keys2, matches12); N = len(i1)
    sets = draw_sets(rand_values, N)
    n1, n2 = normalize(keys1), normalize(keys2)
    T1, T2 = T_of(n1), T_of(n2)
    with _quiet():
        pn1 = (keys1[i1] - n1[:2]) * n1[2:]; pn2 = (keys2[i2] - n2[:2]) * n2[2:]
    p1, p2 = pn1[sets], pn2[sets]
    H21 = mul3(mul3(inv3(T2), compute_H21(p1, p2)), T1)
    F21 = mul3(mul3(T2.T.copy(), compute_F21(p1, p2)), T1)
    sh, ih = check_homography(H21, inv3(H21), m, sigma)
    sf, i_f = check_fundamental(F21, m, sigma)
    return np.stack([sh, sf], axis=1), H21, F21, ih, i_f


def initialize(keys1, keys2, matches12, K4, rand_values, sigma=1.0, max_iterations=200, min_parallax=1.0, min_triangulated=50, negate=False):
    """Initialize -> dict of every field of CorbInitResult plus p3d [n1, 3], triangulated [n1], inliers_h, inliers_f [N], scores [its, 2].  negate: hand -H or -F to
    the reconstruction (the sign of a null vector is not part of any reading)"""
    keys1 = np.asarray(keys1, f32).reshape(-1, 2); n1 = len(keys1)
    rv = np.asarray(rand_values).reshape(max_iterations, 8)
    scores, H21, F21, ih, i_f = hypotheses(keys1, keys2, matches12, rv, sigma)
    m, i1, i2 = pack_matches(keys1, keys2, matches12); N = len(i1)
    sh, bh = first_best(scores[:, 0]); sf, bf = first_best(scores[:, 1])
    with _quiet():
        rh = f32(sh) / (f32(sh) + f32(sf))
    model = 0 if f64(rh) > 0.40 else 1
    out = dict(status=OK, model=model, n_matches=N, score_h=f32(sh), score_f=f32(sf), rh=rh, best_it_h=bh, best_it_f=bf,
               H21=(H21[bh].reshape(9) if bh >= 0 else np.zeros(9, f32)), F21=(F21[bf].reshape(9) if bf >= 0 else np.zeros(9, f32)),
               inliers_h=(ih[bh] if bh >= 0 else np.zeros(N, bool)), inliers_f=(i_f[bf] if bf >= 0 else np.zeros(N, bool)), scores=scores,
               n_inliers=0, n_good=np.zeros(8, np.int32), cos_parallax=np.zeros(8, f32), best_hypothesis=-1, second_best_good=0, R21=np.zeros(9, f32),
               t21=np.zeros(3, f32), p3d=np.zeros((n1, 3), f32), triangulated=np.zeros(n1, bool))
    if rh != rh or (bh if model == 0 else bf) < 0:
        out["status"] = NO_MODEL
    else:
        M = out["H21"] if model == 0 else out["F21"]
        out.update(reconstruct(model, -M if negate else M, out["inliers_h"] if model == 0 else out["inliers_f"], m, i1, K4, n1, sigma, min_parallax, min_triangulated))
    out["parallax"] = np.array([parallax_of(c) if (out["status"] not in (NO_MODEL, H_DEGENERATE) and k < (4 if model else 8)) else f32(0)
                                for k, c in enumerate(out["cos_parallax"])], f32)
    out["n_triangulated"] = int(np.sum(out["triangulated"]))
    return out


def result_record(r):
    """the CorbInitResult of a result of initialize()"""
    rec = np.zeros((), RESULT_DTYPE)
    for k in RESULT_DTYPE.names:
        rec[k] = r[k]
    return rec


def draws(seed, n_problems, max_iterations):
    return np.random.default_rng(seed).integers(0, RAND_RANGE, size=(n_problems, max_iterations, 8), dtype=np.int64).astype(np.int32)

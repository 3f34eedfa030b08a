"""numpy restatement of PnPsolver (C/src/PnPsolver.cc): the constructor's filter (:67-110), SetRansacParameters (:166-202), the draws (:233-246 with
DUtils::Random::RandomInt), compute_pose (:420-570, :595-995), CheckInliers (:353-384), Refine (:305-350) and the rule that turns per-hypothesis inlier counts into
iterate()'s returns (:210-303).  Double arithmetic is unfused and every sum is written out in the order of the source; the functions are vectorised over hypotheses
(leading axis H) with masked updates through np.where.  The readings of the OpenCV calls the reference cannot pin are those of DESIGN.md section 2 and this file is
their definition: cvSVD of a symmetric matrix = jacobi_eig (cyclic Jacobi, FP64), cvInvert / cvSolve / cvSVD(ABt) = hestenes (one-sided Jacobi, FP64) with the
pseudo-inverse's drop rule.  NaN payloads and signs are not part of any reading."""
import math
import numpy as np
from ransac_reference import draw_set, draw_set_literal          # the draws (:233-246): the shared rule and its literal emulation

f32, f64 = np.float32, np.float64
NO_MAP_POINT = 0xFFFFFFFFFFFFFFFF
RAND_RANGE = 2 ** 31                          # RAND_MAX + 1
TWO_M60 = f64(2.0 ** -60)
SV_DROP = f64(2.0 ** -51)                     # 2 * DBL_EPSILON
BRANCHES = dict(sv_drop=0, cross=0, nan_R=0, qr_singular=0)      # how often the special branches were taken (test_pnpsolver_reference reads them)


def _quiet():
    return np.errstate(all="ignore")


# ---- SetRansacParameters (:166-202) ----
def ransac_parameters(N, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991):
    """-> (mRansacMaxIts, mRansacMinInliers); mRansacMaxIts = 0: iterate() sets bNoMore at once (N < mRansacMinInliers, :218-222)"""
    eps = f32(epsilon)
    m = int(f32(N) * eps)                                             # int nMinInliers = N * mRansacEpsilon: a float product, truncated
    m = max(m, int(min_inliers), int(min_set))
    if N < m or N <= 0:
        return 0, m
    if eps < f32(m) / f32(N):
        eps = f32(m) / f32(N)
    if m == N:
        nit = 1
    else:
        x = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(eps), 3.0)))
        nit = max_iterations if not x < max_iterations else (1 if x < 1 else int(x))
    return max(1, min(nit, max_iterations)), m


def max_errors(sigma2, th2=5.991):
    """mvMaxError[i] = mvSigma2[i] * th2 (:199-201): a float product"""
    return (np.asarray(sigma2, f32) * f32(th2)).astype(f32)


# ---- the decompositions ----
def order_desc(key):
    """indices of key in descending order, the lower index first among equals: a selection with a strict comparison (NaN is never greater)"""
    key = [float(k) for k in key]; n = len(key); order = list(range(n))
    for i in range(n - 1):
        b = i
        for j in range(i + 1, n):
            if key[order[j]] > key[order[b]]:
                b = j
        order.insert(i, order.pop(b))
    return order


def _orders(keys):
    return np.array([order_desc(k) for k in keys], np.int64).reshape(len(keys), keys.shape[1])


def jacobi_eig(A):
    """cvSVD of symmetric matrices A [H, n, n] with CV_SVD_U_T: cyclic Jacobi in float64 from V = I.  A pair (p, q) is rotated iff |a_pq| > 2^-60 max|A_ij|; row-cyclic;
    sweeps until one rotates nothing, at most 30; NaN rotates nothing.  Returns (diagonal [H, n], V [H, n, n] with the eigenvectors in its columns)"""
    A = np.array(A, f64); H, n, _ = A.shape
    V = np.zeros((H, n, n), f64); V[:, np.arange(n), np.arange(n)] = 1.0
    with _quiet():
        scale = np.fmax.reduce(np.abs(A).reshape(H, -1), axis=1, initial=0.0)
        tiny = scale * TWO_M60
        for sweep in range(30):
            rotated = False
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = A[:, p, q].copy()
                    rot = np.abs(apq) > tiny
                    if not rot.any():
                        continue
                    rotated = True
                    app, aqq = A[:, p, p].copy(), A[:, q, q].copy()
                    theta = (aqq - app) / (f64(2.0) * apq)
                    t = np.where(theta >= 0, f64(1.0), f64(-1.0)) / (np.abs(theta) + np.sqrt(theta * theta + f64(1.0)))
                    c = f64(1.0) / np.sqrt(t * t + f64(1.0)); s = t * c
                    akp, akq = A[:, :, p].copy(), A[:, :, q].copy()
                    newp = c[:, None] * akp - s[:, None] * akq; newq = s[:, None] * akp + c[:, None] * akq
                    newp[:, p] = app - t * apq; newp[:, q] = 0.0
                    newq[:, q] = aqq + t * apq; newq[:, p] = 0.0
                    m = rot[:, None]
                    colp = np.where(m, newp, akp); colq = np.where(m, newq, akq)
                    A[:, :, p] = colp; A[:, p, :] = colp; A[:, :, q] = colq; A[:, q, :] = colq
                    vkp, vkq = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p] = np.where(m, c[:, None] * vkp - s[:, None] * vkq, vkp)
                    V[:, :, q] = np.where(m, s[:, None] * vkp + c[:, None] * vkq, vkq)
            if not rotated:
                break
    return A[:, np.arange(n), np.arange(n)].copy(), V


def hestenes(A):
    """one-sided Jacobi SVD of A [H, m, n]: columns p, q are rotated iff |a_p . a_q| > 1e-15 |a_p| |a_q|, at most 30 sweeps.  Returns (UW [H, m, n] the rotated columns,
    V [H, n, n], w [H, n] the column norms, order [H, n] descending w)"""
    A = np.array(A, f64); H, m, n = A.shape
    V = np.zeros((H, n, n), f64); V[:, np.arange(n), np.arange(n)] = 1.0
    with _quiet():
        for sweep in range(30):
            rotated = False
            for p in range(n - 1):
                for q in range(p + 1, n):
                    alpha = np.zeros(H, f64); beta = np.zeros(H, f64); gamma = np.zeros(H, f64)
                    for k in range(m):
                        ap, aq = A[:, k, p], A[:, k, q]
                        alpha = alpha + ap * ap; beta = beta + aq * aq; gamma = gamma + ap * aq
                    rot = np.abs(gamma) > f64(1e-15) * np.sqrt(alpha * beta)
                    if not rot.any():
                        continue
                    rotated = True
                    zeta = (beta - alpha) / (f64(2.0) * gamma)
                    t = np.where(zeta >= 0, f64(1.0), f64(-1.0)) / (np.abs(zeta) + np.sqrt(f64(1.0) + zeta * zeta))
                    c = f64(1.0) / np.sqrt(f64(1.0) + t * t); s = c * t
                    mk = rot[:, None]; c_, s_ = c[:, None], s[:, None]
                    up, uq = A[:, :, p].copy(), A[:, :, q].copy()
                    A[:, :, p] = np.where(mk, c_ * up - s_ * uq, up); A[:, :, q] = np.where(mk, s_ * up + c_ * uq, uq)
                    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p] = np.where(mk, c_ * vp - s_ * vq, vp); V[:, :, q] = np.where(mk, s_ * vp + c_ * vq, vq)
            if not rotated:
                break
        s2 = np.zeros((H, n), f64)
        for k in range(m):
            s2 = s2 + A[:, k, :] * A[:, k, :]
        w = np.sqrt(s2)
    return A, V, w, _orders(w)


def sv_threshold(w):
    s = np.zeros(len(w), f64)
    for j in range(w.shape[1]):
        s = s + w[:, j]
    return SV_DROP * s


def sv_solve(dec, b):
    """x = sum over w_k > 2 * 2^-52 * sum_j w_j (descending w) of v_k ((u_k . b) / w_k), u_k = a_k / w_k; every other term is dropped"""
    UW, V, w, order = dec; H, m, n = UW.shape; ar = np.arange(H)
    with _quiet():
        thr = sv_threshold(w)
        x = np.zeros((H, n), f64)
        for kk in range(n):
            k = order[:, kk]
            ak, vk, wk = UW[ar, :, k], V[ar, :, k], w[ar, k]
            keep = wk > thr
            BRANCHES["sv_drop"] += int((~keep).sum())
            dot = np.zeros(H, f64)
            for i in range(m):
                dot = dot + (ak[:, i] / wk) * b[:, i]
            coef = dot / wk
            x = np.where(keep[:, None], x + vk * coef[:, None], x)
    return x


# ---- compute_pose ----
def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _dist2(p1, p2):
    return (p1[:, 0] - p2[:, 0]) * (p1[:, 0] - p2[:, 0]) + (p1[:, 1] - p2[:, 1]) * (p1[:, 1] - p2[:, 1]) + (p1[:, 2] - p2[:, 2]) * (p1[:, 2] - p2[:, 2])


def _alphas(ci, c0, pi):
    """compute_barycentric_coordinates' row (:468-478); ci [H, 3, 3], c0 [H, 3], pi [H, 3] -> [H, 4]"""
    a = np.empty((len(pi), 4), f64)
    for j in range(3):
        a[:, 1 + j] = ci[:, j, 0] * (pi[:, 0] - c0[:, 0]) + ci[:, j, 1] * (pi[:, 1] - c0[:, 1]) + ci[:, j, 2] * (pi[:, 2] - c0[:, 2])
    a[:, 0] = f64(1.0) - a[:, 1] - a[:, 2] - a[:, 3]
    return a


def _pc(a, ccs):
    """compute_pcs' row (:517-518); ccs [H, 4, 3] -> [H, 3]"""
    return a[:, 0, None] * ccs[:, 0] + a[:, 1, None] * ccs[:, 1] + a[:, 2, None] * ccs[:, 2] + a[:, 3, None] * ccs[:, 3]


_MTM_A, _MTM_B = np.triu_indices(12)


def _L_6x10(v):
    """compute_L_6x10 (:805-845); v [H, 4, 12] = rows 11, 10, 9, 8 of ut"""
    H = len(v); L = np.empty((H, 6, 10), f64)
    two = f64(2.0)
    for r, (a, b) in enumerate([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]):
        dv = v[:, :, 3 * a: 3 * a + 3] - v[:, :, 3 * b: 3 * b + 3]
        d = lambda i, j: _dot3(dv[:, i], dv[:, j])
        L[:, r, 0] = d(0, 0); L[:, r, 1] = two * d(0, 1); L[:, r, 2] = d(1, 1); L[:, r, 3] = two * d(0, 2); L[:, r, 4] = two * d(1, 2)
        L[:, r, 5] = d(2, 2); L[:, r, 6] = two * d(0, 3); L[:, r, 7] = two * d(1, 3); L[:, r, 8] = two * d(2, 3); L[:, r, 9] = d(3, 3)
    return L


def _find_betas(which, L, rho):
    """find_betas_approx_1 / 2 / 3 (:712-803)"""
    cols = {1: [0, 1, 3, 6], 2: [0, 1, 2], 3: [0, 1, 2, 3, 4]}[which]
    b = sv_solve(hestenes(L[:, :, cols]), rho)
    H = len(L); betas = np.zeros((H, 4), f64)
    neg = b[:, 0] < 0
    if which == 1:
        b0 = np.where(neg, np.sqrt(-b[:, 0]), np.sqrt(b[:, 0]))
        betas[:, 0] = b0
        for k in (1, 2, 3):
            betas[:, k] = np.where(neg, -b[:, k] / b0, b[:, k] / b0)
        return betas
    b0 = np.where(neg, np.sqrt(-b[:, 0]), np.sqrt(b[:, 0]))
    betas[:, 1] = np.where(neg, np.where(b[:, 2] < 0, np.sqrt(-b[:, 2]), f64(0.0)), np.where(b[:, 2] > 0, np.sqrt(b[:, 2]), f64(0.0)))
    b0 = np.where(b[:, 1] < 0, -b0, b0)
    betas[:, 0] = b0
    if which == 3:
        betas[:, 2] = b[:, 3] / b0
    return betas


def qr_solve(A, b, X):
    """qr_solve (:905-995) on A [H, 6, 4], b [H, 6]; X [H, 4] is what it was where eta == 0 returns early.  The search for eta reads rows k .. nr - 2, as the source's
    pointer does"""
    A = A.copy(); b = b.copy(); H, nr, nc = A.shape
    alive = np.ones(H, bool); A1 = np.zeros((H, nc), f64); A2 = np.zeros((H, nc), f64)
    for k in range(nc):
        eta = np.abs(A[:, k, k])
        for i in range(k + 1, nr):
            elt = np.abs(A[:, i - 1, k]); eta = np.where(eta < elt, elt, eta)
        alive = alive & ~(eta == 0)
        inv_eta = f64(1.0) / eta; ssum = np.zeros(H, f64)
        for i in range(k, nr):
            A[:, i, k] = A[:, i, k] * inv_eta; ssum = ssum + A[:, i, k] * A[:, i, k]
        sigma = np.sqrt(ssum); sigma = np.where(A[:, k, k] < 0, -sigma, sigma)
        A[:, k, k] = A[:, k, k] + sigma
        A1[:, k] = sigma * A[:, k, k]; A2[:, k] = -eta * sigma
        for j in range(k + 1, nc):
            s2 = np.zeros(H, f64)
            for i in range(k, nr):
                s2 = s2 + A[:, i, k] * A[:, i, j]
            tau = s2 / A1[:, k]
            for i in range(k, nr):
                A[:, i, j] = A[:, i, j] - tau * A[:, i, k]
    for j in range(nc):
        tau = np.zeros(H, f64)
        for i in range(j, nr):
            tau = tau + A[:, i, j] * b[:, i]
        tau = tau / A1[:, j]
        for i in range(j, nr):
            b[:, i] = b[:, i] - tau * A[:, i, j]
    Xn = np.empty((H, nc), f64)
    Xn[:, nc - 1] = b[:, nc - 1] / A2[:, nc - 1]
    for i in range(nc - 2, -1, -1):
        ssum = np.zeros(H, f64)
        for j in range(i + 1, nc):
            ssum = ssum + A[:, i, j] * Xn[:, j]
        Xn[:, i] = (b[:, i] - ssum) / A2[:, i]
    BRANCHES["qr_singular"] += int((~alive).sum())
    return np.where(alive[:, None], Xn, X)


def _gauss_newton(L, rho, betas):
    """gauss_newton (:885-903) with compute_A_and_b_gauss_newton (:857-883); X starts as zeros"""
    betas = betas.copy(); H = len(L); X = np.zeros((H, 4), f64); two = f64(2.0)
    r = lambda k: L[:, :, k]                                           # [H, 6]
    for it in range(5):
        B = [betas[:, k, None] for k in range(4)]
        A = np.empty((H, 6, 4), f64)
        A[:, :, 0] = two * r(0) * B[0] + r(1) * B[1] + r(3) * B[2] + r(6) * B[3]
        A[:, :, 1] = r(1) * B[0] + two * r(2) * B[1] + r(4) * B[2] + r(7) * B[3]
        A[:, :, 2] = r(3) * B[0] + r(4) * B[1] + two * r(5) * B[2] + r(8) * B[3]
        A[:, :, 3] = r(6) * B[0] + r(7) * B[1] + r(8) * B[2] + two * r(9) * B[3]
        b = rho - (r(0) * B[0] * B[0] + r(1) * B[0] * B[1] + r(2) * B[1] * B[1] + r(3) * B[0] * B[2] + r(4) * B[1] * B[2] + r(5) * B[2] * B[2] +
                   r(6) * B[0] * B[3] + r(7) * B[1] * B[3] + r(8) * B[2] * B[3] + r(9) * B[3] * B[3])
        X = qr_solve(A, b, X)
        betas = betas + X
    return betas


def estimate_R_and_t(pc0, pw0, abt):
    """estimate_R_and_t (:635-672) from the sums: R = U V^T of the Hestenes SVD of ABt.  A dropped smallest singular value's left vector is the cross product of the other
    two; two dropped ones leave NaN"""
    H = len(abt); ar = np.arange(H)
    UW, V, w, order = hestenes(abt)
    thr = sv_threshold(w)
    o0, o1, o2 = order[:, 0], order[:, 1], order[:, 2]
    u0 = UW[ar, :, o0] / w[ar, o0, None]; u1 = UW[ar, :, o1] / w[ar, o1, None]
    has2 = w[ar, o2] > thr; has1 = w[ar, o1] > thr
    BRANCHES["cross"] += int((has1 & ~has2).sum()); BRANCHES["nan_R"] += int((~has1).sum())
    cross = np.stack([u0[:, 1] * u1[:, 2] - u0[:, 2] * u1[:, 1], u0[:, 2] * u1[:, 0] - u0[:, 0] * u1[:, 2], u0[:, 0] * u1[:, 1] - u0[:, 1] * u1[:, 0]], axis=1)
    u2 = np.where(has2[:, None], UW[ar, :, o2] / w[ar, o2, None], cross)
    v0, v1, v2 = V[ar, :, o0], V[ar, :, o1], V[ar, :, o2]
    R = u0[:, :, None] * v0[:, None, :] + u1[:, :, None] * v1[:, None, :] + u2[:, :, None] * v2[:, None, :]
    R = np.where(has1[:, None, None], R, f64(np.nan))
    det = R[:, 0, 0] * R[:, 1, 1] * R[:, 2, 2] + R[:, 0, 1] * R[:, 1, 2] * R[:, 2, 0] + R[:, 0, 2] * R[:, 1, 0] * R[:, 2, 1] - \
        R[:, 0, 2] * R[:, 1, 1] * R[:, 2, 0] - R[:, 0, 1] * R[:, 1, 0] * R[:, 2, 2] - R[:, 0, 0] * R[:, 1, 2] * R[:, 2, 1]
    R[:, 2, :] = np.where((det < 0)[:, None], -R[:, 2, :], R[:, 2, :])
    t = np.stack([pc0[:, i] - _dot3(R[:, i], pw0) for i in range(3)], axis=1)
    return R, t


def compute_pose(pws, us, K):
    """compute_pose (:522-570) for H sets of n correspondences: pws [H, n, 3], us [H, n, 2] (the float inputs, taken into double by add_correspondence), K = (fx, fy, cx,
    cy) floats taken into the doubles fu, fv, uc, vc.  Returns dict(R [H, 3, 3], t [H, 3], rep [H, 3], chosen [H]) in float64"""
    pws = np.asarray(pws, f32).astype(f64); us = np.asarray(us, f32).astype(f64)
    H, n, _ = pws.shape
    fu, fv, uc, vc = [f64(f32(k)) for k in K]
    nn = f64(n)
    with _quiet():
        # choose_control_points (:420-454)
        c0 = np.zeros((H, 3), f64)
        for i in range(n):
            c0 = c0 + pws[:, i]
        c0 = c0 / nn
        P = np.zeros((H, 3, 3), f64)
        for i in range(n):
            d = pws[:, i] - c0
            P = P + d[:, :, None] * d[:, None, :]                      # the upper triangle is what is read; the product is commutative, so the mirror is exact
        lam, V = jacobi_eig(P)
        lam = np.abs(lam); order = _orders(lam); ar = np.arange(H)
        cws = np.empty((H, 4, 3), f64); cws[:, 0] = c0
        for i in range(1, 4):
            o = order[:, i - 1]
            k = np.sqrt(lam[ar, o] / nn)
            cws[:, i] = c0 + k[:, None] * V[ar, :, o]
        # compute_barycentric_coordinates (:456-466): cvInvert(CC, CV_SVD), column j = the solve with e_j
        CC = np.empty((H, 3, 3), f64)
        for i in range(3):
            for j in range(1, 4):
                CC[:, i, j - 1] = cws[:, j, i] - cws[:, 0, i]
        dec = hestenes(CC); ci = np.empty((H, 3, 3), f64)
        for j in range(3):
            e = np.zeros((H, 3), f64); e[:, j] = 1.0
            ci[:, :, j] = sv_solve(dec, e)
        # fill_M + cvMulTransposed (:481-496, :527-537)
        S = np.zeros((H, 78), f64)
        zero = np.zeros(H, f64)
        for i in range(n):
            a = _alphas(ci, c0, pws[:, i]); u, v = us[:, i, 0], us[:, i, 1]
            M1 = np.stack([x for j in range(4) for x in (a[:, j] * fu, zero, a[:, j] * (uc - u))], axis=1)
            M2 = np.stack([x for j in range(4) for x in (zero, a[:, j] * fv, a[:, j] * (vc - v))], axis=1)
            S = S + M1[:, _MTM_A] * M1[:, _MTM_B]
            S = S + M2[:, _MTM_A] * M2[:, _MTM_B]
        MtM = np.empty((H, 12, 12), f64); MtM[:, _MTM_A, _MTM_B] = S; MtM[:, _MTM_B, _MTM_A] = S
        lam, V = jacobi_eig(MtM)
        order = _orders(np.abs(lam))
        v4 = np.stack([V[ar, :, order[:, 11 - i]] for i in range(4)], axis=1)      # rows 11, 10, 9, 8 of ut
        L = _L_6x10(v4)
        rho = np.stack([_dist2(cws[:, 0], cws[:, 1]), _dist2(cws[:, 0], cws[:, 2]), _dist2(cws[:, 0], cws[:, 3]), _dist2(cws[:, 1], cws[:, 2]),
                        _dist2(cws[:, 1], cws[:, 3]), _dist2(cws[:, 2], cws[:, 3])], axis=1)
        Rs, ts, reps = [], [], []
        for which in (1, 2, 3):
            betas = _gauss_newton(L, rho, _find_betas(which, L, rho))
            ccs = np.zeros((H, 4, 3), f64)                              # compute_ccs (:498-509)
            for i in range(4):
                ccs = ccs + betas[:, i, None, None] * v4[:, i].reshape(H, 4, 3)
            # solve_for_sign (:681-694): pcs[2] of the first correspondence; negating ccs negates every pc exactly
            pc_first = _pc(_alphas(ci, c0, pws[:, 0]), ccs)
            ccs = np.where((pc_first[:, 2] < 0.0)[:, None, None], -ccs, ccs)
            pc0 = np.zeros((H, 3), f64); pw0 = np.zeros((H, 3), f64)
            for i in range(n):
                pc0 = pc0 + _pc(_alphas(ci, c0, pws[:, i]), ccs); pw0 = pw0 + pws[:, i]
            pc0 = pc0 / nn; pw0 = pw0 / nn
            abt = np.zeros((H, 3, 3), f64)
            for i in range(n):
                pc = _pc(_alphas(ci, c0, pws[:, i]), ccs)
                abt = abt + (pc - pc0)[:, :, None] * (pws[:, i] - pw0)[:, None, :]
            R, t = estimate_R_and_t(pc0, pw0, abt)
            sum2 = np.zeros(H, f64)                                     # reprojection_error (:595-612)
            for i in range(n):
                pw = pws[:, i]
                Xc = _dot3(R[:, 0], pw) + t[:, 0]; Yc = _dot3(R[:, 1], pw) + t[:, 1]
                inv_Zc = f64(1.0) / (_dot3(R[:, 2], pw) + t[:, 2])
                ue = uc + fu * Xc * inv_Zc; ve = vc + fv * Yc * inv_Zc
                u, v = us[:, i, 0], us[:, i, 1]
                sum2 = sum2 + np.sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve))
            Rs.append(R); ts.append(t); reps.append(sum2 / nn)
        chosen = np.where(reps[1] < reps[0], 2, 1)
        rep_c = np.where(chosen == 2, reps[1], reps[0])
        chosen = np.where(reps[2] < rep_c, 3, chosen)
        Rs, ts = np.stack(Rs, axis=1), np.stack(ts, axis=1)
        return dict(R=Rs[ar, chosen - 1], t=ts[ar, chosen - 1], rep=np.stack(reps, axis=1), chosen=chosen.astype(np.int64))


def pose16(h):
    """the per-hypothesis layout of pose_out: R[9], t[3], the three rep_errors, chosen N, as doubles"""
    H = len(h["t"])
    return np.concatenate([h["R"].reshape(H, 9), h["t"], h["rep"], h["chosen"].astype(f64)[:, None]], axis=1)


# ---- CheckInliers (:353-384) ----
def check_inliers(pr, R, t):
    """R [H, 3, 3], t [H, 3] doubles -> bool [H, N], in the source's mixed types"""
    R = np.asarray(R, f64).reshape(-1, 3, 3); t = np.asarray(t, f64).reshape(-1, 3)
    X = pr["p3dw"].astype(f64)[None]; P = pr["p2d"].astype(f64)[None]
    fu, fv, uc, vc = [f64(f32(k)) for k in pr["K"]]
    with _quiet():
        row = lambda i: R[:, i, 0, None] * X[:, :, 0] + R[:, i, 1, None] * X[:, :, 1] + R[:, i, 2, None] * X[:, :, 2] + t[:, i, None]
        Xc = row(0).astype(f32); Yc = row(1).astype(f32)
        invZc = (f64(1.0) / row(2)).astype(f32)
        ue = uc + fu * Xc.astype(f64) * invZc.astype(f64); ve = vc + fv * Yc.astype(f64) * invZc.astype(f64)
        dX = (P[:, :, 0] - ue).astype(f32); dY = (P[:, :, 1] - ve).astype(f32)
        err = dX * dX + dY * dY
        return err < pr["max_err"][None]


# ---- problems ----
def problem(p3dw, p2d, sigma2, K, th2=5.991):
    p3dw = np.ascontiguousarray(p3dw, f32).reshape(-1, 3); p2d = np.ascontiguousarray(p2d, f32).reshape(-1, 2); sigma2 = np.ascontiguousarray(sigma2, f32).reshape(-1)
    return dict(n=len(sigma2), p3dw=p3dw, p2d=p2d, sigma2=sigma2, K=tuple(f32(k) for k in K), max_err=max_errors(sigma2, th2))


def constructor(kp, octave, matched_ids, points, scale, K, th2=5.991):
    """the constructor over a Frame / KeyFrame (:67-110 / :112-155): kp [n, 2] = mvKeysUn[i].pt, octave [n], matched_ids [n] uint64 (NO_MAP_POINT = NULL), points = {id:
    dict(pos, bad)} (an id the map does not hold is skipped, as a NULL is), scale = mvScaleFactors.  Returns (problem, mvKeyPointIndices)"""
    idx, X, P, s2 = [], [], [], []
    sc = np.asarray(scale, f32)
    for i in range(len(matched_ids)):
        mid = int(matched_ids[i])
        if mid == NO_MAP_POINT or mid not in points or points[mid]["bad"]:
            continue
        o = min(max(int(octave[i]), 0), len(sc) - 1)
        idx.append(i); X.append(points[mid]["pos"]); P.append(kp[i]); s2.append(sc[o] * sc[o])
    return problem(np.array(X, f32).reshape(-1, 3), np.array(P, f32).reshape(-1, 2), np.array(s2, f32), K, th2), np.array(idx, np.int32)


# ---- the rule that replaces iterate()'s state ----
def records_of(counts, m):
    """0-based iterations i with c_i >= m and c_i > every earlier c_j >= m"""
    out, best = [], 0
    for i, c in enumerate(counts):
        if c >= m and c > best:
            best = c; out.append(i)
    return out


def replay(counts, refine_ok, m, cap, n_iterations_seq):
    """iterate() as a pure function.  counts: c_i of every evaluated hypothesis; refine_ok: {record i: bool}; the calls iterate(n) for n in n_iterations_seq, from
    mnIterations = 0.  Returns per call (kind, record, mnIterations after, bNoMore): kind 'refined' = the refined pose of `record`, 'best' = its unrefined pose, None =
    an empty Mat.  A call from mnIterations = s returns at the first i >= s with c_i >= m and b(i) ok, else at max(cap, s + n) with bNoMore."""
    recs = records_of(counts, m); out = []; s = 0
    b = [None] * len(counts); last = None
    for i in range(len(counts)):
        if i in recs:
            last = i
        b[i] = last
    for n in n_iterations_seq:
        end = max(cap, s + n)
        hit = next((i for i in range(s, min(end, len(counts))) if counts[i] >= m and refine_ok[b[i]]), None)
        if hit is not None:
            s = hit + 1; out.append(("refined", b[hit], s, False)); continue
        s = end
        bi = b[min(end, len(counts)) - 1] if end > 0 and len(counts) else None
        out.append(("best" if bi is not None else None, bi, s, True))
    return out


def iterate_literal(counts, refine_ok, m, cap, n_iterations_seq):
    """a literal, stateful transcription of iterate() (:210-303) + Refine()'s verdict (:337), over given per-iteration counts (N >= m)"""
    st = dict(mnIterations=0, mnBestInliers=0, best=None)
    out = []

    def iterate(nIterations):
        bNoMore = False
        nCurrentIterations = 0
        while st["mnIterations"] < cap or nCurrentIterations < nIterations:
            nCurrentIterations += 1; st["mnIterations"] += 1
            mnInliersi = counts[st["mnIterations"] - 1]
            if mnInliersi >= m:
                if mnInliersi > st["mnBestInliers"]:
                    st["mnBestInliers"] = mnInliersi; st["best"] = st["mnIterations"] - 1
                if refine_ok[st["best"]]:
                    return ("refined", st["best"], st["mnIterations"], bNoMore)
        if st["mnIterations"] >= cap:
            bNoMore = True
            if st["mnBestInliers"] >= m:
                return ("best", st["best"], st["mnIterations"], bNoMore)
        return (None, None, st["mnIterations"], bNoMore)

    for n in n_iterations_seq:
        out.append(iterate(n))
    return out


# ---- a whole call ----
def gather_sets(pr, idx):
    idx = np.asarray(idx, np.int64)
    return pr["p3dw"][idx], pr["p2d"][idx]


def tcw32(R, t):
    """Rcw.convertTo(CV_32F), tcw.convertTo(CV_32F) into the 3 x 4 [R | t] (:262-268)"""
    return np.concatenate([np.asarray(R, f64).reshape(3, 3), np.asarray(t, f64).reshape(3, 1)], axis=1).astype(f32).reshape(12)


def ransac(pr, rand_values, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991, tail_iterations=0, pose_dev=None, refine_dev=None):
    """everything a call returns for one problem.  rand_values [>= cap + tail, min_set].  pose_dev [its, 16] / refine_dev {iteration: [16]}: evaluate everything
    downstream of the (device's) poses instead of the restatement's own.  Returns dict(cap, m, its, sets, pose [its, 16], counts, flags [its, N], records = [dict(i,
    n_inliers, Tcw_best, flags, set, pose [16], n_refined, refine_ok, Tcw_refined, refined_flags)])"""
    N = pr["n"]; cap, m = ransac_parameters(N, probability, min_inliers, max_iterations, min_set, epsilon, th2)
    its = 0 if cap == 0 else cap + tail_iterations
    rv = np.asarray(rand_values).reshape(-1, min_set)
    out = dict(cap=cap, m=m, its=its, sets=np.zeros((0, min_set), np.int64), pose=np.zeros((0, 16), f64), counts=np.zeros(0, np.int32), flags=np.zeros((0, N), bool), records=[])
    if its == 0:
        return out
    sets = np.array([draw_set(rv[i], min_set, N) for i in range(its)], np.int64)
    pose = pose16(compute_pose(*gather_sets(pr, sets), pr["K"]))
    use = pose if pose_dev is None else np.asarray(pose_dev, f64).reshape(its, 16)
    flags = check_inliers(pr, use[:, :9], use[:, 9:12])
    counts = flags.sum(axis=1).astype(np.int32)
    out.update(sets=sets, pose=pose, counts=counts, flags=flags)
    for i in records_of(counts, m):
        inl = np.flatnonzero(flags[i])
        rp = pose16(compute_pose(*[x[None] for x in gather_sets(pr, inl)], pr["K"]))[0]
        ru = rp if refine_dev is None else np.asarray(refine_dev[i], f64).reshape(16)
        rfl = check_inliers(pr, ru[:9], ru[9:12])[0]
        out["records"].append(dict(i=i, n_inliers=int(counts[i]), Tcw_best=tcw32(use[i, :9], use[i, 9:12]), flags=flags[i], set=inl, pose=rp, n_refined=int(rfl.sum()),
                                   refine_ok=bool(rfl.sum() > m), Tcw_refined=tcw32(ru[:9], ru[9:12]), refined_flags=rfl))
    return out


def same_bits(a, b):
    """equal as bit patterns, any NaN equal to any NaN"""
    a = np.asarray(a, f64); b = np.asarray(b, f64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


# ---- scenes ----
KITTI = (718.856, 718.856, 607.1928, 185.2157)


def _rot(rng, max_angle):
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax); ang = rng.uniform(0.05, max_angle)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def scene(seed, n, inlier_share=0.5, noise_px=0.0, max_angle=0.6, n_inliers=None):
    """n world points in the scene box of sim3solver_reference.scene seen by a KITTI-calibrated camera at a known pose; all but a share of them get an unrelated pixel.
    n_inliers: exactly that many true correspondences (the first ones after a seeded shuffle).  Returns (problem, dict(R, t, inlier))"""
    rng = np.random.default_rng(seed)
    R = _rot(rng, max_angle); t = rng.uniform(-0.5, 0.5, 3)
    Xc = np.stack([rng.uniform(-6, 6, n), rng.uniform(-2, 2, n), rng.uniform(5, 30, n)], axis=1)
    Xw = (Xc - t) @ R                                                  # Xc = R Xw + t
    fx, fy, cx, cy = KITTI
    uv = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], axis=1) + rng.normal(scale=1.0, size=(n, 2)) * noise_px
    if n_inliers is None:
        inl = rng.random(n) < inlier_share
    else:
        inl = np.zeros(n, bool); inl[rng.permutation(n)[:n_inliers]] = True
    uv[~inl] = np.stack([rng.uniform(0, 1241, (~inl).sum()), rng.uniform(0, 376, (~inl).sum())], axis=1)
    sig = (f32(1.2) ** rng.integers(0, 4, n).astype(f32)) ** 2
    return problem(Xw, uv, sig.astype(f32), KITTI), dict(R=R, t=t, inlier=inl)


def draws(seed, n_problems, n_iterations, min_set=4):
    return np.random.RandomState(seed).randint(0, RAND_RANGE, (n_problems, n_iterations, min_set)).astype(np.int32)

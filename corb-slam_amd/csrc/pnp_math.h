// pnp_math.h -- the arithmetic of PnPsolver::compute_pose and CheckInliers (C/src/PnPsolver.cc:353-384, :420-570, :595-995), stated once for the kernels of
// pnp_ransac_kernels.hip and for a stand-alone host program (tests/host/pnp_math_main.cpp).  Everything is double arithmetic in the order of the source, unfused
// (-ffp-contract=off); tests/pnpsolver_reference.py restates every line and DESIGN.md section 2 lists the readings.  The decompositions OpenCV would supply:
//   cvSVD of the symmetric PW0tPW0 / MtM with CV_SVD_U_T  -> pnp_jacobi_eig: cyclic Jacobi, a pair rotated iff |a_pq| > 2^-60 max|A_ij|, row-cyclic, at most 30 sweeps
//   cvInvert / cvSolve with CV_SVD, cvSVD(ABt)             -> pnp_hestenes: one-sided Jacobi, rotate iff |a_p . a_q| > 1e-15 |a_p| |a_q|, at most 30 sweeps; terms with
//                                                             w_k <= 2^-51 sum_j w_j are dropped
// On the device a function here is entered by all 64 lanes of a single-wave workgroup with its PnpWork in LDS: PNP_FOR_LANES spreads independent entries over the
// lanes (each entry is the same expression whichever lane evaluates it), PNP_LANE0 marks what one lane does alone, PNP_SYNC orders the two.  On the host the same text
// is a serial loop.
#pragma once
#include <math.h>
#include "ransac_common.h"

#if defined(__HIPCC__)
#define PNP_HD __host__ __device__ __forceinline__
#else
#define PNP_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define PNP_LANE ((int)threadIdx.x)
#define PNP_LANES 64
#define PNP_SYNC() __syncthreads()
#else
#define PNP_LANE 0
#define PNP_LANES 1
#define PNP_SYNC() ((void)0)
#endif
#define PNP_FOR_LANES(e, count) for (int e = PNP_LANE; e < (count); e += PNP_LANES)
#define PNP_LANE0 if (PNP_LANE == 0)

// one correspondence: mvP3Dw, mvP2D, mvMaxError
struct PnpCorr { float X[3], u[2], max_err; };
// what compute_pose leaves: R row-major, t, rep_errors[1..3], the chosen N
struct PnpPose { double R[9], t[3], rep[3], chosen; };

struct PnpWork {
    double A[144], V[144];                       // the symmetric matrix under pnp_jacobi_eig and its rotations
    double lam[12]; int order[12];
    double v4[4][12];                            // rows 11, 10, 9, 8 of ut
    double cws[4][3], cci[9];                    // control points, CC^-1
    double sv_a[30], sv_v[25], sv_w[5], sv_b[6], sv_x[5]; int sv_order[5];
    double l[60], rho[6], betas[4], gn_a[24], gn_b[6], gn_x[4], qr_a1[4], qr_a2[4];
    double ccs[4][3], pc0[3], pw0[3], abt[9];
    double Rs[3][9], ts[3][3], rep[3];
};

// ---- sets of correspondences, walked in ascending order ----
struct PnpIndexSet {                             // the min_set draws of one hypothesis
    const PnpCorr* corr; const int* idx; int n;
    struct Cursor { int k; };
    PNP_HD void start(Cursor& c) const { c.k = 0; }
    PNP_HD bool next(Cursor& c, double* pw, double* u) const
    {
        if (c.k >= n) return false;
        const PnpCorr& p = corr[idx[c.k++]];
        pw[0] = (double)p.X[0]; pw[1] = (double)p.X[1]; pw[2] = (double)p.X[2]; u[0] = (double)p.u[0]; u[1] = (double)p.u[1];
        return true;
    }
};
struct PnpMaskSet {                              // Refine(): the set bits of a record's inlier mask (:310-326)
    const PnpCorr* corr; const unsigned long long* mask; int words; int n;
    struct Cursor { int w; unsigned long long bits; };
    PNP_HD void start(Cursor& c) const { c.w = -1; c.bits = 0; }
    PNP_HD bool next(Cursor& c, double* pw, double* u) const
    {
        while (c.bits == 0) { if (++c.w >= words) return false; c.bits = mask[c.w]; }
        const PnpCorr& p = corr[c.w * 64 + __builtin_ctzll(c.bits)];
        c.bits &= c.bits - 1;
        pw[0] = (double)p.X[0]; pw[1] = (double)p.X[1]; pw[2] = (double)p.X[2]; u[0] = (double)p.u[0]; u[1] = (double)p.u[1];
        return true;
    }
};

// ---- cvSVD of a symmetric n x n matrix: cyclic Jacobi.  A (row-major, destroyed: its diagonal becomes the eigenvalues), V = the rotations from I (columns =
// eigenvectors).  Entered by all lanes; lane k updates row / column entry k of a rotation.  NaN rotates nothing.
PNP_HD void pnp_jacobi_eig(double* A, double* V, int n)
{
    PNP_FOR_LANES(e, n * n) V[e] = (e / n == e % n) ? 1.0 : 0.0;
    PNP_SYNC();
    double scale = 0;
    for (int e = 0; e < n * n; e++) { const double v = fabs(A[e]); if (v > scale) scale = v; }
    const double tiny = scale * 8.673617379884035e-19;                 // 2^-60
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = A[p * n + q];
                if (!(fabs(apq) > tiny)) continue;                     // (the same for every lane)
                rotated = true;
                const double app = A[p * n + p], aqq = A[q * n + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                PNP_SYNC();
                PNP_FOR_LANES(k, n) {
                    if (k == p) { A[p * n + p] = app - t * apq; A[p * n + q] = 0.0; }
                    else if (k == q) { A[q * n + q] = aqq + t * apq; A[q * n + p] = 0.0; }
                    else {
                        const double akp = A[k * n + p], akq = A[k * n + q];
                        const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
                        A[k * n + p] = np_; A[p * n + k] = np_; A[k * n + q] = nq_; A[q * n + k] = nq_;
                    }
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq; V[k * n + q] = s * vkp + c * vkq;
                }
                PNP_SYNC();
            }
        if (!rotated) break;
    }
}
// descending order of key[0..n), the lower index first among equals (a selection with a strict comparison)
PNP_HD void pnp_order_desc(const double* key, int n, int* order)
{
    for (int i = 0; i < n; i++) order[i] = i;
    for (int i = 0; i < n - 1; i++) {
        int b = i;
        for (int j = i + 1; j < n; j++) if (key[order[j]] > key[order[b]]) b = j;
        const int ob = order[b];
        for (int j = b; j > i; j--) order[j] = order[j - 1];
        order[i] = ob;
    }
}

// ---- cvSVD / cvSolve / cvInvert with CV_SVD: one-sided (Hestenes) Jacobi on the columns of the m x n A (row-major, becomes U W), V from I; w = column norms, order =
// descending w.  One lane.
PNP_HD void pnp_hestenes(double* A, double* V, double* w, int* order, int m, int n)
{
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int k = 0; k < m; k++) { const double ap = A[k * n + p], aq = A[k * n + q]; alpha += ap * ap; beta += aq * aq; gamma += ap * aq; }
                if (!(fabs(gamma) > 1e-15 * sqrt(alpha * beta))) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int k = 0; k < m; k++) { const double up = A[k * n + p], uq = A[k * n + q]; A[k * n + p] = c * up - s * uq; A[k * n + q] = s * up + c * uq; }
                for (int k = 0; k < n; k++) { const double vp = V[k * n + p], vq = V[k * n + q]; V[k * n + p] = c * vp - s * vq; V[k * n + q] = s * vp + c * vq; }
            }
        if (!rotated) break;
    }
    for (int j = 0; j < n; j++) { double s = 0; for (int k = 0; k < m; k++) s += A[k * n + j] * A[k * n + j]; w[j] = sqrt(s); }
    pnp_order_desc(w, n, order);
}
// the drop threshold of the pseudo-inverse: 2 * DBL_EPSILON * sum_j w_j
PNP_HD double pnp_sv_threshold(const double* w, int n)
{
    double s = 0;
    for (int j = 0; j < n; j++) s += w[j];
    return 4.440892098500626e-16 * s;                                  // 2^-51
}
// x = sum over kept k (descending w) of v_k ((u_k . b) / w_k), u_k = a_k / w_k
PNP_HD void pnp_sv_solve(const double* A, const double* V, const double* w, const int* order, int m, int n, const double* b, double* x)
{
    const double thr = pnp_sv_threshold(w, n);
    for (int i = 0; i < n; i++) x[i] = 0.0;
    for (int kk = 0; kk < n; kk++) {
        const int k = order[kk];
        if (!(w[k] > thr)) continue;
        double dot = 0;
        for (int i = 0; i < m; i++) dot += (A[i * n + k] / w[k]) * b[i];
        const double coef = dot / w[k];
        for (int i = 0; i < n; i++) x[i] += V[i * n + k] * coef;
    }
}

// ---- pieces of compute_pose ----
// v[i] for an index that differs between lanes, without indexing a register array
PNP_HD double pnp_sel3(const double* v, int i) { return i == 0 ? v[0] : (i == 1 ? v[1] : v[2]); }
PNP_HD double pnp_sel4(const double* v, int i) { return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3])); }
PNP_HD double pnp_dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PNP_HD double pnp_dist2(const double* p1, const double* p2)
{
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}
// compute_barycentric_coordinates' row (:468-478)
PNP_HD void pnp_alphas(const double* ci, const double* c0, const double* pi, double* a)
{
    for (int j = 0; j < 3; j++)
        a[1 + j] = ci[3 * j] * (pi[0] - c0[0]) + ci[3 * j + 1] * (pi[1] - c0[1]) + ci[3 * j + 2] * (pi[2] - c0[2]);
    a[0] = 1.0 - a[1] - a[2] - a[3];
}
// fill_M (:481-496): entry `col` of row M1 (row = 0) or M2 (row = 1); K = fu, fv, uc, vc
PNP_HD double pnp_M(int row, int col, const double* as, const double* u, const double* K)
{
    const int r = col % 3;
    const double ai = pnp_sel4(as, col / 3);
    if (r == 2) return ai * (K[2 + row] - u[row]);
    return r == row ? ai * K[row] : 0.0;
}
// compute_pcs' row (:517-518)
PNP_HD void pnp_pc(const double* a, const double ccs[4][3], double* pc)
{
    for (int j = 0; j < 3; j++) pc[j] = a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
}
// compute_L_6x10 (:805-845); v[i] = row 11 - i of ut
PNP_HD void pnp_L_6x10(const double v[4][12], double* l)
{
    for (int r = 0, a = 0, b = 1; r < 6; r++) {
        double dv[4][3];
        for (int i = 0; i < 4; i++) for (int k = 0; k < 3; k++) dv[i][k] = v[i][3 * a + k] - v[i][3 * b + k];
        double* row = l + 10 * r;
        row[0] = pnp_dot3(dv[0], dv[0]);
        row[1] = 2.0 * pnp_dot3(dv[0], dv[1]);
        row[2] = pnp_dot3(dv[1], dv[1]);
        row[3] = 2.0 * pnp_dot3(dv[0], dv[2]);
        row[4] = 2.0 * pnp_dot3(dv[1], dv[2]);
        row[5] = pnp_dot3(dv[2], dv[2]);
        row[6] = 2.0 * pnp_dot3(dv[0], dv[3]);
        row[7] = 2.0 * pnp_dot3(dv[1], dv[3]);
        row[8] = 2.0 * pnp_dot3(dv[2], dv[3]);
        row[9] = pnp_dot3(dv[3], dv[3]);
        b++;
        if (b > 3) { a++; b = a + 1; }
    }
}
// compute_rho (:847-855)
PNP_HD void pnp_rho(const double cws[4][3], double* rho)
{
    rho[0] = pnp_dist2(cws[0], cws[1]); rho[1] = pnp_dist2(cws[0], cws[2]); rho[2] = pnp_dist2(cws[0], cws[3]);
    rho[3] = pnp_dist2(cws[1], cws[2]); rho[4] = pnp_dist2(cws[1], cws[3]); rho[5] = pnp_dist2(cws[2], cws[3]);
}
// find_betas_approx_1 / 2 / 3 (:712-803): cvSolve(L_6xnc, Rho, CV_SVD) over the columns `cols`
PNP_HD void pnp_find_betas(int which, PnpWork& W)
{
    const int nc = which == 1 ? 4 : (which == 2 ? 3 : 5);
    for (int i = 0; i < 6; i++) {
        for (int j = 0; j < nc; j++) W.sv_a[i * nc + j] = W.l[10 * i + (which == 1 && j >= 2 ? 3 * (j - 1) : j)];
        W.sv_b[i] = W.rho[i];
    }
    pnp_hestenes(W.sv_a, W.sv_v, W.sv_w, W.sv_order, 6, nc);
    pnp_sv_solve(W.sv_a, W.sv_v, W.sv_w, W.sv_order, 6, nc, W.sv_b, W.sv_x);
    const double* b = W.sv_x; double* betas = W.betas;
    if (which == 1) {
        if (b[0] < 0) { betas[0] = sqrt(-b[0]); betas[1] = -b[1] / betas[0]; betas[2] = -b[2] / betas[0]; betas[3] = -b[3] / betas[0]; }
        else { betas[0] = sqrt(b[0]); betas[1] = b[1] / betas[0]; betas[2] = b[2] / betas[0]; betas[3] = b[3] / betas[0]; }
        return;
    }
    if (b[0] < 0) { betas[0] = sqrt(-b[0]); betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0; }
    else { betas[0] = sqrt(b[0]); betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0; }
    if (b[1] < 0) betas[0] = -betas[0];
    betas[2] = which == 3 ? b[3] / betas[0] : 0.0;
    betas[3] = 0.0;
}
// qr_solve (:905-995) for the 6 x 4 system of gauss_newton, line for line; the singular return leaves X as it was.  (The search for eta reads rows k .. nr - 2, as
// the source's pointer does.)
PNP_HD void pnp_qr_solve(double* A, double* b, double* X, double* A1, double* A2)
{
    const int nr = 6, nc = 4;
    for (int k = 0; k < nc; k++) {
        double eta = fabs(A[k * nc + k]);
        for (int i = k + 1; i < nr; i++) { const double elt = fabs(A[(i - 1) * nc + k]); if (eta < elt) eta = elt; }
        if (eta == 0) { A1[k] = A2[k] = 0.0; return; }
        double sum = 0.0; const double inv_eta = 1. / eta;
        for (int i = k; i < nr; i++) { A[i * nc + k] *= inv_eta; sum += A[i * nc + k] * A[i * nc + k]; }
        double sigma = sqrt(sum);
        if (A[k * nc + k] < 0) sigma = -sigma;
        A[k * nc + k] += sigma;
        A1[k] = sigma * A[k * nc + k];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            double s2 = 0;
            for (int i = k; i < nr; i++) s2 += A[i * nc + k] * A[i * nc + j];
            const double tau = s2 / A1[k];
            for (int i = k; i < nr; i++) A[i * nc + j] -= tau * A[i * nc + k];
        }
    }
    for (int j = 0; j < nc; j++) {
        double tau = 0;
        for (int i = j; i < nr; i++) tau += A[i * nc + j] * b[i];
        tau /= A1[j];
        for (int i = j; i < nr; i++) b[i] -= tau * A[i * nc + j];
    }
    X[nc - 1] = b[nc - 1] / A2[nc - 1];
    for (int i = nc - 2; i >= 0; i--) {
        double sum = 0;
        for (int j = i + 1; j < nc; j++) sum += A[i * nc + j] * X[j];
        X[i] = (b[i] - sum) / A2[i];
    }
}
// gauss_newton (:885-903) with compute_A_and_b_gauss_newton (:857-883)
PNP_HD void pnp_gauss_newton(PnpWork& W)
{
    double* betas = W.betas;
    for (int i = 0; i < 4; i++) W.gn_x[i] = 0.0;
    for (int it = 0; it < 5; it++) {
        for (int i = 0; i < 6; i++) {
            const double* rowL = W.l + i * 10; double* rowA = W.gn_a + i * 4;
            rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
            rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
            rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
            rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
            W.gn_b[i] = W.rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] + rowL[3] * betas[0] * betas[2] +
                                    rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] + rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] +
                                    rowL[8] * betas[2] * betas[3] + rowL[9] * betas[3] * betas[3]);
        }
        pnp_qr_solve(W.gn_a, W.gn_b, W.gn_x, W.qr_a1, W.qr_a2);
        for (int i = 0; i < 4; i++) betas[i] += W.gn_x[i];
    }
}
// compute_ccs (:498-509)
PNP_HD void pnp_ccs(const double* betas, const double v[4][12], double ccs[4][3])
{
    for (int j = 0; j < 4; j++) for (int k = 0; k < 3; k++) ccs[j][k] = 0.0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 3; k++) ccs[j][k] += betas[i] * v[i][3 * j + k];
}
// estimate_R_and_t (:614-672) from the sums pc0, pw0 (already divided) and ABt: R = U V^T of the Hestenes SVD of ABt; a dropped smallest singular value's left vector
// is the cross product of the other two, two dropped ones leave NaN
PNP_HD void pnp_estimate_R_and_t(PnpWork& W, double* R, double* t)
{
    for (int e = 0; e < 9; e++) W.sv_a[e] = W.abt[e];
    pnp_hestenes(W.sv_a, W.sv_v, W.sv_w, W.sv_order, 3, 3);
    const double thr = pnp_sv_threshold(W.sv_w, 3);
    const int o0 = W.sv_order[0], o1 = W.sv_order[1], o2 = W.sv_order[2];
    if (!(W.sv_w[o1] > thr)) {
        for (int e = 0; e < 9; e++) R[e] = __builtin_nan("");
    } else {
        double u0[3], u1[3], u2[3];
        for (int i = 0; i < 3; i++) { u0[i] = W.sv_a[i * 3 + o0] / W.sv_w[o0]; u1[i] = W.sv_a[i * 3 + o1] / W.sv_w[o1]; }
        if (W.sv_w[o2] > thr) { for (int i = 0; i < 3; i++) u2[i] = W.sv_a[i * 3 + o2] / W.sv_w[o2]; }
        else { u2[0] = u0[1] * u1[2] - u0[2] * u1[1]; u2[1] = u0[2] * u1[0] - u0[0] * u1[2]; u2[2] = u0[0] * u1[1] - u0[1] * u1[0]; }
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[3 * i + j] = u0[i] * W.sv_v[j * 3 + o0] + u1[i] * W.sv_v[j * 3 + o1] + u2[i] * W.sv_v[j * 3 + o2];
    }
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
    if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
    t[0] = W.pc0[0] - pnp_dot3(R, W.pw0);
    t[1] = W.pc0[1] - pnp_dot3(R + 3, W.pw0);
    t[2] = W.pc0[2] - pnp_dot3(R + 6, W.pw0);
}
// one term of reprojection_error (:599-609)
PNP_HD double pnp_reprojection_term(const double* R, const double* t, const double* pw, const double* uv, const double* K)
{
    const double Xc = pnp_dot3(R, pw) + t[0], Yc = pnp_dot3(R + 3, pw) + t[1];
    const double inv_Zc = 1.0 / (pnp_dot3(R + 6, pw) + t[2]);
    const double ue = K[2] + K[0] * Xc * inv_Zc, ve = K[3] + K[1] * Yc * inv_Zc;
    return sqrt((uv[0] - ue) * (uv[0] - ue) + (uv[1] - ve) * (uv[1] - ve));
}

// compute_pose (:522-570) on the correspondences of S; K = fu, fv, uc, vc as the doubles of PnPsolver.h.  Entered by all lanes; `out` is written by lane 0.
template <class Set>
PNP_HD void pnp_compute_pose(const Set& S, const double* K, PnpWork& W, PnpPose& out)
{
    const int n = S.n;
    typename Set::Cursor cur; double pw[3], uv[2];
    // choose_control_points (:420-454)
    PNP_FOR_LANES(j, 3) {
        double s = 0;
        for (S.start(cur); S.next(cur, pw, uv);) s += pnp_sel3(pw, j);
        W.cws[0][j] = s / n;
    }
    PNP_SYNC();
    PNP_FOR_LANES(e, 6) {                                              // cvMulTransposed: the upper triangle, mirrored
        const int a = e < 3 ? 0 : (e < 5 ? 1 : 2), b = e < 3 ? e : (e < 5 ? e - 2 : 2);
        double s = 0;
        for (S.start(cur); S.next(cur, pw, uv);) s += (pnp_sel3(pw, a) - W.cws[0][a]) * (pnp_sel3(pw, b) - W.cws[0][b]);
        W.A[a * 3 + b] = s; W.A[b * 3 + a] = s;
    }
    PNP_SYNC();
    pnp_jacobi_eig(W.A, W.V, 3);
    PNP_LANE0 {
        double* lam = W.lam;
        for (int i = 0; i < 3; i++) lam[i] = fabs(W.A[i * 3 + i]);
        pnp_order_desc(lam, 3, W.order);
        for (int i = 1; i < 4; i++) {
            const int o = W.order[i - 1];
            const double k = sqrt(lam[o] / n);
            for (int j = 0; j < 3; j++) W.cws[i][j] = W.cws[0][j] + k * W.V[j * 3 + o];
        }
        // compute_barycentric_coordinates (:456-466): cvInvert(CC, CV_SVD)
        for (int i = 0; i < 3; i++) for (int j = 1; j < 4; j++) W.sv_a[3 * i + j - 1] = W.cws[j][i] - W.cws[0][i];
        pnp_hestenes(W.sv_a, W.sv_v, W.sv_w, W.sv_order, 3, 3);
        for (int j = 0; j < 3; j++) {
            for (int i = 0; i < 3; i++) W.sv_b[i] = i == j ? 1.0 : 0.0;
            pnp_sv_solve(W.sv_a, W.sv_v, W.sv_w, W.sv_order, 3, 3, W.sv_b, W.sv_x);
            for (int i = 0; i < 3; i++) W.cci[3 * i + j] = W.sv_x[i];
        }
    }
    PNP_SYNC();
    // fill_M + cvMulTransposed(M, MtM, 1) (:527-537): entry (a, b), a <= b, summed over the rows of M in ascending order
    PNP_FOR_LANES(e, 78) {
        int a = 0, b = e;
        while (b >= 12 - a) { b -= 12 - a; a++; }
        b += a;
        double s = 0, as[4];
        for (S.start(cur); S.next(cur, pw, uv);) {
            pnp_alphas(W.cci, W.cws[0], pw, as);
            s += pnp_M(0, a, as, uv, K) * pnp_M(0, b, as, uv, K);
            s += pnp_M(1, a, as, uv, K) * pnp_M(1, b, as, uv, K);
        }
        W.A[a * 12 + b] = s; W.A[b * 12 + a] = s;
    }
    PNP_SYNC();
    pnp_jacobi_eig(W.A, W.V, 12);
    PNP_LANE0 {
        for (int i = 0; i < 12; i++) W.lam[i] = fabs(W.A[i * 12 + i]);
        pnp_order_desc(W.lam, 12, W.order);
        for (int i = 0; i < 4; i++) for (int j = 0; j < 12; j++) W.v4[i][j] = W.V[j * 12 + W.order[11 - i]];
        pnp_L_6x10(W.v4, W.l);
        pnp_rho(W.cws, W.rho);
    }
    for (int m = 0; m < 3; m++) {
        PNP_LANE0 {
            pnp_find_betas(m + 1, W);
            pnp_gauss_newton(W);
            pnp_ccs(W.betas, W.v4, W.ccs);
            // solve_for_sign (:681-694): pcs[2] is the first correspondence's z; negating ccs negates every pc exactly
            double as[4], pc[3];
            S.start(cur);
            if (S.next(cur, pw, uv)) {
                pnp_alphas(W.cci, W.cws[0], pw, as); pnp_pc(as, W.ccs, pc);
                if (pc[2] < 0.0) for (int i = 0; i < 4; i++) for (int j = 0; j < 3; j++) W.ccs[i][j] = -W.ccs[i][j];
            }
        }
        PNP_SYNC();
        PNP_FOR_LANES(e, 6) {                                          // pc0, pw0 (:618-633)
            double s = 0.0, as[4], pc[3];
            for (S.start(cur); S.next(cur, pw, uv);) {
                if (e < 3) { pnp_alphas(W.cci, W.cws[0], pw, as); pnp_pc(as, W.ccs, pc); s += pnp_sel3(pc, e); }
                else s += pnp_sel3(pw, e - 3);
            }
            if (e < 3) W.pc0[e] = s / n; else W.pw0[e - 3] = s / n;
        }
        PNP_SYNC();
        PNP_FOR_LANES(e, 9) {                                          // ABt (:641-651)
            const int j = e / 3, c = e % 3;
            double s = 0.0, as[4], pc[3];
            for (S.start(cur); S.next(cur, pw, uv);) {
                pnp_alphas(W.cci, W.cws[0], pw, as); pnp_pc(as, W.ccs, pc);
                s += (pnp_sel3(pc, j) - W.pc0[j]) * (pnp_sel3(pw, c) - W.pw0[c]);
            }
            W.abt[e] = s;
        }
        PNP_SYNC();
        PNP_LANE0 {
            pnp_estimate_R_and_t(W, W.Rs[m], W.ts[m]);
            double sum2 = 0.0;
            for (S.start(cur); S.next(cur, pw, uv);) sum2 += pnp_reprojection_term(W.Rs[m], W.ts[m], pw, uv, K);
            W.rep[m] = sum2 / n;
        }
        PNP_SYNC();
    }
    PNP_LANE0 {
        int N = 1;
        if (W.rep[1] < W.rep[0]) N = 2;
        if (W.rep[2] < W.rep[N - 1]) N = 3;
        for (int e = 0; e < 9; e++) out.R[e] = W.Rs[N - 1][e];
        for (int e = 0; e < 3; e++) { out.t[e] = W.ts[N - 1][e]; out.rep[e] = W.rep[e]; }
        out.chosen = (double)N;
    }
}

// CheckInliers (:357-383) for one correspondence, in the source's mixed types: float Xc, Yc, invZc from double sums; double ue, ve; float distances and error
PNP_HD bool pnp_check_inlier(const double* R, const double* t, const PnpCorr& p, const double* K)
{
    const float Xc = (float)(R[0] * (double)p.X[0] + R[1] * (double)p.X[1] + R[2] * (double)p.X[2] + t[0]);
    const float Yc = (float)(R[3] * (double)p.X[0] + R[4] * (double)p.X[1] + R[5] * (double)p.X[2] + t[1]);
    const float invZc = (float)(1 / (R[6] * (double)p.X[0] + R[7] * (double)p.X[1] + R[8] * (double)p.X[2] + t[2]));
    const double ue = K[2] + K[0] * (double)Xc * (double)invZc;
    const double ve = K[3] + K[1] * (double)Yc * (double)invZc;
    const float distX = (float)((double)p.u[0] - ue), distY = (float)((double)p.u[1] - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < p.max_err;
}

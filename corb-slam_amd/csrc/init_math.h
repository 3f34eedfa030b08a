// init_math.h -- the arithmetic of the monocular Initializer (C/src/Initializer.cc), stated once for the kernels of init_kernels.hip and for a stand-alone host
// program (tests/host/initializer_main.cpp).  The source's float expressions are non-fused IEEE operations in the types C++ gives them (-ffp-contract=off);
// tests/initializer_reference.py restates every line and DESIGN.md section 2 lists the readings.  What OpenCV would supply:
//   cv::SVDecomp / cv::SVD::compute of a float matrix -> init_hestenes: the one-sided Jacobi of pnp_hestenes / np_svd_null in FP64 on the columns of the matrix taken
//                                                        into double (rotate iff |a_p . a_q| > 1e-15 |a_p| |a_q|, at most 30 sweeps), V from I; singular values
//                                                        descending, the lower index first among equals; w, U = a_k / w_k and V rounded to float once
//   Mat::inv() of a 3 x 3                             -> init_inv3: adjugate times 1 / det, both in double, each entry rounded once; det == 0 gives the zero matrix
//   a float 3 x 3 product                             -> init_mul3: entries accumulated in double in ascending k from 0.0, rounded once
//   cv::determinant, cv::norm, Mat::dot               -> sums in double
// On the device a body here is entered by every lane of a workgroup: INIT_FOR_LANES spreads independent entries over the lanes (each entry is the same expression
// whichever lane evaluates it), INIT_LANE0 marks what one lane does alone, INIT_SYNC orders the two.  On the host the same text is a serial loop.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "ransac_common.h"

#if defined(__HIPCC__)
#define INIT_HD __host__ __device__ __forceinline__
#else
#define INIT_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define INIT_LANE ((int)threadIdx.x)
#define INIT_LANES ((int)blockDim.x)
#define INIT_SYNC() __syncthreads()
#define INIT_BALLOT(p) __ballot(p)
#define INIT_SHARED_ADD(ptr, v) atomicAdd(ptr, v)
#else
#define INIT_LANE 0
#define INIT_LANES 1
#define INIT_SYNC() ((void)0)
#define INIT_BALLOT(p) ((p) ? 1ull : 0ull)
#define INIT_SHARED_ADD(ptr, v) (*(ptr) += (v))
#endif
#define INIT_FOR_LANES(e, count) for (int e = INIT_LANE; e < (count); e += INIT_LANES)
#define INIT_LANE0 if (INIT_LANE == 0)

// CorbInitResult::status
#define INIT_OK 0
#define INIT_NO_MODEL 1
#define INIT_H_DEGENERATE 2
#define INIT_AMBIGUOUS 3
#define INIT_FEW_POINTS 4
#define INIT_LOW_PARALLAX 5

// one entry of mvMatches12 with both keys' coordinates
struct InitMatch { float u1, v1, u2, v2; int i1, i2; };
// one problem: Normalize (:749-795) of both key sets as (meanX, meanY, sX, sY), mK
struct InitProb { int N, n1, match_off, pad; float fx, fy, cx, cy; float nrm1[4], nrm2[4]; };
// CorbInitResult, field for field
struct InitResult {
    int status, model, n_matches; float score_h, score_f, rh; int best_it_h, best_it_f; float H21[9], F21[9]; int n_inliers;
    int n_good[8]; float cos_parallax[8], parallax[8]; int best_hypothesis, second_best_good; float R21[9], t21[3]; int n_triangulated;
};
// what the select step leaves for CheckRT: the motion hypotheses in the source's order
struct InitSel { int n_hyp, best_it; float R[8][9], t[8][3]; };
struct InitDev {
    int n_problems, max_iterations, words, cap1, p3d_stride, flags_stride, min_triangulated;   // words = 64-match mask words per hypothesis, cap1 >= every n1
    float sigma, min_parallax, cos_thr_f, cos_thr_h;    // parallax > min_parallax <=> -1 <= c <= cos_thr_f (:525), parallax >= min_parallax <=> -1 <= c <= cos_thr_h (:721)
    const InitProb* prob; const InitMatch* match; const int* rand_values;      // [P], all problems' matches, [P][its][8]
    float* scores; float* hyp_m; unsigned long long* mask;                     // [P][its][2], [P][its][2][9], [P][its][2][words]
    InitSel* sel;                                                              // [P]
    float* cand_p3d; unsigned char* cand_good;                                 // [P][8][cap1 * 3], [P][8][cap1]: vP3Di, vbTriangulatedi
    float* cand_cos; unsigned char* cand_pushed;                               // [P][8][words * 64]: cosParallax of match i, whether it went into vCosParallax
    InitResult* res; float* p3d; unsigned char* tri; unsigned char* inl_h; unsigned char* inl_f;   // outputs (inl_h, inl_f may be NULL)
};

// ---- small matrices ----
INIT_HD void init_mul3(const float* A, const float* B, float* C)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += (double)A[3 * i + k] * (double)B[3 * k + j];
            C[3 * i + j] = (float)s;
        }
}
INIT_HD void init_transpose3(const float* A, float* At) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) At[3 * i + j] = A[3 * j + i]; }
INIT_HD double init_det3(const float* M)
{
    const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
    return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
}
INIT_HD void init_inv3(const float* M, float* Mi)
{
    const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
    const double det = init_det3(M);
    if (det == 0) { for (int k = 0; k < 9; k++) Mi[k] = 0.f; return; }
    const double r = 1.0 / det;
    Mi[0] = (float)((e * i - f * h) * r); Mi[1] = (float)((c * h - b * i) * r); Mi[2] = (float)((b * f - c * e) * r);
    Mi[3] = (float)((f * g - d * i) * r); Mi[4] = (float)((a * i - c * g) * r); Mi[5] = (float)((c * d - a * f) * r);
    Mi[6] = (float)((d * h - e * g) * r); Mi[7] = (float)((b * g - a * h) * r); Mi[8] = (float)((a * e - b * d) * r);
}
INIT_HD void init_K(const InitProb& P, float* K) { K[0] = P.fx; K[1] = 0.f; K[2] = P.cx; K[3] = 0.f; K[4] = P.fy; K[5] = P.cy; K[6] = 0.f; K[7] = 0.f; K[8] = 1.f; }
// T of Normalize (:790-794) from (meanX, meanY, sX, sY)
INIT_HD void init_T(const float* n, float* T)
{
    T[0] = n[2]; T[1] = 0.f; T[2] = -n[0] * n[2]; T[3] = 0.f; T[4] = n[3]; T[5] = -n[1] * n[3]; T[6] = 0.f; T[7] = 0.f; T[8] = 1.f;
}

// descending order of key[0..n), the lower index first among equals (pnp_order_desc's text)
INIT_HD void init_order_desc(const double* key, int n, int* order)
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
// one-sided (Hestenes) Jacobi on the columns of the m x n A (row-major, becomes U W), V from I; w = column norms, order = descending w.  pnp_hestenes' arithmetic;
// entered by all lanes: every lane forms the three sums of a pair (rows ascending), lane k rotates row k of A or row k - m of V.
INIT_HD void init_hestenes(double* A, double* V, double* w, int* order, int m, int n)
{
    INIT_FOR_LANES(e, n * n) V[e] = (e / n == e % n) ? 1.0 : 0.0;
    INIT_SYNC();
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int k = 0; k < m; k++) { const double ap = A[k * n + p], aq = A[k * n + q]; alpha += ap * ap; beta += aq * aq; gamma += ap * aq; }
                if (!(fabs(gamma) > 1e-15 * sqrt(alpha * beta))) continue;             // (the same for every lane)
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                INIT_SYNC();
                INIT_FOR_LANES(k, m + n) {
                    double* row = k < m ? A + k * n : V + (k - m) * n;
                    const double up = row[p], uq = row[q];
                    row[p] = c * up - s * uq; row[q] = s * up + c * uq;
                }
                INIT_SYNC();
            }
        if (!rotated) break;
    }
    INIT_FOR_LANES(j, n) { double s = 0; for (int k = 0; k < m; k++) s += A[k * n + j] * A[k * n + j]; w[j] = sqrt(s); }
    INIT_SYNC();
    INIT_LANE0 init_order_desc(w, n, order);
    INIT_SYNC();
}

// the LDS work area of one decomposition
struct InitSvdWork { double A[144], V[81], w[9]; int order[9]; };

// cv::SVD::compute of a float 3 x 3: U (columns), w, Vt (rows) in descending order, rounded to float once.  u_k = a_k / w_k; a smallest singular value that is not
// above 2^-51 sum_j w_j leaves the cross product of the other two columns (pnp_estimate_R_and_t's rule), two such leave NaN.  Entered by all lanes; the outputs are
// written by lane 0 and ordered behind a sync.
INIT_HD void init_svd3(const float* M, InitSvdWork& S, float* U, float* w, float* Vt)
{
    INIT_SYNC();
    INIT_FOR_LANES(e, 9) S.A[e] = (double)M[e];
    INIT_SYNC();
    init_hestenes(S.A, S.V, S.w, S.order, 3, 3);
    INIT_LANE0 {
        const int o0 = S.order[0], o1 = S.order[1], o2 = S.order[2];
        const double thr = 4.440892098500626e-16 * (S.w[0] + S.w[1] + S.w[2]);
        double u[3][3];
        if (!(S.w[o1] > thr)) { for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) u[i][k] = __builtin_nan(""); }
        else {
            for (int i = 0; i < 3; i++) { u[i][0] = S.A[i * 3 + o0] / S.w[o0]; u[i][1] = S.A[i * 3 + o1] / S.w[o1]; }
            if (S.w[o2] > thr) { for (int i = 0; i < 3; i++) u[i][2] = S.A[i * 3 + o2] / S.w[o2]; }
            else {
                u[0][2] = u[1][0] * u[2][1] - u[2][0] * u[1][1]; u[1][2] = u[2][0] * u[0][1] - u[0][0] * u[2][1]; u[2][2] = u[0][0] * u[1][1] - u[1][0] * u[0][1];
            }
        }
        for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) U[3 * i + k] = (float)u[i][k];
        w[0] = (float)S.w[o0]; w[1] = (float)S.w[o1]; w[2] = (float)S.w[o2];
        for (int k = 0; k < 3; k++) { const int o = S.order[k]; for (int j = 0; j < 3; j++) Vt[3 * k + j] = (float)S.V[j * 3 + o]; }
    }
    INIT_SYNC();
}

// ---- CheckHomography (:337-385) / CheckFundamental (:413-465) for one match: the two terms of the score, whether each is added, the inlier bit ----
INIT_HD bool init_check_h(const float* h, const float* hi, const InitMatch& m, float invSigmaSquare, float* t1, bool* a1, float* t2, bool* a2)
{
    const float th = 5.991f;
    const float u1 = m.u1, v1 = m.v1, u2 = m.u2, v2 = m.v2;
    bool bIn = true;
    const float w2in1inv = (float)(1.0 / (double)(hi[6] * u2 + hi[7] * v2 + hi[8]));
    const float u2in1 = (hi[0] * u2 + hi[1] * v2 + hi[2]) * w2in1inv;
    const float v2in1 = (hi[3] * u2 + hi[4] * v2 + hi[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = false; *a1 = false; } else *a1 = true;
    *t1 = th - chiSquare1;
    const float w1in2inv = (float)(1.0 / (double)(h[6] * u1 + h[7] * v1 + h[8]));
    const float u1in2 = (h[0] * u1 + h[1] * v1 + h[2]) * w1in2inv;
    const float v1in2 = (h[3] * u1 + h[4] * v1 + h[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = false; *a2 = false; } else *a2 = true;
    *t2 = th - chiSquare2;
    return bIn;
}
INIT_HD bool init_check_f(const float* f, const InitMatch& m, float invSigmaSquare, float* t1, bool* a1, float* t2, bool* a2)
{
    const float th = 3.841f, thScore = 5.991f;
    const float u1 = m.u1, v1 = m.v1, u2 = m.u2, v2 = m.v2;
    bool bIn = true;
    const float a2_ = f[0] * u1 + f[1] * v1 + f[2];
    const float b2 = f[3] * u1 + f[4] * v1 + f[5];
    const float c2 = f[6] * u1 + f[7] * v1 + f[8];
    const float num2 = a2_ * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2_ * a2_ + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = false; *a1 = false; } else *a1 = true;
    *t1 = thScore - chiSquare1;
    const float a1_ = f[0] * u2 + f[3] * v2 + f[6];
    const float b1 = f[1] * u2 + f[4] * v2 + f[7];
    const float c1 = f[2] * u2 + f[5] * v2 + f[8];
    const float num1 = a1_ * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1_ * a1_ + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = false; *a2 = false; } else *a2 = true;
    *t2 = thScore - chiSquare2;
    return bIn;
}

// ---- one hypothesis: iteration `it` of FindHomography (model 0, :148-171) or FindFundamental (model 1, :199-222) of problem c ----
struct InitHypWork { InitSvdWork S; int idx[8]; float M[9], Mi[9], U[9], w[3], Vt[9]; float t1[64], t2[64]; unsigned long long b1, b2; float score; };

INIT_HD void init_hypothesis_body(const InitDev& d, int c, int it, int model, InitHypWork& W)
{
    const InitProb& P = d.prob[c];
    const InitMatch* match = d.match + P.match_off;
    const int N = P.N;
    const size_t h = ((size_t)c * d.max_iterations + it) * 2 + model;
    INIT_LANE0 {
        ransac_draw<8>(d.rand_values + ((size_t)c * d.max_iterations + it) * 8, 8, N, W.idx);
        for (int k = 0; k < 8; k++) W.idx[k] = W.idx[k] < 0 ? 0 : (W.idx[k] > N - 1 ? N - 1 : W.idx[k]);      // (no effect on draws in [0, 2^31))
    }
    INIT_SYNC();
    // ComputeH21 (:226-266): A is 16 x 9; ComputeF21 (:268-303): A is 8 x 9
    const int m = model == 0 ? 16 : 8;
    INIT_FOR_LANES(j, 8) {
        const InitMatch& mt = match[W.idx[j]];
        const float u1 = (mt.u1 - P.nrm1[0]) * P.nrm1[2], v1 = (mt.v1 - P.nrm1[1]) * P.nrm1[3];       // vPn1, vPn2 (:771-787)
        const float u2 = (mt.u2 - P.nrm2[0]) * P.nrm2[2], v2 = (mt.v2 - P.nrm2[1]) * P.nrm2[3];
        if (model == 0) {
            double* r0 = W.S.A + 18 * j; double* r1 = r0 + 9;
            r0[0] = 0.0; r0[1] = 0.0; r0[2] = 0.0; r0[3] = (double)(-u1); r0[4] = (double)(-v1); r0[5] = -1.0;
            r0[6] = (double)(v2 * u1); r0[7] = (double)(v2 * v1); r0[8] = (double)v2;
            r1[0] = (double)u1; r1[1] = (double)v1; r1[2] = 1.0; r1[3] = 0.0; r1[4] = 0.0; r1[5] = 0.0;
            r1[6] = (double)(-u2 * u1); r1[7] = (double)(-u2 * v1); r1[8] = (double)(-u2);
        } else {
            double* r = W.S.A + 9 * j;
            r[0] = (double)(u2 * u1); r[1] = (double)(u2 * v1); r[2] = (double)u2; r[3] = (double)(v2 * u1); r[4] = (double)(v2 * v1); r[5] = (double)v2;
            r[6] = (double)u1; r[7] = (double)v1; r[8] = 1.0;
        }
    }
    INIT_SYNC();
    init_hestenes(W.S.A, W.S.V, W.S.w, W.S.order, m, 9);
    INIT_LANE0 { const int o = W.S.order[8]; for (int k = 0; k < 9; k++) W.M[k] = (float)W.S.V[k * 9 + o]; }     // vt.row(8)
    INIT_SYNC();
    if (model == 1) {                                                  // the rank-2 Fn = u diag(w0, w1, 0) vt (:298-302)
        init_svd3(W.M, W.S, W.U, W.w, W.Vt);
        INIT_LANE0 {
            const float D[9] = {W.w[0], 0.f, 0.f, 0.f, W.w[1], 0.f, 0.f, 0.f, 0.f};
            float UD[9];
            init_mul3(W.U, D, UD); init_mul3(UD, W.Vt, W.M);
        }
        INIT_SYNC();
    }
    INIT_LANE0 {
        float T1[9], T2[9], L[9], LM[9];
        init_T(P.nrm1, T1); init_T(P.nrm2, T2);
        if (model == 0) init_inv3(T2, L); else init_transpose3(T2, L);                 // T2inv * Hn * T1 (:160), T2t * Fn * T1 (:212)
        init_mul3(L, W.M, LM); init_mul3(LM, T1, W.M);
        if (model == 0) init_inv3(W.M, W.Mi); else for (int k = 0; k < 9; k++) W.Mi[k] = 0.f;      // H12i (:161)
        for (int k = 0; k < 9; k++) d.hyp_m[h * 9 + k] = W.M[k];
        W.score = 0.f;
    }
    INIT_SYNC();
    float M[9], Mi[9];
    for (int k = 0; k < 9; k++) { M[k] = W.M[k]; Mi[k] = W.Mi[k]; }
    const float invSigmaSquare = (float)(1.0 / (double)(d.sigma * d.sigma));
    unsigned long long* mask = d.mask + h * d.words;
    // the matches in chunks of one per lane; the score is summed by one lane in ascending match order
    for (int base = 0; base < N; base += INIT_LANES) {
        const int i = base + INIT_LANE;
        float t1 = 0.f, t2 = 0.f; bool a1 = false, a2 = false, in = false;
        if (i < N) in = model == 0 ? init_check_h(M, Mi, match[i], invSigmaSquare, &t1, &a1, &t2, &a2) : init_check_f(M, match[i], invSigmaSquare, &t1, &a1, &t2, &a2);
        const unsigned long long bin = INIT_BALLOT(in), b1 = INIT_BALLOT(a1), b2 = INIT_BALLOT(a2);
        W.t1[INIT_LANE] = t1; W.t2[INIT_LANE] = t2;
        INIT_SYNC();
        INIT_LANE0 {
            if ((base & 63) == 0) mask[base >> 6] = 0ull;
            mask[base >> 6] |= bin << (base & 63);
            float score = W.score;
            const int cnt = N - base < INIT_LANES ? N - base : INIT_LANES;
            for (int k = 0; k < cnt; k++) {
                if ((b1 >> k) & 1ull) score += W.t1[k];
                if ((b2 >> k) & 1ull) score += W.t2[k];
            }
            W.score = score;
        }
        INIT_SYNC();
    }
    INIT_LANE0 d.scores[h] = W.score;
}

// ---- select: the winners of both RANSACs (:148-171, :199-222), RH and the model (:112-118), then DecomposeE (:909-929) or the 8 hypotheses of :584-686 ----
struct InitSelWork { InitSvdWork S; float best[2][64]; int best_it[2][64]; float E[9], U[9], w[3], Vt[9]; int status, model, it[2]; };

INIT_HD void init_select_body(const InitDev& d, int c, InitSelWork& W)
{
    const InitProb& P = d.prob[c];
    InitResult& R = d.res[c]; InitSel& sel = d.sel[c];
    const int its = d.max_iterations, N = P.N;
    const float* scores = d.scores + (size_t)c * its * 2;
    // the first maximum of the positive scores (the source's strict >; NaN is never greater)
    for (int model = 0; model < 2; model++)
        INIT_FOR_LANES(l, 64) {
            float best = 0.f; int bi = -1;
            for (int it = l; it < its; it += 64) { const float s = scores[2 * it + model]; if (s > best) { best = s; bi = it; } }
            W.best[model][l] = best; W.best_it[model][l] = bi;
        }
    INIT_SYNC();
    INIT_LANE0 {
        for (int model = 0; model < 2; model++) {
            float best = 0.f; int bi = -1;
            for (int l = 0; l < 64; l++) {
                const float s = W.best[model][l]; const int i = W.best_it[model][l];
                if (i >= 0 && (s > best || (s == best && i < bi))) { best = s; bi = i; }
            }
            W.it[model] = bi;
            if (model == 0) R.score_h = best; else R.score_f = best;
        }
        R.n_matches = N; R.best_it_h = W.it[0]; R.best_it_f = W.it[1];
        const float RH = R.score_h / (R.score_h + R.score_f);                          // :112
        R.rh = RH;
        const int model = (double)RH > 0.40 ? 0 : 1;
        R.model = model; W.model = model;
        for (int k = 0; k < 9; k++) {
            R.H21[k] = W.it[0] >= 0 ? d.hyp_m[(((size_t)c * its + W.it[0]) * 2) * 9 + k] : 0.f;
            R.F21[k] = W.it[1] >= 0 ? d.hyp_m[(((size_t)c * its + W.it[1]) * 2 + 1) * 9 + k] : 0.f;
        }
        W.status = (RH != RH || W.it[model] < 0) ? INIT_NO_MODEL : INIT_OK;
        for (int k = 0; k < 8; k++) { R.n_good[k] = 0; R.cos_parallax[k] = 0.f; R.parallax[k] = 0.f; }
        R.best_hypothesis = -1; R.second_best_good = 0; R.n_triangulated = 0; R.n_inliers = 0;
        for (int k = 0; k < 9; k++) R.R21[k] = 0.f;
        for (int k = 0; k < 3; k++) R.t21[k] = 0.f;
        sel.n_hyp = 0; sel.best_it = W.it[model];
    }
    INIT_SYNC();
    // vbMatchesInliersH / F, one byte per match
    for (int model = 0; model < 2; model++) {
        unsigned char* out = model == 0 ? d.inl_h : d.inl_f;
        if (!out) continue;
        const int bi = W.it[model];
        const unsigned long long* mask = d.mask + (((size_t)c * its + (bi < 0 ? 0 : bi)) * 2 + model) * d.words;
        INIT_FOR_LANES(i, N) out[(size_t)c * d.flags_stride + i] = bi >= 0 ? (unsigned char)((mask[i >> 6] >> (i & 63)) & 1ull) : 0;
    }
    const int model = W.model;
    if (W.status != INIT_OK) { INIT_LANE0 R.status = W.status; return; }                // (the same for every lane)
    const unsigned long long* mask = d.mask + (((size_t)c * its + W.it[model]) * 2 + model) * d.words;
    INIT_LANE0 {
        int n = 0;
        for (int w = 0; w < (N + 63) / 64; w++) n += __builtin_popcountll(mask[w]);
        R.n_inliers = n;
        float K[9], L[9], LM[9];
        init_K(P, K);
        if (model == 1) init_transpose3(K, L); else init_inv3(K, L);                    // E21 = K.t() * F21 * K (:479), A = invK * H21 * K (:584-585)
        init_mul3(L, model == 1 ? R.F21 : R.H21, LM); init_mul3(LM, K, W.E);
    }
    init_svd3(W.E, W.S, W.U, W.w, W.Vt);
    INIT_LANE0 {
        const float* U = W.U; const float* Vt = W.Vt;
        if (model == 1) {
            // DecomposeE: t = u.col(2) / norm, R1 = u W vt, R2 = u W^T vt, each negated if its determinant is negative; then (R1, t), (R2, t), (R1, -t), (R2, -t)
            float t[3] = {U[2], U[5], U[8]};
            const double nt = sqrt((double)t[0] * t[0] + (double)t[1] * t[1] + (double)t[2] * t[2]);
            for (int k = 0; k < 3; k++) t[k] = (float)((double)t[k] / nt);
            const float Wm[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
            float Wt[9], UW[9], R1[9], R2[9];
            init_transpose3(Wm, Wt);
            init_mul3(U, Wm, UW); init_mul3(UW, Vt, R1);
            if (init_det3(R1) < 0) for (int k = 0; k < 9; k++) R1[k] = -R1[k];
            init_mul3(U, Wt, UW); init_mul3(UW, Vt, R2);
            if (init_det3(R2) < 0) for (int k = 0; k < 9; k++) R2[k] = -R2[k];
            for (int hy = 0; hy < 4; hy++) {
                for (int k = 0; k < 9; k++) sel.R[hy][k] = (hy & 1) ? R2[k] : R1[k];
                for (int k = 0; k < 3; k++) sel.t[hy][k] = hy < 2 ? t[k] : -t[k];
            }
            sel.n_hyp = 4;
        } else {
            const float s = (float)(init_det3(U) * init_det3(Vt));                      // :591
            const float d1 = W.w[0], d2 = W.w[1], d3 = W.w[2];
            if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) W.status = INIT_H_DEGENERATE;      // :597
            else {
                const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
                const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
                const float x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
                const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
                const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
                const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
                const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
                const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
                const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
                for (int hy = 0; hy < 8; hy++) {
                    const int i = hy & 3;
                    float Rp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tp[3];
                    if (hy < 4) { Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta; tp[0] = x1[i]; tp[1] = 0.f; tp[2] = -x3[i]; }
                    else { Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1.f; Rp[6] = sphi[i]; Rp[8] = -cphi; tp[0] = x1[i]; tp[1] = 0.f; tp[2] = x3[i]; }
                    const float f = hy < 4 ? d1 - d3 : d1 + d3;
                    for (int k = 0; k < 3; k++) tp[k] = tp[k] * f;                      // tp *= d1 -+ d3
                    // R = s * U * Rp * Vt: the scale goes into the first product before its rounding
                    float SURp[9];
                    for (int a = 0; a < 3; a++)
                        for (int b = 0; b < 3; b++) {
                            double acc = 0.0;
                            for (int k = 0; k < 3; k++) acc += (double)U[3 * a + k] * (double)Rp[3 * k + b];
                            SURp[3 * a + b] = (float)((double)s * acc);
                        }
                    init_mul3(SURp, Vt, sel.R[hy]);
                    float t[3];
                    for (int a = 0; a < 3; a++) { double acc = 0.0; for (int k = 0; k < 3; k++) acc += (double)U[3 * a + k] * (double)tp[k]; t[a] = (float)acc; }
                    const double nt = sqrt((double)t[0] * t[0] + (double)t[1] * t[1] + (double)t[2] * t[2]);
                    for (int k = 0; k < 3; k++) sel.t[hy][k] = (float)((double)t[k] / nt);
                }
                sel.n_hyp = 8;
            }
        }
        R.status = W.status;
    }
}

// ---- CheckRT (:798-907) of motion hypothesis hy of problem c ----
// Triangulate (:734-747): the null vector of the float 4 x 4 A by the same one-sided Jacobi in registers (np_svd_null's arithmetic; the smallest singular value is
// the last of the descending order, the higher index among equals)
INIT_HD void init_svd_null4(const float* Af, float* v4)
{
    double U[4][4], V[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) { U[i][j] = (double)Af[i * 4 + j]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; p++) {
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) { alpha += U[k][p] * U[k][p]; beta += U[k][q] * U[k][q]; gamma += U[k][p] * U[k][q]; }
                if (fabs(gamma) > 1e-15 * sqrt(alpha * beta)) {
                    rotated = true;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const double up = U[k][p], uq = U[k][q]; U[k][p] = c * up - s * uq; U[k][q] = s * up + c * uq;
                        const double vp = V[k][p], vq = V[k][q]; V[k][p] = c * vp - s * vq; V[k][q] = s * vp + c * vq;
                    }
                }
            }
        }
        if (!rotated) break;
    }
    double w[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double n2 = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) n2 += U[k][j] * U[k][j];
        w[j] = sqrt(n2);
    }
    // the last of the descending order: no other column is strictly smaller, and no later column is equal
    int jb = 0;
#pragma unroll
    for (int j = 1; j < 4; j++) if (!(w[j] > w[jb])) jb = j;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double v = V[i][0];
#pragma unroll
        for (int j = 1; j < 4; j++) if (j == jb) v = V[i][j];
        v4[i] = (float)v;
    }
}
INIT_HD bool init_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }
// rank order of vCosParallax: value, then position; NaN last
INIT_HD bool init_cos_before(float a, int ia, float b, int ib)
{
    const bool na = a != a, nb = b != b;
    if (na || nb) return na == nb ? ia < ib : nb;
    return a < b || (a == b && ia < ib);
}

struct InitRtWork { int nGood; };

INIT_HD void init_checkrt_body(const InitDev& d, int c, int hy, InitRtWork& W)
{
    const InitProb& P = d.prob[c];
    const InitSel& sel = d.sel[c];
    if (hy >= sel.n_hyp) return;                                                        // (the same for every lane)
    InitResult& res = d.res[c];
    const InitMatch* match = d.match + P.match_off;
    const int N = P.N, capN = d.words * 64;
    const unsigned long long* mask = d.mask + (((size_t)c * d.max_iterations + sel.best_it) * 2 + res.model) * d.words;
    float* p3d = d.cand_p3d + ((size_t)c * 8 + hy) * d.cap1 * 3;
    unsigned char* good = d.cand_good + ((size_t)c * 8 + hy) * d.cap1;
    float* cosv = d.cand_cos + ((size_t)c * 8 + hy) * capN;
    unsigned char* pushed = d.cand_pushed + ((size_t)c * 8 + hy) * capN;
    INIT_LANE0 W.nGood = 0;
    INIT_SYNC();
    const float fx = P.fx, fy = P.fy, cx = P.cx, cy = P.cy;
    const float th2 = (float)(4.0 * (double)(d.sigma * d.sigma));                       // 4.0 * mSigma2 (:494)
    float R[9], t[3], K[9], P2[12], O2[3];
    for (int k = 0; k < 9; k++) R[k] = sel.R[hy][k];
    for (int k = 0; k < 3; k++) t[k] = sel.t[hy][k];
    init_K(P, K);
    // P1 = K [I | 0]; P2 = K [R | t] (:821-824); O2 = -R^T t (:826)
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += (double)K[3 * i + k] * (double)(j < 3 ? R[3 * k + j] : t[k]);
            P2[4 * i + j] = (float)s;
        }
    for (int i = 0; i < 3; i++) { double s = 0.0; for (int k = 0; k < 3; k++) s += (double)(-R[3 * k + i]) * (double)t[k]; O2[i] = (float)s; }
    const float P1[12] = {K[0], K[1], K[2], 0.f, K[3], K[4], K[5], 0.f, K[6], K[7], K[8], 0.f};
    int mine = 0;
    INIT_FOR_LANES(i, N) {
        pushed[i] = 0;
        if (!((mask[i >> 6] >> (i & 63)) & 1ull)) continue;
        const InitMatch& m = match[i];
        float A[16], v[4];
        for (int k = 0; k < 4; k++) {
            A[0 * 4 + k] = m.u1 * P1[2 * 4 + k] - P1[0 * 4 + k];
            A[1 * 4 + k] = m.v1 * P1[2 * 4 + k] - P1[1 * 4 + k];
            A[2 * 4 + k] = m.u2 * P2[2 * 4 + k] - P2[0 * 4 + k];
            A[3 * 4 + k] = m.v2 * P2[2 * 4 + k] - P2[1 * 4 + k];
        }
        init_svd_null4(A, v);
        const float X[3] = {v[0] / v[3], v[1] / v[3], v[2] / v[3]};
        if (!init_finite(X[0]) || !init_finite(X[1]) || !init_finite(X[2])) continue;   // (vbGood is false already)
        const float n2[3] = {X[0] - O2[0], X[1] - O2[1], X[2] - O2[2]};
        const float dist1 = (float)sqrt((double)X[0] * X[0] + (double)X[1] * X[1] + (double)X[2] * X[2]);
        const float dist2 = (float)sqrt((double)n2[0] * n2[0] + (double)n2[1] * n2[1] + (double)n2[2] * n2[2]);
        const double dot = (double)X[0] * n2[0] + (double)X[1] * n2[1] + (double)X[2] * n2[2];
        const float cosParallax = (float)(dot / (double)(dist1 * dist2));
        if (X[2] <= 0 && (double)cosParallax < 0.99998) continue;
        float X2[3];
        for (int a = 0; a < 3; a++) { double s = 0.0; for (int k = 0; k < 3; k++) s += (double)R[3 * a + k] * (double)X[k]; X2[a] = (float)(s + (double)t[a]); }
        if (X2[2] <= 0 && (double)cosParallax < 0.99998) continue;
        const float invZ1 = (float)(1.0 / (double)X[2]);
        const float im1x = fx * X[0] * invZ1 + cx, im1y = fy * X[1] * invZ1 + cy;
        const float squareError1 = (im1x - m.u1) * (im1x - m.u1) + (im1y - m.v1) * (im1y - m.v1);
        if (squareError1 > th2) continue;
        const float invZ2 = (float)(1.0 / (double)X2[2]);
        const float im2x = fx * X2[0] * invZ2 + cx, im2y = fy * X2[1] * invZ2 + cy;
        const float squareError2 = (im2x - m.u2) * (im2x - m.u2) + (im2y - m.v2) * (im2y - m.v2);
        if (squareError2 > th2) continue;
        cosv[i] = cosParallax; pushed[i] = 1;
        p3d[3 * m.i1] = X[0]; p3d[3 * m.i1 + 1] = X[1]; p3d[3 * m.i1 + 2] = X[2];
        mine++;
        if ((double)cosParallax < 0.99998) good[m.i1] = 1;
    }
    if (mine) INIT_SHARED_ADD(&W.nGood, mine);
    INIT_SYNC();
    const int nGood = W.nGood;
    INIT_LANE0 { res.n_good[hy] = nGood; if (nGood == 0) res.cos_parallax[hy] = 1.f; }  // parallax = 0 (:904) = the parallax of a cosine of 1
    if (nGood == 0) return;
    // vCosParallax[min(50, size - 1)] after the sort (:898-901), by rank
    const int want = nGood - 1 < 50 ? nGood - 1 : 50;
    INIT_FOR_LANES(i, N) {
        if (!pushed[i]) continue;
        const float ci = cosv[i];
        int rank = 0;
        for (int j = 0; j < N; j++) if (pushed[j] && init_cos_before(cosv[j], j, ci, i)) rank++;
        if (rank == want) res.cos_parallax[hy] = ci;
    }
}

// ---- the decision of ReconstructF (:499-569) or ReconstructH (:689-731) on the cosines, then vP3D and vbTriangulated of the winner ----
struct InitDecWork { int status, best, n_tri; };

INIT_HD bool init_parallax_passes(float c, float thr) { return c >= -1.f && c <= thr; }

INIT_HD void init_decide_body(const InitDev& d, int c, InitDecWork& W)
{
    const InitProb& P = d.prob[c];
    const InitSel& sel = d.sel[c];
    InitResult& R = d.res[c];
    if (R.status != INIT_OK) return;                                                    // (the same for every lane: written by the select step)
    INIT_LANE0 {
        const int N = R.n_inliers;
        int bestGood = 0, secondBestGood = 0, best = -1;
        for (int i = 0; i < sel.n_hyp; i++) {
            const int nGood = R.n_good[i];
            if (nGood > bestGood) { secondBestGood = bestGood; bestGood = nGood; best = i; }
            else if (nGood > secondBestGood) secondBestGood = nGood;
        }
        int status = INIT_OK;
        if (R.model == 1) {
            const int maxGood = bestGood;
            if (best < 0) best = 0;                                                     // maxGood == nGood1 == 0 (:523)
            int nMinGood = (int)(0.9 * N); if (nMinGood < d.min_triangulated) nMinGood = d.min_triangulated;
            int nsimilar = 0;
            for (int i = 0; i < 4; i++) if ((double)R.n_good[i] > 0.7 * maxGood) nsimilar++;
            if (maxGood < nMinGood) status = INIT_FEW_POINTS;
            else if (nsimilar > 1) status = INIT_AMBIGUOUS;
            else if (!init_parallax_passes(R.cos_parallax[best], d.cos_thr_f)) status = INIT_LOW_PARALLAX;     // the else-if chain: only the first maximum is tried
        } else {
            const bool par = best < 0 ? -1.f >= d.min_parallax : init_parallax_passes(R.cos_parallax[best], d.cos_thr_h);
            if (!par) status = INIT_LOW_PARALLAX;                                       // several failing tests of :721: parallax, second best, few points
            else if (!((double)secondBestGood < 0.75 * bestGood)) status = INIT_AMBIGUOUS;
            else if (!(bestGood > d.min_triangulated && (double)bestGood > 0.9 * N)) status = INIT_FEW_POINTS;
        }
        R.best_hypothesis = best; R.second_best_good = secondBestGood; R.status = status;
        if (status == INIT_OK) {
            for (int k = 0; k < 9; k++) R.R21[k] = sel.R[best][k];
            for (int k = 0; k < 3; k++) R.t21[k] = sel.t[best][k];
        }
        W.status = status; W.best = best; W.n_tri = 0;
    }
    INIT_SYNC();
    if (W.status != INIT_OK) return;
    const float* p3d = d.cand_p3d + ((size_t)c * 8 + W.best) * d.cap1 * 3;
    const unsigned char* good = d.cand_good + ((size_t)c * 8 + W.best) * d.cap1;
    int mine = 0;
    INIT_FOR_LANES(i, P.n1) {
        for (int k = 0; k < 3; k++) d.p3d[((size_t)c * d.p3d_stride + i) * 3 + k] = p3d[3 * i + k];
        d.tri[(size_t)c * d.p3d_stride + i] = good[i];
        mine += good[i];
    }
    if (mine) INIT_SHARED_ADD(&W.n_tri, mine);
    INIT_SYNC();
    INIT_LANE0 R.n_triangulated = W.n_tri;
}

// ---- the call's set-up on the host ----
// Normalize (:749-795): float sums in ascending index order -> (meanX, meanY, sX, sY).  x, y at a stride of `stride` floats.
inline void init_normalize(const float* xy, int stride, int n, float* out)
{
    float meanX = 0, meanY = 0;
    for (int i = 0; i < n; i++) { meanX += xy[(size_t)i * stride]; meanY += xy[(size_t)i * stride + 1]; }
    meanX = meanX / n; meanY = meanY / n;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < n; i++) { meanDevX += fabsf(xy[(size_t)i * stride] - meanX); meanDevY += fabsf(xy[(size_t)i * stride + 1] - meanY); }
    meanDevX = meanDevX / n; meanDevY = meanDevY / n;
    out[0] = meanX; out[1] = meanY; out[2] = (float)(1.0 / (double)meanDevX); out[3] = (float)(1.0 / (double)meanDevY);
}
// parallax = float(acos((double)c) * 180 / pi) (:901)
inline float init_parallax(float c) { return (float)(acos((double)c) * 180 / 3.1415926535897932384626433832795); }
// the largest c in [-1, 1] whose parallax is > min_parallax (strict) or >= min_parallax, by bisection over the float bit patterns (the parallax does not increase with
// c); -2 if there is none
inline float init_cos_threshold(float min_parallax, bool strict)
{
    auto key = [](float f) { uint32_t u; memcpy(&u, &f, 4); return (u & 0x80000000u) ? (int64_t)0x80000000u - (int64_t)u : (int64_t)u; };   // increasing with f, -0 = +0
    auto val = [](int64_t k) { uint32_t u = k < 0 ? (uint32_t)((int64_t)0x80000000u - k) : (uint32_t)k; float f; memcpy(&f, &u, 4); return f; };
    auto ok = [&](float c) { const float p = init_parallax(c); return strict ? p > min_parallax : p >= min_parallax; };
    int64_t lo = key(-1.f), hi = key(1.f);
    if (!ok(val(lo))) return -2.f;
    if (ok(val(hi))) return 1.f;
    while (hi - lo > 1) { const int64_t mid = lo + (hi - lo) / 2; if (ok(val(mid))) lo = mid; else hi = mid; }
    return val(lo);
}
// the four steps over every workgroup of a call, one after the other: what the kernels compute, on one core.  The candidate arrays, p3d and tri are zero on entry.
inline void init_run_serial(const InitDev& d)
{
    static InitHypWork hw; static InitSelWork sw; InitRtWork rw; InitDecWork dw;
    for (int c = 0; c < d.n_problems; c++) {
        for (int it = 0; it < d.max_iterations; it++) for (int model = 0; model < 2; model++) init_hypothesis_body(d, c, it, model, hw);
        init_select_body(d, c, sw);
        for (int hy = 0; hy < 8; hy++) init_checkrt_body(d, c, hy, rw);
        init_decide_body(d, c, dw);
    }
}
// the reported parallax of the hypotheses CheckRT has run on, from the returned cosines
inline void init_fill_parallax(InitResult& r)
{
    const int n = (r.status == INIT_NO_MODEL || r.status == INIT_H_DEGENERATE) ? 0 : (r.model == 1 ? 4 : 8);
    for (int k = 0; k < 8; k++) r.parallax[k] = k < n ? init_parallax(r.cos_parallax[k]) : 0.f;
}

// sim3_ransac_kernels.hip -- the Sim3Solver RANSAC of LoopClosing::ComputeSim3 (C/src/Sim3Solver.cc) for gfx950:
//   sim3_ransac_prepare_kernel    : the constructor's per-correspondence work (:62-109) -- camera coordinates, both FromCameraToImage projections, the two integer
//                                   thresholds; on records also the filter (:64-79) through the map's id index and the observation lists
//   sim3_ransac_compact_kernel    : record route: the accepted features of keyframe 1 in ascending order (mvnIndices1), after the scan of device_util.hip
//   sim3_ransac_hypothesis_kernel : one wavefront per (candidate, iteration): the three draws (:163-177), ComputeSim3 (:226-337) wave-uniform in registers, then
//                                   CheckInliers (:340-364) with the lanes striding over the correspondences -- a ballot per 64, one 64-bit mask word each
// Arithmetic: the reference's expressions as non-fused IEEE operations with the C++ types of the source (-ffp-contract=off); cv::gemm = double accumulation and one
// rounding, Mat::dot = a double sum, cv::eigen = a cyclic Jacobi iteration in FP64, atan2 + cv::Rodrigues = the same rotation written algebraically in double
// (numerics contract; tests/sim3solver_reference.py restates every line).  A call is a few hundred to a few thousand waves and latency bound.
#include "sim3_ransac_internal.h"

namespace {

#define S3R_NAN __int_as_float(0x7FC00000)

// mvnMaxError: vector<size_t>::push_back(9.210 * sigmaSquare) -- double x float, truncated; compared as float err < (float)that integer (:87-88, :356)
__device__ __forceinline__ float s3r_threshold(float sigma2) { return (float)(unsigned long long)(9.210 * (double)sigma2); }
// one row of Rcw * X + tcw: cv::gemm, double accumulation, one rounding
__device__ __forceinline__ float s3r_row(const float* r, const float* X, float t)
{
    double s = (double)r[0] * (double)X[0];
    s = s + (double)r[1] * (double)X[1];
    s = s + (double)r[2] * (double)X[2];
    s = s + (double)t;
    return (float)s;
}
// FromCameraToImage / Project (:382-423): const float invz = 1 / z
__device__ __forceinline__ void s3r_project(const float* X, const float* K, float* uv)
{
    const float invz = 1.0f / X[2];
    const float x = X[0] * invz, y = X[1] * invz;
    uv[0] = K[0] * x + K[2]; uv[1] = K[1] * y + K[3];
}
__device__ __forceinline__ void s3r_intrinsics(const S3rDev& d, const S3rCand& c, float* K1, float* K2)
{
    if (d.kf1) {
        const KfHeader* h1 = reinterpret_cast<const KfHeader*>(d.kf1); const KfHeader* h2 = reinterpret_cast<const KfHeader*>(c.kf2);
        K1[0] = h1->m.fx; K1[1] = h1->m.fy; K1[2] = h1->m.cx; K1[3] = h1->m.cy;
        K2[0] = h2->m.fx; K2[1] = h2->m.fy; K2[2] = h2->m.cx; K2[3] = h2->m.cy;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) { K1[k] = c.K1[k]; K2[k] = c.K2[k]; }
    }
}
// MapPoint::GetIndexInKeyFrame through the record's observation list; -1 = the point does not observe the keyframe
__device__ __forceinline__ int s3r_index_in_keyframe(const char* rec, int max_obs, unsigned long long kf_id)
{
    const CorbMapPointRecord* h = reinterpret_cast<const CorbMapPointRecord*>(rec);
    const MpLayout L(max_obs);
    const unsigned long long* okf = reinterpret_cast<const unsigned long long*>(rec + L.obs_kf);
    const uint32_t* oidx = reinterpret_cast<const uint32_t*>(rec + L.obs_idx);
    const int n_obs = min(h->n_obs, max_obs);
    for (int k = 0; k < n_obs; k++) if (okf[k] == kf_id) return (int)oidx[k];
    return -1;
}

__global__ __launch_bounds__(256) void sim3_ransac_prepare_kernel(S3rDev d)
{
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    const S3rCand& cd = d.cand[c];
    if (i >= cd.n || i >= d.cap) return;
    const size_t e = (size_t)c * d.cap + i;
    float K1[4], K2[4]; s3r_intrinsics(d, cd, K1, K2);
    S3rCorr o;
    if (!d.kf1) {
        const float* r = d.in + 8 * ((size_t)cd.in_off + i);
#pragma unroll
        for (int k = 0; k < 3; k++) { o.x1[k] = r[k]; o.x2[k] = r[3 + k]; }
        o.th1 = s3r_threshold(r[6]); o.th2 = s3r_threshold(r[7]);
        s3r_project(o.x1, K1, o.p1); s3r_project(o.x2, K2, o.p2);
        d.set.corr[e] = o;
        return;
    }
    // the constructor's filter for feature i1 = i of keyframe 1 (:64-79)
    int ok = 0;
    const RecLayout L(d.F);
    const KfHeader* h1 = reinterpret_cast<const KfHeader*>(d.kf1); const KfHeader* h2 = reinterpret_cast<const KfHeader*>(cd.kf2);
    const unsigned long long id2 = d.matched12[e], id1 = reinterpret_cast<const unsigned long long*>(d.kf1 + L.mp_id)[i];
    if (id2 != CORB_NO_MAP_POINT && id1 != CORB_NO_MAP_POINT) {
        const int s1 = corb_idtab_find(d.idt, id1), s2 = corb_idtab_find(d.idt, id2);
        if (s1 >= 0 && s2 >= 0) {
            const char* r1 = d.mp_base + (size_t)s1 * d.mp_bytes; const char* r2 = d.mp_base + (size_t)s2 * d.mp_bytes;
            const CorbMapPointRecord* m1 = reinterpret_cast<const CorbMapPointRecord*>(r1); const CorbMapPointRecord* m2 = reinterpret_cast<const CorbMapPointRecord*>(r2);
            if (!(m1->flags & CORB_MP_BAD) && !(m2->flags & CORB_MP_BAD)) {
                const int idx1 = s3r_index_in_keyframe(r1, d.max_obs, h1->m.id), idx2 = s3r_index_in_keyframe(r2, d.max_obs, h2->m.id);
                if (idx1 >= 0 && idx1 < cd.n && idx2 >= 0 && idx2 < cd.n2) {
                    // kp1 = mvKeysUn[indexKF1], kp2 = mvKeysUn[indexKF2]; mvLevelSigma2 = scale^2 in float
                    const int o1 = min(max(reinterpret_cast<const CorbKeyPoint*>(d.kf1 + L.kp)[idx1].octave, 0), d.nlevels1 - 1);
                    const int o2 = min(max(reinterpret_cast<const CorbKeyPoint*>(cd.kf2 + L.kp)[idx2].octave, 0), cd.nlevels2 - 1);
                    o.th1 = s3r_threshold(d.scale1[o1] * d.scale1[o1]); o.th2 = s3r_threshold(cd.scale2[o2] * cd.scale2[o2]);
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        o.x1[k] = s3r_row(h1->m.Tcw + 4 * k, m1->world_pos, h1->m.Tcw[4 * k + 3]);
                        o.x2[k] = s3r_row(h2->m.Tcw + 4 * k, m2->world_pos, h2->m.Tcw[4 * k + 3]);
                    }
                    s3r_project(o.x1, K1, o.p1); s3r_project(o.x2, K2, o.p2);
                    d.set.dense[e] = o;
                    ok = 1;
                }
            }
        }
    }
    d.set.flag[e] = ok;
}

__global__ __launch_bounds__(256) void sim3_ransac_compact_kernel(S3rDev d) { ransac_compact(d.set, d.cap); }

// ComputeCentroid (:215-224): cv::reduce sums a row in float, left to right; C / P.cols multiplies by the double 1.0 / 3 and rounds once
__device__ __forceinline__ void s3r_centroid(const float P[3][3], float Pr[3][3], float* C)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float sum = (P[0][i] + P[1][i]) + P[2][i];
        C[i] = (float)((double)sum * (1.0 / 3.0));
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int i = 0; i < 3; i++) Pr[k][i] = P[k][i] - C[i];
}

// cv::eigen's first eigenvector of the symmetric float 4x4 N: cyclic Jacobi on N taken into FP64.  A pair (p, q) is rotated iff |a_pq| > 2^-60 max|N_ij|; sweeps end
// when one rotates no pair, at most 30 (NaN input rotates nothing).  The column of the largest diagonal entry, lowest index on ties, rounded to float.
__device__ __forceinline__ void s3r_jacobi_top(const float Nf[4][4], float* q)
{
    double A[4][4], V[4][4], scale = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) { A[i][j] = (double)Nf[i][j]; V[i][j] = i == j ? 1.0 : 0.0; if (fabs(A[i][j]) > scale) scale = fabs(A[i][j]); }
    const double tiny = scale * 8.673617379884035e-19;                 // 2^-60
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; p++) {
#pragma unroll
            for (int r_ = p + 1; r_ < 4; r_++) {
                const int qq = r_;
                const double apq = A[p][qq];
                if (fabs(apq) > tiny) {
                    rotated = true;
                    const double app = A[p][p], aqq = A[qq][qq];
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    A[p][p] = app - t * apq; A[qq][qq] = aqq + t * apq; A[p][qq] = 0.0; A[qq][p] = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (k != p && k != qq) {
                            const double akp = A[k][p], akq = A[k][qq];
                            A[k][p] = c * akp - s * akq; A[p][k] = A[k][p];
                            A[k][qq] = s * akp + c * akq; A[qq][k] = A[k][qq];
                        }
                        const double vkp = V[k][p], vkq = V[k][qq];
                        V[k][p] = c * vkp - s * vkq; V[k][qq] = s * vkp + c * vkq;
                    }
                }
            }
        }
        if (!rotated) break;
    }
    double best = A[0][0]; int jb = 0;
#pragma unroll
    for (int j = 1; j < 4; j++) if (A[j][j] > best) { best = A[j][j]; jb = j; }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double v = V[i][0];
#pragma unroll
        for (int j = 1; j < 4; j++) if (j == jb) v = V[i][j];
        q[i] = (float)v;
    }
}

// atan2 + cv::Rodrigues (:278-284) as one algebraic function of the float quaternion, in double: R = I + (2 q0 [v]x + 2 [v]x^2) / |q|^2, every entry rounded once
__device__ __forceinline__ void s3r_rotation(const float* q, float R[3][3])
{
    const double q0 = (double)q[0], v1 = (double)q[1], v2 = (double)q[2], v3 = (double)q[3];
    double vv = v1 * v1; vv = vv + v2 * v2; vv = vv + v3 * v3;
    const double n2 = q0 * q0 + vv, a = 2.0 * q0;
    R[0][0] = (float)(1.0 + (2.0 * (v1 * v1 - vv)) / n2);
    R[0][1] = (float)((a * (-v3) + 2.0 * (v1 * v2)) / n2);
    R[0][2] = (float)((a * v2 + 2.0 * (v1 * v3)) / n2);
    R[1][0] = (float)((a * v3 + 2.0 * (v2 * v1)) / n2);
    R[1][1] = (float)(1.0 + (2.0 * (v2 * v2 - vv)) / n2);
    R[1][2] = (float)((a * (-v1) + 2.0 * (v2 * v3)) / n2);
    R[2][0] = (float)((a * (-v2) + 2.0 * (v3 * v1)) / n2);
    R[2][1] = (float)((a * v1 + 2.0 * (v3 * v2)) / n2);
    R[2][2] = (float)(1.0 + (2.0 * (v3 * v3 - vv)) / n2);
}
__device__ __forceinline__ bool s3r_finite(float x) { return fabsf(x) < __int_as_float(0x7F800000); }

// ComputeSim3 (:226-337) on the three drawn correspondences.  P1[k] / P2[k] = column k of P3Dc1i / P3Dc2i.  Returns false (R, t, s = NaN) when the quaternion's vector
// part is zero -- the reference divides 0 by 0 there -- or when any of R, t, s is not finite.
__device__ __forceinline__ bool s3r_compute_sim3(const float P1[3][3], const float P2[3][3], int fix_scale, S3rHyp& h)
{
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3];
    s3r_centroid(P1, Pr1, O1); s3r_centroid(P2, Pr2, O2);
    float M[3][3];                                                        // M = Pr2 * Pr1.t(): cv::gemm
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s = (double)Pr2[0][i] * (double)Pr1[0][j];
            s = s + (double)Pr2[1][i] * (double)Pr1[1][j];
            s = s + (double)Pr2[2][i] * (double)Pr1[2][j];
            M[i][j] = (float)s;
        }
    // N11 ... N44 (:251-260): float expressions (their double variables receive float results), stored as float
    float N[4][4];
    N[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    N[0][1] = M[1][2] - M[2][1];
    N[0][2] = M[2][0] - M[0][2];
    N[0][3] = M[0][1] - M[1][0];
    N[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    N[1][2] = M[0][1] + M[1][0];
    N[1][3] = M[2][0] + M[0][2];
    N[2][2] = (-M[0][0] + M[1][1]) - M[2][2];
    N[2][3] = M[1][2] + M[2][1];
    N[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
    N[1][0] = N[0][1]; N[2][0] = N[0][2]; N[3][0] = N[0][3]; N[2][1] = N[1][2]; N[3][1] = N[1][3]; N[3][2] = N[2][3];
    s3r_jacobi_top(N, h.q);
    float R[3][3];
    s3r_rotation(h.q, R);
    float s12 = 1.0f;
    if (!fix_scale) {
        float P3[3][3];                                                   // P3 = mR12i * Pr2 (cv::gemm); P3[i][k] = row i, column (point) k
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double s = (double)R[i][0] * (double)Pr2[k][0];
                s = s + (double)R[i][1] * (double)Pr2[k][1];
                s = s + (double)R[i][2] * (double)Pr2[k][2];
                P3[i][k] = (float)s;
            }
        double nom = 0, den = 0;                                          // Pr1.dot(P3): a double sum in memory order; cv::pow(P3, 2) = the float product x * x
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double pn = (double)Pr1[k][i] * (double)P3[i][k], pd = (double)(P3[i][k] * P3[i][k]);
                nom = (i == 0 && k == 0) ? pn : nom + pn;
                den = (i == 0 && k == 0) ? pd : den + pd;
            }
        s12 = (float)(nom / den);
    }
    bool ok = !(h.q[1] == 0 && h.q[2] == 0 && h.q[3] == 0) && s3r_finite(s12);
    // mt12i = O1 - ms12i * mR12i * O2: one cv::gemm with alpha = -s, beta = 1 -- the double sum, scaled and added in double, rounded once
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double s = (double)R[i][0] * (double)O2[0];
        s = s + (double)R[i][1] * (double)O2[1];
        s = s + (double)R[i][2] * (double)O2[2];
        h.t[i] = (float)((double)O1[i] - (double)s12 * s);
        ok = ok && s3r_finite(h.t[i]);
#pragma unroll
        for (int j = 0; j < 3; j++) { h.R[3 * i + j] = R[i][j]; ok = ok && s3r_finite(R[i][j]); }
    }
    h.s = s12;
    if (!ok) {
        h.s = S3R_NAN;
#pragma unroll
        for (int k = 0; k < 9; k++) h.R[k] = S3R_NAN;
#pragma unroll
        for (int k = 0; k < 3; k++) h.t[k] = S3R_NAN;
    }
    return ok;
}

__global__ __launch_bounds__(64) void sim3_ransac_hypothesis_kernel(S3rDev d)
{
    const int it = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    const S3rCand& cd = d.cand[c];
    const int N = min(d.set.ncorr[c], d.cap);
    if (it >= cd.its || it >= d.max_its || N < d.min_inliers || N < 3) return;          // (wave-uniform)
    const S3rCorr* corr = d.set.corr + (size_t)c * d.cap;
    const int* rv = d.rand_values + 3 * ((size_t)c * d.max_its + it);
    int idx[3]; ransac_draw<3>(rv, 3, N, idx);
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const S3rCorr& p = corr[min(max(idx[k], 0), N - 1)];
#pragma unroll
        for (int i = 0; i < 3; i++) { P1[k][i] = p.x1[i]; P2[k][i] = p.x2[i]; }
    }
    S3rHyp h;
    const bool ok = s3r_compute_sim3(P1, P2, d.fix_scale, h);
    // T12 = [s R | t]: sR = ms12i * mR12i is a float product per entry; T21 = [(1.0 / s) R^T | -sRinv t]: the double reciprocal times the entry, rounded once; cv::gemm
    float sR[3][3], sRinv[3][3], tinv[3];
    const double alpha = 1.0 / (double)h.s;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { sR[i][j] = h.s * h.R[3 * i + j]; sRinv[i][j] = (float)(alpha * (double)h.R[3 * j + i]); }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double s = (double)sRinv[i][0] * (double)h.t[0];
        s = s + (double)sRinv[i][1] * (double)h.t[1];
        s = s + (double)sRinv[i][2] * (double)h.t[2];
        tinv[i] = (float)(-s);
    }
    float K1[4], K2[4]; s3r_intrinsics(d, cd, K1, K2);
    // CheckInliers (:340-364): the lanes stride over the correspondences; NaN compares false
    const size_t e = (size_t)c * d.max_its + it;
    const int count = ransac_inlier_words(N, d.words, d.out.mask + e * d.words, [&](int i) {
        if (!ok) return false;
        const S3rCorr p = corr[i];
        float X[3], uv[2];
#pragma unroll
        for (int k = 0; k < 3; k++) X[k] = s3r_row(sR[k], p.x2, h.t[k]);
        s3r_project(X, K1, uv);
        const float d1x = p.p1[0] - uv[0], d1y = p.p1[1] - uv[1];
        const float err1 = (float)((double)d1x * (double)d1x + (double)d1y * (double)d1y);
#pragma unroll
        for (int k = 0; k < 3; k++) X[k] = s3r_row(sRinv[k], p.x1, tinv[k]);
        s3r_project(X, K2, uv);
        const float d2x = uv[0] - p.p2[0], d2y = uv[1] - p.p2[1];
        const float err2 = (float)((double)d2x * (double)d2x + (double)d2y * (double)d2y);
        return err1 < p.th1 && err2 < p.th2;
    });
    if (lane == 0) { h.count = count; d.out.hyp[e] = h; }
}

}  // namespace

void corb_launch_sim3_ransac(const S3rDev& d, int grid_its, int* scan_scratch, hipStream_t s)
{
    if (d.n_cand <= 0 || d.cap <= 0) return;
    ransac_launch_corr_set(sim3_ransac_prepare_kernel, sim3_ransac_compact_kernel, d, d.kf1 != nullptr, scan_scratch, s);
    if (grid_its > 0) hipLaunchKernelGGL(sim3_ransac_hypothesis_kernel, dim3(grid_its, d.n_cand), dim3(64), 0, s, d);
}

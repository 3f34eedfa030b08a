// newpoints_kernels.hip -- the triangulation loop of LocalMapping::CreateNewMapPoints (C/src/LocalMapping.cc:262-418) for gfx950:
//   newpoints_kernel        : one lane per matched pair -- parallax test, linear triangulation (FP64 one-sided Jacobi SVD of the float 4x4 system) or
//                             UnprojectStereo, depth / reprojection / scale tests (:268-398)
//   newpoints_rank_kernel   : record form: rank of every accepted pair in (neighbour, idx1) order
//   newpoints_apply_kernel  : record form: the new MapPoint records and both keyframes' map-point ids (:401-415)
// Arithmetic: the reference's float expressions as non-fused IEEE operations with the C++ types of the source (-ffp-contract=off); cv::Mat products = cv::gemm
// (double accumulation, one rounding), cv::norm / Mat::dot = double sums (numerics contract).  The kernel is a few waves of dependent FP64 per call and
// latency bound: one lane per pair, the 4x4 A and V of the Jacobi iteration in registers (every index below is a compile-time constant after unrolling).
#include "newpoints_internal.h"
#include "kfinsert_math.h"              // NpCam, np_cam_finish, np_unproject_uv: shared with kfinsert_kernels.hip

namespace {

__device__ __forceinline__ void np_load_cam(const NpSide& s, NpCam& c)
{
    const float* T = s.hdr ? s.hdr->m.Tcw : s.Tcw;
#pragma unroll
    for (int k = 0; k < 12; k++) c.T[k] = T[k];
    c.fx = s.hdr ? s.hdr->m.fx : s.fx; c.fy = s.hdr ? s.hdr->m.fy : s.fy; c.cx = s.hdr ? s.hdr->m.cx : s.cx; c.cy = s.hdr ? s.hdr->m.cy : s.cy;
    np_cam_finish(c);                                                  // invfx = 1.0f / fx; Ow = -Rcw^T * tcw
}
// Rcw.row(r).dot(x3Dt) : Mat::dot, a double sum
__device__ __forceinline__ double np_rowdot(const NpCam& c, int r, const float* X)
{
    double s = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) s += (double)c.T[r * 4 + k] * (double)X[k];
    return s;
}
__device__ __forceinline__ double np_norm3(const float* v) { return sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]); }

// right singular vector of the smallest singular value of the float 4x4 A: one-sided (Hestenes) Jacobi in FP64 on the columns of A, V accumulates the
// rotations; sweeps until no pair of columns is rotated, at most 30.  Components rounded to float.
__device__ __forceinline__ void np_svd_null(const float* Af, float* v4)
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
    double best = 0; int jb = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double n2 = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) n2 += U[k][j] * U[k][j];
        if (j == 0 || n2 < best) { best = n2; jb = j; }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double v = V[i][0];
#pragma unroll
        for (int j = 1; j < 4; j++) if (j == jb) v = V[i][j];
        v4[i] = (float)v;
    }
}

// (d*d - h*h) / (d*d + h*h) in double = cos(2 atan2(h, d)), rounded once (:289 / :291)
__device__ __forceinline__ float np_cos_stereo(float mb, float depth)
{
    const double h = (double)(mb / 2), d = (double)depth;
    return (float)((d * d - h * h) / (d * d + h * h));
}
// KeyFrame::UnprojectStereo (C/src/KeyFrame.cc:741-754): Twc = [Rcw^T | Ow]
__device__ __forceinline__ void np_unproject(const NpCam& c, const CorbKeyPoint& k, float z, float* X) { np_unproject_uv(c, k.x, k.y, z, X); }
// reprojection test of one keyframe (:334-379); bf is the CURRENT keyframe's in both (:349, :372)
__device__ __forceinline__ bool np_reproj_ok(const NpCam& c, const float* X, float z, const CorbKeyPoint& k, float ur, bool stereo, float bf, float sigma2)
{
    const float x = (float)(np_rowdot(c, 0, X) + (double)c.T[3]);
    const float y = (float)(np_rowdot(c, 1, X) + (double)c.T[7]);
    const float invz = (float)(1.0 / (double)z);
    const float u = c.fx * x * invz + c.cx, v = c.fy * y * invz + c.cy;
    const float ex = u - k.x, ey = v - k.y;
    if (!stereo) return !((double)(ex * ex + ey * ey) > 5.991 * (double)sigma2);
    const float u_r = u - bf * invz, er = u_r - ur;
    return !((double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2);
}

__device__ __forceinline__ int np_decide(const NpDev& d, const NpCam& c1, const NpCam& c2, int idx1, int idx2, float* X, int* source)
{
    const CorbKeyPoint k1 = d.s1.kp[idx1], k2 = d.s2.kp[idx2];
    const float ur1 = d.s1.ur[idx1], ur2 = d.s2.ur[idx2];
    const bool st1 = ur1 >= 0, st2 = ur2 >= 0;
    X[0] = X[1] = X[2] = 0.f; *source = 0;
    const float xn1[3] = {(k1.x - c1.cx) * c1.invfx, (k1.y - c1.cy) * c1.invfy, 1.0f};
    const float xn2[3] = {(k2.x - c2.cx) * c2.invfx, (k2.y - c2.cy) * c2.invfy, 1.0f};
    float ray1[3], ray2[3];                                           // Rwc * xn
#pragma unroll
    for (int i = 0; i < 3; i++) {
        ray1[i] = (float)((double)c1.T[0 * 4 + i] * (double)xn1[0] + (double)c1.T[1 * 4 + i] * (double)xn1[1] + (double)c1.T[2 * 4 + i] * (double)xn1[2]);
        ray2[i] = (float)((double)c2.T[0 * 4 + i] * (double)xn2[0] + (double)c2.T[1 * 4 + i] * (double)xn2[1] + (double)c2.T[2 * 4 + i] * (double)xn2[2]);
    }
    const double dot = (double)ray1[0] * ray2[0] + (double)ray1[1] * ray2[1] + (double)ray1[2] * ray2[2];
    const float cosRays = (float)(dot / (np_norm3(ray1) * np_norm3(ray2)));
    float cos1 = cosRays + 1, cos2 = cos1;
    if (st1) cos1 = np_cos_stereo(d.s1.mb, d.s1.depth[idx1]);
    else if (st2) cos2 = np_cos_stereo(d.s2.mb, d.s2.depth[idx2]);   // (the reference's `else if`: with both sides stereo only side 1 is evaluated)
    const float cosStereo = fminf(cos1, cos2);
    if (cosRays < cosStereo && cosRays > 0 && (st1 || st2 || (double)cosRays < 0.9998)) {
        float A[16];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            A[0 * 4 + k] = xn1[0] * c1.T[2 * 4 + k] - c1.T[0 * 4 + k];
            A[1 * 4 + k] = xn1[1] * c1.T[2 * 4 + k] - c1.T[1 * 4 + k];
            A[2 * 4 + k] = xn2[0] * c2.T[2 * 4 + k] - c2.T[0 * 4 + k];
            A[3 * 4 + k] = xn2[1] * c2.T[2 * 4 + k] - c2.T[1 * 4 + k];
        }
        float v[4]; np_svd_null(A, v);
        if (v[3] == 0) return CORB_NP_W_ZERO;
        X[0] = v[0] / v[3]; X[1] = v[1] / v[3]; X[2] = v[2] / v[3];
    } else if (st1 && cos1 < cos2 && d.s1.depth[idx1] > 0) { np_unproject(c1, k1, d.s1.depth[idx1], X); *source = 1; }
    else if (st2 && cos2 < cos1 && d.s2.depth[idx2] > 0) { np_unproject(c2, k2, d.s2.depth[idx2], X); *source = 2; }
    else return CORB_NP_NO_PARALLAX;

    const float z1 = (float)(np_rowdot(c1, 2, X) + (double)c1.T[11]);
    if (z1 <= 0) return CORB_NP_BEHIND_1;
    const float z2 = (float)(np_rowdot(c2, 2, X) + (double)c2.T[11]);
    if (z2 <= 0) return CORB_NP_BEHIND_2;
    const int o1 = min(max(k1.octave, 0), d.s1.nlevels - 1), o2 = min(max(k2.octave, 0), d.s2.nlevels - 1);
    const float sc1 = d.s1.scale[o1], sc2 = d.s2.scale[o2];
    const float bf = d.s1.hdr ? d.s1.hdr->m.bf : d.s1.bf;
    if (!np_reproj_ok(c1, X, z1, k1, ur1, st1, bf, sc1 * sc1)) return CORB_NP_REPROJ_1;
    if (!np_reproj_ok(c2, X, z2, k2, ur2, st2, bf, sc2 * sc2)) return CORB_NP_REPROJ_2;
    const float n1[3] = {X[0] - c1.Ow[0], X[1] - c1.Ow[1], X[2] - c1.Ow[2]}, n2[3] = {X[0] - c2.Ow[0], X[1] - c2.Ow[1], X[2] - c2.Ow[2]};
    const float dist1 = (float)np_norm3(n1), dist2 = (float)np_norm3(n2);
    if (dist1 == 0 || dist2 == 0) return CORB_NP_SCALE;
    const float ratioDist = dist2 / dist1, ratioFactor = 1.5f * d.s1.scale[d.s1.nlevels > 1 ? 1 : 0], ratioOctave = sc1 / sc2;      // mfScaleFactor = mvScaleFactors[1]
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return CORB_NP_SCALE;
    return CORB_NP_OK;
}

__global__ __launch_bounds__(64) void newpoints_kernel(NpDev d)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= d.n) return;
    int idx1, idx2;
    if (d.pairs) { idx1 = d.pairs[2 * i]; idx2 = d.pairs[2 * i + 1]; }
    else {
        idx1 = i; idx2 = d.match[i];
        if (idx2 < 0 || idx2 >= d.n2) { d.status[i] = CORB_NP_NONE; d.source[i] = 0; d.x3d[3 * (size_t)i] = d.x3d[3 * (size_t)i + 1] = d.x3d[3 * (size_t)i + 2] = 0.f; return; }
    }
    NpCam c1, c2; np_load_cam(d.s1, c1); np_load_cam(d.s2, c2);
    float X[3]; int source;
    const int st = np_decide(d, c1, c2, idx1, idx2, X, &source);
    d.x3d[3 * (size_t)i] = X[0]; d.x3d[3 * (size_t)i + 1] = X[1]; d.x3d[3 * (size_t)i + 2] = X[2];
    d.status[i] = (unsigned char)st; d.source[i] = (unsigned char)source;
    if (st == CORB_NP_OK) {
        atomicAdd(d.n_new, 1);
        if (d.flags1) d.flags1[idx1] = 1;                              // mpCurrentKeyFrame->AddMapPoint(pMP, idx1): later neighbours skip the feature
        if (d.winner) atomicMax(&d.winner[idx2], idx1);
    }
}

// k of every OK pair in (neighbour, idx1) order: one workgroup, each thread a contiguous run of the dense array
__global__ __launch_bounds__(1024) void newpoints_rank_kernel(NpApplyDev d)
{
    __shared__ int part[1024];
    const int total = d.n_nb * d.n1, per = (total + 1023) / 1024;
    const int b = min((int)threadIdx.x * per, total), e = min(b + per, total);
    int cnt = 0;
    for (int i = b; i < e; i++) cnt += d.status[i] == CORB_NP_OK;
    part[threadIdx.x] = cnt;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int k = part[threadIdx.x] - cnt;
    for (int i = b; i < e; i++) d.rank[i] = d.status[i] == CORB_NP_OK ? k++ : -1;
    if (threadIdx.x == 1023) { d.totals[0] = part[1023]; d.totals[1] = (d.apply && part[1023] > d.mp_capacity - d.first_mp_slot) ? 1 : 0; }
}

// the new MapPoint of one OK pair (:401-415) and its two AddMapPoint calls, on the records
__global__ __launch_bounds__(256) void newpoints_apply_kernel(NpApplyDev d)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n_nb * d.n1 || d.totals[1]) return;
    const int k = d.rank[i];
    if (k < 0) return;
    const int j = i / d.n1, idx1 = i - j * d.n1, idx2 = d.match[i];
    const RecLayout KL(d.F); const MpLayout ML(d.max_obs);
    char* r1 = d.kf_base + (size_t)d.cur_slot * d.kf_bytes; char* r2 = d.kf_base + (size_t)d.nb_slots[j] * d.kf_bytes;
    const KfHeader* h1 = reinterpret_cast<const KfHeader*>(r1); const KfHeader* h2 = reinterpret_cast<const KfHeader*>(r2);
    char* rec = d.mp_base + (size_t)(d.first_mp_slot + k) * d.mp_bytes;
    unsigned long long* w = reinterpret_cast<unsigned long long*>(rec);
    for (int q = 0; q < CORB_MP_HEADER_BYTES / 8; q++) w[q] = 0ull;                         // header and counters
    unsigned long long* okf = reinterpret_cast<unsigned long long*>(rec + ML.obs_kf); uint32_t* oidx = reinterpret_cast<uint32_t*>(rec + ML.obs_idx);
    for (int q = 0; q < d.max_obs; q++) { okf[q] = 0ull; oidx[q] = 0u; }
    unsigned long long* sc = reinterpret_cast<unsigned long long*>(rec + ML.scratch);
    for (int q = 0; q < (int)(sizeof(CorbMapPointScratch) / 8); q++) sc[q] = 0ull;
    CorbMapPointRecord* m = reinterpret_cast<CorbMapPointRecord*>(rec);
    const unsigned long long id = d.first_mp_id + (unsigned long long)k, id1 = h1->m.id, id2 = h2->m.id;
    m->id = id; m->ref_kf_id = id1; m->client_id = d.client_id; m->flags = 0;
    const float X[3] = {d.x3d[3 * (size_t)i], d.x3d[3 * (size_t)i + 1], d.x3d[3 * (size_t)i + 2]};
    m->world_pos[0] = X[0]; m->world_pos[1] = X[1]; m->world_pos[2] = X[2];
    // mObservations ascends in the keyframe id; ComputeDistinctiveDescriptors of two observations keeps the first one's descriptor (both medians are 0,
    // MapPoint.cc:383-394: the rule of corb_distinctive_descriptors)
    const bool first1 = id1 <= id2;
    if (d.max_obs >= 2) { okf[0] = first1 ? id1 : id2; oidx[0] = (uint32_t)(first1 ? idx1 : idx2); okf[1] = first1 ? id2 : id1; oidx[1] = (uint32_t)(first1 ? idx2 : idx1); m->n_obs = 2; }
    const unsigned long long* dsrc = reinterpret_cast<const unsigned long long*>((first1 ? r1 : r2) + KL.desc) + 4 * (size_t)(first1 ? idx1 : idx2);
    unsigned long long* ddst = reinterpret_cast<unsigned long long*>(m->descriptor);
#pragma unroll
    for (int q = 0; q < 4; q++) ddst[q] = dsrc[q];
    // MapPoint::UpdateNormalAndDepth (MapPoint.cc:424-471) over the two observations, in list order; mpRefKF = the current keyframe
    float Oa[3], Ob[3];
    const float* Ta = first1 ? h1->m.Tcw : h2->m.Tcw; const float* Tb = first1 ? h2->m.Tcw : h1->m.Tcw;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        double s_ = 0, t_ = 0;
        for (int q = 0; q < 3; q++) { s_ += (double)(-Ta[q * 4 + a]) * (double)Ta[q * 4 + 3]; t_ += (double)(-Tb[q * 4 + a]) * (double)Tb[q * 4 + 3]; }
        Oa[a] = (float)s_; Ob[a] = (float)t_;
    }
    const float va[3] = {X[0] - Oa[0], X[1] - Oa[1], X[2] - Oa[2]}, vb[3] = {X[0] - Ob[0], X[1] - Ob[1], X[2] - Ob[2]};
    const double na = np_norm3(va), nb = np_norm3(vb), ia = 1.0 / na, ib = 1.0 / nb;         // Mat / double scales by the reciprocal
#pragma unroll
    for (int a = 0; a < 3; a++) {
        float n = 0.f; n = n + (float)((double)va[a] * ia); n = n + (float)((double)vb[a] * ib);
        m->normal[a] = (float)((double)n * (1.0 / 2.0));
    }
    const float dist = (float)(first1 ? na : nb);
    const int nl = min(max(d.nlevels, 1), CORB_MAX_LEVELS);
    const int level = min(max(reinterpret_cast<const CorbKeyPoint*>(r1 + KL.kp)[idx1].octave, 0), nl - 1);
    m->max_distance = dist * d.scale[level];
    m->min_distance = m->max_distance / d.scale[nl - 1];
    // AddMapPoint on both keyframes; of two pairs of one neighbour that share idx2 the later one stays
    reinterpret_cast<unsigned long long*>(r1 + KL.mp_id)[idx1] = id; reinterpret_cast<unsigned char*>(r1 + KL.flags)[idx1] |= 1u;
    if (d.winner[(size_t)j * d.F + idx2] == idx1) { reinterpret_cast<unsigned long long*>(r2 + KL.mp_id)[idx2] = id; reinterpret_cast<unsigned char*>(r2 + KL.flags)[idx2] |= 1u; }
}

}  // namespace

void corb_launch_newpoints(const NpDev& d, hipStream_t s)
{
    if (d.n > 0) hipLaunchKernelGGL(newpoints_kernel, dim3((d.n + 63) / 64), dim3(64), 0, s, d);
}
void corb_launch_newpoints_apply(const NpApplyDev& d, hipStream_t s)
{
    hipLaunchKernelGGL(newpoints_rank_kernel, dim3(1), dim3(1024), 0, s, d);
    const int total = d.n_nb * d.n1;
    if (d.apply && total > 0) hipLaunchKernelGGL(newpoints_apply_kernel, dim3((total + 255) / 256), dim3(256), 0, s, d);
}

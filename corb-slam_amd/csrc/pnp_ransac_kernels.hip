// pnp_ransac_kernels.hip -- the PnPsolver RANSAC of Tracking::Relocalization and the server's map fusion (C/src/PnPsolver.cc) for gfx950:
//   pnp_ransac_prepare_kernel    : per correspondence: mvP3Dw, mvP2D and mvMaxError = mvSigma2 * th2 (:199-201); on records also the constructor's filter for feature
//                                  i of the frame (:79-101) through the map's id index
//   pnp_ransac_compact_kernel    : record route: the accepted features in ascending order (mvKeyPointIndices), after the scan of device_util.hip
//   pnp_ransac_hypothesis_kernel : one single-wave workgroup per (iteration, candidate): the min_set draws (:233-246), EPnP's compute_pose (:522-570) on them, then
//                                  CheckInliers (:353-384) with the lanes striding over the correspondences -- a ballot per 64, one 64-bit mask word each
//   pnp_ransac_refine_kernel     : the same grid; a workgroup whose hypothesis changes the running best (c_i >= m and c_i > every earlier c_j >= m) runs Refine()
//                                  (:305-350): compute_pose on the set bits of its mask in ascending order, CheckInliers over all N
// The arithmetic is csrc/pnp_math.h, the same text a host program runs: doubles in the order of the source, unfused (-ffp-contract=off).  Its PnpWork -- the 12 x 12
// MtM and its rotations (2.3 KB) and the small systems -- lives in LDS; sums over correspondences are taken by one lane per output entry, rows ascending (78 entries
// of MtM, 9 of ABt, 6 of PW0tPW0), a Jacobi rotation's row / column updates by one lane per index, the rest by lane 0.  alphas and pcs are recomputed where they are
// used: no array grows with hypotheses x N.  A call is a few hundred waves and latency bound.
// Compiler's resource summary (hipcc -O3, gfx950):
//   kernel                          VGPRs  SGPRs  scratch bytes  LDS bytes
//   pnp_ransac_prepare_kernel          16     27              0          0
//   pnp_ransac_compact_kernel          16     29              0          0
//   pnp_ransac_hypothesis_kernel      140     98              0       5208
//   pnp_ransac_refine_kernel          140    100              0       5208
#include "pnp_ransac_internal.h"

namespace {

__global__ __launch_bounds__(256) void pnp_ransac_prepare_kernel(PnrDev d)
{
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    const PnrCand& cd = d.cand[c];
    if (i >= cd.n || i >= d.cap) return;
    const size_t e = (size_t)c * d.cap + i;
    PnpCorr o;
    if (!d.kf) {
        const float* r = d.in + 6 * ((size_t)cd.in_off + i);
        o.X[0] = r[0]; o.X[1] = r[1]; o.X[2] = r[2]; o.u[0] = r[3]; o.u[1] = r[4];
        o.max_err = r[5] * d.th2;
        d.set.corr[e] = o;
        return;
    }
    // the constructor's filter for feature i of the frame (:79-101): a match that the map's id index resolves to a record that is not bad
    int ok = 0;
    const unsigned long long id = d.matched[e];
    if (id != CORB_NO_MAP_POINT) {
        const int s = corb_idtab_find(d.idt, id);
        if (s >= 0) {
            const CorbMapPointRecord* m = reinterpret_cast<const CorbMapPointRecord*>(d.mp_base + (size_t)s * d.mp_bytes);
            if (!(m->flags & CORB_MP_BAD)) {
                const RecLayout L(d.F);
                const CorbKeyPoint kp = reinterpret_cast<const CorbKeyPoint*>(d.kf + L.kp)[i];             // mvKeysUn[i]
                const int oc = min(max(kp.octave, 0), d.nlevels - 1);
                o.X[0] = m->world_pos[0]; o.X[1] = m->world_pos[1]; o.X[2] = m->world_pos[2]; o.u[0] = kp.x; o.u[1] = kp.y;
                o.max_err = (d.scale[oc] * d.scale[oc]) * d.th2;                                          // mvLevelSigma2 = scale^2 in float, times th2
                d.set.dense[e] = o;
                ok = 1;
            }
        }
    }
    d.set.flag[e] = ok;
}

__global__ __launch_bounds__(256) void pnp_ransac_compact_kernel(PnrDev d) { ransac_compact(d.set, d.cap); }

// mRansacMinInliers after SetRansacParameters' adjustment (:179-184): int(N * epsilon) is a float product, truncated
__device__ __forceinline__ int pnr_min_inliers(int N, const PnrDev& d) { return max(max((int)((float)N * d.epsilon), d.min_inliers), d.min_set); }
__device__ __forceinline__ void pnr_intrinsics(const PnrDev& d, const PnrCand& cd, double* K)
{
    if (d.kf) { const KfHeader* h = reinterpret_cast<const KfHeader*>(d.kf); K[0] = (double)h->m.fx; K[1] = (double)h->m.fy; K[2] = (double)h->m.cx; K[3] = (double)h->m.cy; }
    else for (int k = 0; k < 4; k++) K[k] = (double)cd.K[k];
}

// CheckInliers (:353-384) over the N correspondences of a candidate with the pose the workgroup holds in LDS; the count comes back in every lane
__device__ __forceinline__ int pnr_check_inliers(const PnpPose& pose, const double* K, const PnpCorr* corr, int N, int words, unsigned long long* mask)
{
    double R[9], t[3], Kr[4];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = pose.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = pose.t[k];
#pragma unroll
    for (int k = 0; k < 4; k++) Kr[k] = K[k];
    return ransac_inlier_words(N, words, mask, [&](int i) { return pnp_check_inlier(R, t, corr[i], Kr); });
}

struct PnrShared { PnpWork W; PnpPose pose; double K[4]; int idx[8]; };

__global__ __launch_bounds__(64) void pnp_ransac_hypothesis_kernel(PnrDev d)
{
    const int it = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    const PnrCand& cd = d.cand[c];
    const int N = min(d.set.ncorr[c], d.cap);
    if (it >= cd.its || it >= d.stride_its || N < pnr_min_inliers(N, d)) return;                    // (wave-uniform; mRansacMinInliers >= min_set)
    __shared__ PnrShared sh;
    const PnpCorr* corr = d.set.corr + (size_t)c * d.cap;
    if (lane == 0) {
        ransac_draw<8>(d.rand_values + (size_t)d.min_set * ((size_t)c * d.stride_its + it), d.min_set, N, sh.idx);
        for (int k = 0; k < d.min_set; k++) sh.idx[k] = min(max(sh.idx[k], 0), N - 1);
        pnr_intrinsics(d, cd, sh.K);
    }
    __syncthreads();
    const PnpIndexSet S{corr, sh.idx, d.min_set};
    pnp_compute_pose(S, sh.K, sh.W, sh.pose);
    __syncthreads();
    const size_t h = (size_t)c * d.stride_its + it;
    const int count = pnr_check_inliers(sh.pose, sh.K, corr, N, d.words, d.out.mask + h * d.words);
    if (lane == 0) { d.out.hyp[h].count = count; d.out.hyp[h].pad = 0; d.out.hyp[h].pose = sh.pose; }
}

__global__ __launch_bounds__(64) void pnp_ransac_refine_kernel(PnrDev d)
{
    const int it = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    const PnrCand& cd = d.cand[c];
    const int N = min(d.set.ncorr[c], d.cap), m = pnr_min_inliers(N, d);
    if (it >= cd.its || it >= d.stride_its || N < m) return;
    // a record?  c_i >= m and c_i > every earlier c_j >= m
    const PnrHyp* hyp = d.out.hyp + (size_t)c * d.stride_its;
    const int ci = hyp[it].count;
    if (ci < m) return;
    bool beaten = false;
    for (int j = lane; j < it; j += 64) { const int cj = hyp[j].count; beaten = beaten || (cj >= m && cj >= ci); }
    if (__ballot(beaten) != 0ull) return;
    __shared__ PnrShared sh;
    const PnpCorr* corr = d.set.corr + (size_t)c * d.cap;
    if (lane == 0) pnr_intrinsics(d, cd, sh.K);
    __syncthreads();
    const size_t h = (size_t)c * d.stride_its + it;
    const PnpMaskSet S{corr, d.out.mask + h * d.words, d.words, ci};
    pnp_compute_pose(S, sh.K, sh.W, sh.pose);
    __syncthreads();
    const int count = pnr_check_inliers(sh.pose, sh.K, corr, N, d.words, d.ref.mask + h * d.words);
    if (lane == 0) { d.ref.hyp[h].count = count; d.ref.hyp[h].pad = 0; d.ref.hyp[h].pose = sh.pose; }
}

}  // namespace

void corb_launch_pnp_ransac(const PnrDev& d, int grid_its, int* scan_scratch, hipStream_t s)
{
    if (d.n_cand <= 0 || d.cap <= 0) return;
    ransac_launch_corr_set(pnp_ransac_prepare_kernel, pnp_ransac_compact_kernel, d, d.kf != nullptr, scan_scratch, s);
    if (grid_its <= 0) return;
    hipLaunchKernelGGL(pnp_ransac_hypothesis_kernel, dim3(grid_its, d.n_cand), dim3(64), 0, s, d);
    hipLaunchKernelGGL(pnp_ransac_refine_kernel, dim3(grid_its, d.n_cand), dim3(64), 0, s, d);
}

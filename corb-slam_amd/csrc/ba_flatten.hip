// ba_flatten.hip -- the graph flattening of Optimizer::BundleAdjustment on the device.
// What ba_flatten_host.cpp's host flattening does for a CorbBAProblem in host memory (active-edge filter, g2o's index mapping -- free poses, then free
// landmarks, ascending: G/core/sparse_optimizer.cpp:166-190 --, edges sorted by landmark with the free-pose edges first, per-keyframe edge lists,
// block pattern of the reduced camera system: G/core/block_solver.hpp:143-295) for a problem whose arrays already live in device memory
// (CorbBADeviceProblem: edges grouped by map point, as corb_ba_solve_store derives them from the map-point records).  Same lists, element for element;
// nothing travels to the host but a handful of counts.
//
//   flat_point_kernel      per map point: active edges (an edge between two fixed vertices is dropped, sparse_optimizer.cpp:234), free-pose edges
//   (scans)                landmark / pose hessian indices, edge offsets
//   flat_edge_kernel       per map point: its edges to their sorted places (free poses first), structure-of-arrays, per-keyframe counts
//   flat_pose_list_kernel  per edge: into its keyframe's list (unordered), then
//   flat_pose_sort_kernel  per keyframe: list sorted ascending in LDS (bitonic), landmark of every entry
//   flat_rows_kernel       per keyframe: the block row of the reduced system as a bitmap over the keyframes in LDS (count pass / fill pass)
#include "ba_flatten.h"
#include "lane_exchange.h"
#include "ba_math.h"

__global__ __launch_bounds__(256) void flat_point_kernel(BAFlattenDev d)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m < d.K) d.pflag[m] = d.pose_fixed[m] ? 0 : 1;
    if (m >= d.M) return;
    const bool xf = d.point_fixed[m] != 0;
    int nact = 0, nfree = 0;
    for (int e = d.edge_off[m]; e < d.edge_off[m + 1]; e++) {
        const bool pf = d.pose_fixed[d.edges[e].pose] != 0;
        if (pf && xf) continue;                            // allVerticesFixed
        nact++; nfree += pf ? 0 : 1;
    }
    const int lflag = (!xf && nact > 0) ? 1 : 0;           // points without edges are removed (Optimizer.cc:198-202)
    d.lflag[m] = lflag; d.cntA[m] = lflag ? nact : 0; d.cntB[m] = lflag ? 0 : nact; d.nfree_pt[m] = nfree;
    d.pt_touched[m] = nact > 0 ? 1 : 0;
    if (lflag && nfree > 0) atomicAdd(d.scal + FLAT_PAIRS, nfree < 32768 ? nfree * nfree : 0x3FFFFFFF);      // (read by the local-window driver only: a window's sum is far from 2^31)
}

// estimates and per-vertex tables: Converter::toSE3Quat (float R, t -> double -> Eigen::Quaterniond(R), normalised), points as doubles, intrinsics as doubles
__global__ __launch_bounds__(256) void flat_state_in_kernel(BAFlattenDev d)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < d.K) {
        const float* T = d.poses + 16 * (size_t)i;
        const double R[9] = { T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10] };
        double q[4]; quat_from_R(R, q); quat_normalize(q);
        double* Q = d.state + 4 * (size_t)i;
        Q[0] = q[0]; Q[1] = q[1]; Q[2] = q[2]; Q[3] = q[3];
        double* t = d.state + 4 * (size_t)d.K + 3 * (size_t)i;
        t[0] = T[3]; t[1] = T[7]; t[2] = T[11];
        for (int a = 0; a < 5; a++) d.cam[5 * (size_t)i + a] = d.intr[5 * (size_t)i + a];
        const int p = d.pflag[i] ? d.pidx[i] : -1;
        if (p >= 0) d.pose_vertex[p] = i;
    }
    if (i < d.M) {
        double* x = d.state + 7 * (size_t)d.K + 3 * (size_t)i;
        x[0] = d.points[3 * (size_t)i]; x[1] = d.points[3 * (size_t)i + 1]; x[2] = d.points[3 * (size_t)i + 2];
    }
}
// Converter::toCvMat (double -> float) of the non-fixed keyframes and of the optimised, non-fixed map points; everything else keeps its input value
__global__ __launch_bounds__(256) void flat_state_out_kernel(BAFlattenDev d)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < d.K && !d.pose_fixed[i] && d.pcnt[d.pidx[i]] > 0) {      // (a free keyframe without an observation was never optimised: it keeps its input value, like the host path's)
        double R[9]; quat_to_R(d.state + 4 * (size_t)i, R);
        const double* t = d.state + 4 * (size_t)d.K + 3 * (size_t)i;
        float* T = d.poses + 16 * (size_t)i;
        T[0] = (float)R[0]; T[1] = (float)R[1]; T[2] = (float)R[2]; T[3] = (float)t[0];
        T[4] = (float)R[3]; T[5] = (float)R[4]; T[6] = (float)R[5]; T[7] = (float)t[1];
        T[8] = (float)R[6]; T[9] = (float)R[7]; T[10] = (float)R[8]; T[11] = (float)t[2];
        T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
    }
    if (i < d.M && !d.point_fixed[i] && d.pt_touched[i]) {
        const double* x = d.state + 7 * (size_t)d.K + 3 * (size_t)i;
        d.points[3 * (size_t)i] = (float)x[0]; d.points[3 * (size_t)i + 1] = (float)x[1]; d.points[3 * (size_t)i + 2] = (float)x[2];
    }
}

// FEW > 0 (= the number of free keyframes, at most 64: local windows): the per-keyframe counts are summed in LDS and reach device memory as one atomic per
// (workgroup, keyframe) -- a window's ten thousand edges otherwise queue up on five addresses
template <bool FEW>
__global__ __launch_bounds__(256) void flat_edge_kernel(BAFlattenDev d, int few)
{
    __shared__ int hist[64];
    if (FEW) { if (threadIdx.x < 64) hist[threadIdx.x] = 0; __syncthreads(); }
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m < d.M) {
    const int A = d.eoffA[d.M];                            // edges of free landmarks come first
    if (m == 0) d.loff[d.lidx[d.M]] = A;
    const bool xf = d.point_fixed[m] != 0;
    const int lf = d.lflag[m];
    const int l = lf ? d.lidx[m] : -1;
    if (lf) { d.loff[l] = d.eoffA[m]; d.lnfree[l] = d.nfree_pt[m]; d.point_vertex[l] = m; }
    const int e0 = d.edge_off[m], e1 = d.edge_off[m + 1];
    const int base = lf ? d.eoffA[m] : A + d.eoffB[m];
    int jf = base, jx = base + d.nfree_pt[m];              // next place of a free-pose / fixed-pose edge
    for (int e = e0; e < e1; e++) {
        const CorbBAEdge ed = d.edges[e];
        const bool pf = d.pose_fixed[ed.pose] != 0;
        if (pf && xf) continue;
        const int j = pf ? jx++ : jf++;
        const int ep = pf ? -1 : d.pidx[ed.pose];
        d.e_pose[j] = ep; d.e_point[j] = l; d.e_vpose[j] = ed.pose; d.e_vpoint[j] = m;
        d.e_dim[j] = ed.u_right < 0 ? 2 : 3;               // mvuRight<0 -> EdgeSE3ProjectXYZ, else EdgeStereoSE3ProjectXYZ (Optimizer.cc:147)
        double* o = d.e_obs + 3 * (size_t)j; o[0] = ed.u; o[1] = ed.v; o[2] = ed.u_right;
        d.e_w[j] = ed.inv_sigma2;
        if (d.e_src) d.e_src[j] = e;
        if (ep >= 0) { if (FEW) atomicAdd(&hist[ep], 1); else if (!d.erel) atomicAdd(&d.pcnt[ep], 1); }            // (integer counts: order-free; maps count in flat_pose_count_kernel)
    }
    }
    if (FEW) { __syncthreads(); if ((int)threadIdx.x < few && hist[threadIdx.x]) atomicAdd(&d.pcnt[threadIdx.x], hist[threadIdx.x]); }
}
// Maps: the same placement with a thread per EDGE (consecutive threads read consecutive 24-byte edges and write nearly consecutive places; the per-point form's threads
// stride over ~5.5 edges each: 2.1 ms at 27.5 M observations).  An edge's rank among the earlier edges of its class (free / fixed keyframe) inside its map point is
// counted from the point's first edge -- at most max_obs - 1 neighbouring records.  Counts per keyframe: flat_pose_count_kernel.
__global__ __launch_bounds__(256) void flat_edge_by_edge_kernel(BAFlattenDev d)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int A = d.eoffA[d.M];                            // edges of free landmarks come first
    if (e == 0) d.loff[d.lidx[d.M]] = A;
    if (e >= d.E) return;
    const CorbBAEdge ed = d.edges[e];
    const int m = ed.point, e0 = d.edge_off[m];
    const bool xf = d.point_fixed[m] != 0, pf = d.pose_fixed[ed.pose] != 0;
    const int lf = d.lflag[m];
    const int l = lf ? d.lidx[m] : -1;
    const int nfree = d.nfree_pt[m];
    if (e == e0 && lf) { d.loff[l] = d.eoffA[m]; d.lnfree[l] = nfree; d.point_vertex[l] = m; }
    if (pf && xf) return;                                  // allVerticesFixed
    int rank = 0;
    for (int k = e0; k < e; k++) rank += ((d.pose_fixed[d.edges[k].pose] != 0) == pf) ? 1 : 0;
    const int base = lf ? d.eoffA[m] : A + d.eoffB[m];
    const int j = base + (pf ? nfree : 0) + rank;
    const int ep = pf ? -1 : d.pidx[ed.pose];
    d.e_pose[j] = ep; d.e_point[j] = l; d.e_vpose[j] = ed.pose; d.e_vpoint[j] = m;
    d.e_dim[j] = ed.u_right < 0 ? 2 : 3;
    double* o = d.e_obs + 3 * (size_t)j; o[0] = ed.u; o[1] = ed.v; o[2] = ed.u_right;
    d.e_w[j] = ed.inv_sigma2;
    if (d.e_src) d.e_src[j] = e;
}
// one workgroup per free keyframe k: the flattened edges whose keyframe is k, in ascending order, with the landmark of every entry
__global__ __launch_bounds__(1024) void flat_pose_lists_ordered_kernel(BAFlattenDev d, int nE)
{
    __shared__ int wcnt[16];
    const int k = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    int at = d.poff[k];
    for (int j0 = 0; j0 < nE; j0 += 1024) {
        const int j = j0 + t;
        const bool mine = j < nE && d.e_pose[j] == k;
        const unsigned long long b = __ballot(mine);
        if (lane == 0) wcnt[w] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
        for (int i = 0; i < 16; i++) { if (i < w) before += wcnt[i]; total += wcnt[i]; }
        if (mine) { const int pos = at + before + __popcll(b & ((1ull << lane) - 1ull)); d.pedge[pos] = j; d.plm[pos] = d.e_point[j]; }
        at += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void flat_pose_list_kernel(BAFlattenDev d, int nE)
{
    const int j = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    int len = 0;
    const int ep = j < nE ? d.e_pose[j] : -1;
    // The edges are sorted by landmark, so a wavefront's 64 edges belong to a handful of keyframes: one returning atomic per (wavefront, keyframe) instead of one per edge
    // (27.5 M of them on clustered addresses were this kernel's 5.0 ms at 50 000 keyframes), the lanes of a keyframe take consecutive slots behind it.
    bool pending = ep >= 0;
    while (true) {
        const unsigned long long pm = __ballot(pending);
        if (!pm) break;
        const int leader = __ffsll((long long)pm) - 1;
        const int lp = __shfl(ep, leader);
        const bool same = pending && ep == lp;
        const unsigned long long sm = __ballot(same);
        int base = 0;
        if (lane == leader) base = atomicAdd(&d.pcur[lp], __popcll(sm));
        base = __shfl(base, leader);
        if (same) {
            const int slot = base + __popcll(sm & ((1ull << lane) - 1ull));
            d.pedge[d.poff[ep] + slot] = j;
            len = slot + 1;
            pending = false;
        }
    }
    // the longest list: one atomic per wavefront
    len = lx_wave_max_i(len);
    if ((threadIdx.x & 63) == 0 && len > 0) atomicMax(d.scal + FLAT_MAXLIST, len);
}

// Maps (round 6): the per-keyframe counts AND every edge's place in its keyframe's (still unordered) list from ONE pass whose device-memory atomics are per
// (workgroup, keyframe) -- a workgroup's 2 048 consecutive edges are sorted by landmark and meet ~50-100 keyframes, which it counts in an LDS hash table, reserves
// [base, base + count) of each in d.pcnt with one returning atomic, and files base + (rank inside the workgroup) per edge in d.erel.  flat_pose_fill_kernel is then a
// plain map.  (27.5 M observations, 50 000 keyframes: flat_edge_kernel's one atomic per edge + flat_pose_list_kernel's one per (wavefront, keyframe) were 3.1 + 4.9 ms.)
#define FPC_EPT 8
#define FPC_TILE (256 * FPC_EPT)
#define FPC_SLOTS 4096
__global__ __launch_bounds__(256) void flat_pose_count_kernel(BAFlattenDev d, int nE)
{
    __shared__ int hkey[FPC_SLOTS], hcnt[FPC_SLOTS];
    __shared__ int wg_max;
    if (threadIdx.x == 0) wg_max = 0;
    for (int i = threadIdx.x; i < FPC_SLOTS; i += 256) { hkey[i] = -1; hcnt[i] = 0; }
    __syncthreads();
    const int j0 = blockIdx.x * FPC_TILE + threadIdx.x;
    int slot[FPC_EPT], rank[FPC_EPT];
#pragma unroll
    for (int u = 0; u < FPC_EPT; u++) {
        const int j = j0 + u * 256;
        const int ep = j < nE ? d.e_pose[j] : -1;
        slot[u] = -1; rank[u] = 0;
        if (ep < 0) continue;
        unsigned int h = ((unsigned int)ep * 2654435761u) >> 20;           // 12 bits
        while (true) {
            const int old = atomicCAS(&hkey[h], -1, ep);
            if (old == -1 || old == ep) break;
            h = (h + 1) & (FPC_SLOTS - 1);
        }
        slot[u] = (int)h; rank[u] = atomicAdd(&hcnt[h], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < FPC_SLOTS; i += 256) {
        const int k = hkey[i];
        if (k < 0) continue;
        const int c = hcnt[i], base = atomicAdd(&d.pcnt[k], c);
        hcnt[i] = base;
        atomicMax(&wg_max, base + c);                                      // (in LDS first: one device atomic per workgroup on the shared word -- a million of them took 2.2 ms)
    }
    __syncthreads();
    if (threadIdx.x == 0 && wg_max > 0) atomicMax(d.scal + FLAT_MAXLIST, wg_max);
#pragma unroll
    for (int u = 0; u < FPC_EPT; u++) {
        const int j = j0 + u * 256;
        if (slot[u] >= 0) d.erel[j] = hcnt[slot[u]] + rank[u];
    }
}
__global__ __launch_bounds__(256) void flat_pose_fill_kernel(BAFlattenDev d, int nE)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nE) return;
    const int ep = d.e_pose[j];
    if (ep >= 0) d.pedge[d.poff[ep] + d.erel[j]] = j;
}
void flat_launch_pose_count(const BAFlattenDev& d, int nE, hipStream_t s)
{
    if (nE > 0) hipLaunchKernelGGL(flat_pose_count_kernel, dim3((nE + FPC_TILE - 1) / FPC_TILE), dim3(256), 0, s, d, nE);
}
void flat_launch_pose_fill(const BAFlattenDev& d, int nE, hipStream_t s)
{
    if (nE > 0) hipLaunchKernelGGL(flat_pose_fill_kernel, dim3((nE + 255) / 256), dim3(256), 0, s, d, nE);
}

// one workgroup per free keyframe: its edge list ascending (the order the serial flattening produces), the landmark of every entry (ascending per keyframe
// because the edges are sorted by landmark; fixed landmarks, -1, last)
template <int CAP>
__global__ __launch_bounds__(256) void flat_pose_sort_kernel(BAFlattenDev d)
{
    __shared__ int key[CAP];
    const int k = blockIdx.x;
    const int i0 = d.poff[k], n = d.poff[k + 1] - i0;
    int P = 1; while (P < n) P <<= 1;
    for (int i = threadIdx.x; i < P; i += 256) key[i] = i < n ? d.pedge[i0 + i] : 0x7FFFFFFF;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += 256) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const int a = key[lo], b = key[hi];
                if ((a > b) == up) { key[lo] = b; key[hi] = a; }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < n; i += 256) {
        const int j = key[i];
        d.pedge[i0 + i] = j;
        d.plm[i0 + i] = d.e_point[j];
    }
}

// Block row k of the reduced camera system = the free keyframes that share a landmark with keyframe k (and k itself; block_solver.hpp:262-292), as a
// bitmap over the keyframes in LDS.  FILL = false: blocks per row and blocks on / above the diagonal; FILL = true: column indices (ascending), the slot of
// the diagonal block, and (slot, k, q, -) of every block on / above the diagonal in slot order.
template <bool FILL>
__global__ __launch_bounds__(256) void flat_rows_kernel(BAFlattenDev d, int nP)
{
    extern __shared__ unsigned int bits[];
    __shared__ int wsum[4];
    __shared__ int carry[2];
    const int k = blockIdx.x;
    const int nw = (nP + 31) >> 5;
    for (int w = threadIdx.x; w < nw; w += 256) bits[w] = 0u;
    if (threadIdx.x < 2) carry[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x == 0) atomicOr(&bits[k >> 5], 1u << (k & 31));
    for (int ii = d.poff[k] + threadIdx.x; ii < d.poff[k + 1]; ii += 256) {
        const int l = d.plm[ii];
        if (l < 0) continue;
        const int e0 = d.loff[l], kk = d.lnfree[l];
        for (int a = 0; a < kk; a++) { const int q = d.e_pose[e0 + a]; atomicOr(&bits[q >> 5], 1u << (q & 31)); }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = FILL ? d.bsr_rowptr[k] : 0, u0 = FILL ? d.ubase[k] : 0;
    int total = 0, total_u = 0;
    for (int w0 = 0; w0 < nw; w0 += 256) {
        const int w = w0 + threadIdx.x;
        unsigned int v = w < nw ? bits[w] : 0u;
        // bits of this word on / above the diagonal: columns q >= k
        unsigned int vu = v;
        if ((w << 5) + 31 < k) vu = 0u; else if ((w << 5) < k) vu = v & ~((1u << (k - (w << 5))) - 1u);
        const int c = __popc(v), cu = __popc(vu);
        if (!FILL) { total += c; total_u += cu; continue; }
        // exclusive prefix of (c, cu) over the workgroup, packed: the counts of one sweep are < 2^13 each
        int pk = c | (cu << 16), inc = pk;
        inc = lx_wave_incl_scan_i(inc);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int basep = 0;
        for (int i = 0; i < wave; i++) basep += wsum[i];
        const int ex = basep + inc - pk;
        int slot = row0 + carry[0] + (ex & 0xFFFF), us = u0 + carry[1] + (ex >> 16);
        while (v) {
            const int b = __ffs(v) - 1; v &= v - 1;
            const int q = (w << 5) + b;
            d.bsr_col[slot] = q;
            if (q == k) d.bsr_diag[k] = slot;
            if (q >= k) { d.uinfo[4 * (size_t)us] = slot; d.uinfo[4 * (size_t)us + 1] = k; d.uinfo[4 * (size_t)us + 2] = q; d.uinfo[4 * (size_t)us + 3] = 0; us++; }
            slot++;
        }
        __syncthreads();
        if (threadIdx.x == 255) { const int tot = basep + inc; carry[0] += tot & 0xFFFF; carry[1] += tot >> 16; }
        __syncthreads();
    }
    if (!FILL) {
        for (int o = 32; o > 0; o >>= 1) { total += __shfl_down(total, o); total_u += __shfl_down(total_u, o); }
        if (lane == 0) { atomicAdd(&carry[0], total); atomicAdd(&carry[1], total_u); }
        __syncthreads();
        if (threadIdx.x == 0) { d.rowcnt[k] = carry[0]; d.ucnt[k] = carry[1]; atomicMax(d.scal + FLAT_MAXROW, carry[0]); }
    }
}

void flat_launch_points(const BAFlattenDev& d, hipStream_t s)
{
    const int n = d.K > d.M ? d.K : d.M;
    if (n > 0) hipLaunchKernelGGL(flat_point_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d);
}
void flat_launch_state_in(const BAFlattenDev& d, hipStream_t s)
{
    const int n = d.K > d.M ? d.K : d.M;
    if (n > 0) hipLaunchKernelGGL(flat_state_in_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d);
}
void flat_launch_state_out(const BAFlattenDev& d, hipStream_t s)
{
    const int n = d.K > d.M ? d.K : d.M;
    if (n > 0) hipLaunchKernelGGL(flat_state_out_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d);
}
void flat_launch_edges(const BAFlattenDev& d, hipStream_t s, int few_poses)
{
    if (d.M <= 0) return;
    if (d.erel && d.E > 0) { hipLaunchKernelGGL(flat_edge_by_edge_kernel, dim3((d.E + 255) / 256), dim3(256), 0, s, d); return; }
    if (few_poses > 0 && few_poses <= 64) hipLaunchKernelGGL(flat_edge_kernel<true>, dim3((d.M + 255) / 256), dim3(256), 0, s, d, few_poses);
    else hipLaunchKernelGGL(flat_edge_kernel<false>, dim3((d.M + 255) / 256), dim3(256), 0, s, d, 0);
}
void flat_launch_pose_lists_ordered(const BAFlattenDev& d, int nP, int nE, hipStream_t s)
{
    if (nP > 0 && nE > 0) hipLaunchKernelGGL(flat_pose_lists_ordered_kernel, dim3(nP), dim3(1024), 0, s, d, nE);
}
void flat_launch_pose_lists(const BAFlattenDev& d, int nE, hipStream_t s)
{
    if (nE > 0) hipLaunchKernelGGL(flat_pose_list_kernel, dim3((nE + 255) / 256), dim3(256), 0, s, d, nE);
}
int flat_launch_pose_sort(const BAFlattenDev& d, int nP, int max_list, hipStream_t s)
{
    if (nP <= 0) return 0;
    if (max_list <= 1024) hipLaunchKernelGGL(flat_pose_sort_kernel<1024>, dim3(nP), dim3(256), 0, s, d);
    else if (max_list <= 4096) hipLaunchKernelGGL(flat_pose_sort_kernel<4096>, dim3(nP), dim3(256), 0, s, d);
    else if (max_list <= 16384) hipLaunchKernelGGL(flat_pose_sort_kernel<16384>, dim3(nP), dim3(256), 0, s, d);
    else return -1;
    return 0;
}
// one thread per block of the full pattern: row k holds the columns 0 .. nP - 1
__global__ __launch_bounds__(256) void flat_full_pattern_kernel(BAFlattenDev d, int nP)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t <= nP) d.bsr_rowptr[t] = t * nP;
    if (t >= nP * nP) return;
    const int k = t / nP, q = t - k * nP;
    d.bsr_col[t] = q;
    if (q == k) d.bsr_diag[k] = t;
    if (q >= k) {                                          // blocks on / above the diagonal in slot order: row k's start at k nP - k (k - 1) / 2
        const int us = k * nP - (k * (k - 1)) / 2 + (q - k);
        d.uinfo[4 * (size_t)us] = t; d.uinfo[4 * (size_t)us + 1] = k; d.uinfo[4 * (size_t)us + 2] = q; d.uinfo[4 * (size_t)us + 3] = 0;
    }
}
__global__ void flat_counts_kernel(BAFlattenDev d, const int* extra, int* out)
{
    if (threadIdx.x != 0) return;
    out[0] = d.lidx[d.M]; out[1] = d.eoffA[d.M]; out[2] = d.eoffB[d.M]; out[3] = d.pidx[d.K]; out[4] = d.scal[FLAT_PAIRS]; out[5] = d.edge_off[d.M];
    out[6] = extra ? *extra : 0; out[7] = 0;
}
void flat_launch_counts(const BAFlattenDev& d, const int* extra, int* out, hipStream_t s)
{
    hipLaunchKernelGGL(flat_counts_kernel, dim3(1), dim3(64), 0, s, d, extra, out);
}
void flat_launch_full_pattern(const BAFlattenDev& d, int nP, hipStream_t s)
{
    if (nP > 0) hipLaunchKernelGGL(flat_full_pattern_kernel, dim3((nP * nP + 1 + 255) / 256), dim3(256), 0, s, d, nP);
}
__global__ __launch_bounds__(256) void flat_outliers_kernel(const unsigned char* __restrict__ active, const int* __restrict__ e_src, int nE, unsigned char* __restrict__ outlier)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < nE && !active[j]) outlier[e_src[j]] = 1;
}
void flat_launch_outliers(const unsigned char* active, const int* e_src, int nE, unsigned char* outlier, hipStream_t s)
{
    if (nE > 0) hipLaunchKernelGGL(flat_outliers_kernel, dim3((nE + 255) / 256), dim3(256), 0, s, active, e_src, nE, outlier);
}
// An edge between a fixed keyframe and a fixed map point is not part of the flattened graph (g2o does not activate it, sparse_optimizer.cpp:234: its error is never computed,
// its chi2 stays 0) -- but the callers' classification loops still visit it and apply isDepthPositive() to it (Optimizer.cc:722-748, 768-797).  Neither vertex moves, so the
// verdict follows from the inputs: the classification stages are replayed on the constant depth (the device route left these edges at outlier = 0).
struct FlatStageList { int n; int check_depth[FLAT_MAX_STAGES]; int allow_reactivate[FLAT_MAX_STAGES]; };
static_assert(sizeof(FlatStageList) == sizeof(int) * (1 + 2 * FLAT_MAX_STAGES), "FlatStageList must hold every stage corb_ba_staged_device_wanted admits");
__global__ __launch_bounds__(256) void flat_fixed_edge_outliers_kernel(BAFlattenDev d, FlatStageList st, unsigned char* __restrict__ outlier)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= d.E) return;
    const CorbBAEdge ed = d.edges[e];
    if (!d.pose_fixed[ed.pose] || !d.point_fixed[ed.point]) return;
    const float* T = d.poses + 16 * (size_t)ed.pose; const float* X = d.points + 3 * (size_t)ed.point;
    const double z = (double)T[8] * X[0] + (double)T[9] * X[1] + (double)T[10] * X[2] + (double)T[11];
    int active = 1;
    for (int k = 0; k < st.n; k++) {
        if (!active && !st.allow_reactivate[k]) continue;
        active = (st.check_depth[k] && !(z > 0.0)) ? 0 : 1;                 // (the chi2 half of the test sees 0)
    }
    outlier[e] = active ? 0 : 1;
}
int flat_launch_fixed_edge_outliers(const BAFlattenDev& d, const CorbBAStage* used, int n_used, unsigned char* outlier, hipStream_t s)
{
    if (n_used < 0 || n_used > FLAT_MAX_STAGES) return -1;                 // (corb_ba_staged_device_wanted admits at most FLAT_MAX_STAGES: every stage that ran is replayed)
    FlatStageList st; st.n = n_used;
    for (int k = 0; k < st.n; k++) { st.check_depth[k] = used[k].check_depth; st.allow_reactivate[k] = used[k].allow_reactivate; }
    if (d.E > 0 && st.n > 0) hipLaunchKernelGGL(flat_fixed_edge_outliers_kernel, dim3((d.E + 255) / 256), dim3(256), 0, s, d, st, outlier);
    return 0;
}
void flat_launch_rows(const BAFlattenDev& d, int nP, bool fill, hipStream_t s)
{
    if (nP <= 0) return;
    const size_t lds = (size_t)((nP + 31) / 32) * 4;
    if (fill) hipLaunchKernelGGL(flat_rows_kernel<true>, dim3(nP), dim3(256), lds, s, d, nP);
    else hipLaunchKernelGGL(flat_rows_kernel<false>, dim3(nP), dim3(256), lds, s, d, nP);
}

// off[m] = first edge whose point index is >= m, m = 0 .. n_points (edges non-decreasing in .point: the host-array fast path of corb_ba_solve_ex)
__global__ __launch_bounds__(256) void flat_edge_offsets_kernel(const CorbBAEdge* __restrict__ edges, int n_edges, int n_points, int* __restrict__ off)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m > n_points) return;
    int a = 0, b = n_edges;
    while (a < b) { const int mid = (int)(((long long)a + b) >> 1); if (edges[mid].point < m) a = mid + 1; else b = mid; }
    off[m] = a;
}
void ba_launch_edge_offsets(const CorbBAEdge* edges, int n_edges, int n_points, int* off, hipStream_t s)
{
    hipLaunchKernelGGL(flat_edge_offsets_kernel, dim3((n_points + 1 + 255) / 256), dim3(256), 0, s, edges, n_edges, n_points, off);
}

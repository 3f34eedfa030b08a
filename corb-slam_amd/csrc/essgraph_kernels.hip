// essgraph_kernels.hip -- Optimizer::OptimizeEssentialGraph (C/src/Optimizer.cc:840-1117) flattened from store records and the covisibility graph, and its
// write-back; include/corb_essential_graph.h states the definition, essgraph_internal.h the arithmetic rule.  Small, latency-bound kernels:
//   key, rank    which slot holds which keyframe; position of every keyframe among the held ones and among the vertices in ascending id; S / snc / fixed
//   lc           the loop connections (ONE workgroup): tests, positions in (key id, member id) order, sInsertedEdges in (lo, hi) order
//   kf<false>    one wavefront per held keyframe: its edge count.  kf<true>, after the scan of the counts: the same walk, writing vi, vj, kind, measurement
//   pose, points the commit
// The only atomics are integer counters, so no output depends on the order they land in.
#include "essgraph_internal.h"
#include "covis_device.h"
#include "sim3_math.h"
#include "normal_depth.h"

// ---- the loop-edge sets: one thread, the set is at most ESS_LOOP_CAP ids ----
// op 0: insert the id of slot `other` into the set of `slot` (status 1: full, nothing written; 2: `other` holds no keyframe); op 1: clear
__global__ void ess_loop_op_kernel(EssLoopSets L, CovisStores S, int op, int slot, int other, int* status)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (op == 1) { L.n[slot] = 0; status[0] = 0; return; }
    const unsigned long long id = covis_kf(S, other)->m.id;
    if (covis_kf(S, other)->n <= 0 || corb_idtab_find(S.kfid, id) != other) { status[0] = 2; return; }
    unsigned long long* set = L.id + (size_t)slot * ESS_LOOP_CAP;
    const int n = min(max(L.n[slot], 0), ESS_LOOP_CAP);
    int p = 0;
    while (p < n && set[p] < id) p++;
    if (p < n && set[p] == id) { status[0] = 0; return; }
    if (n == ESS_LOOP_CAP) { status[0] = 1; return; }
    for (int i = n; i > p; i--) set[i] = set[i - 1];
    set[p] = id; L.n[slot] = n + 1; status[0] = 0;
}
void ess_launch_loop_op(const EssLoopSets& L, const CovisStores& S, int op, int slot, int other, int* status, hipStream_t s)
{
    hipLaunchKernelGGL(ess_loop_op_kernel, dim3(1), dim3(64), 0, s, L, S, op, slot, other, status);
}

// ---- vertices ----
__global__ __launch_bounds__(COVIS_T) void ess_key_kernel(CovisStores S, EssPlanDev d)
{
    const int x = blockIdx.x * COVIS_T + threadIdx.x;
    if (x >= S.kf_capacity) return;
    const KfHeader* h = covis_kf(S, x);
    const bool held = h->n > 0 && corb_idtab_find(S.kfid, h->m.id) == x;
    d.key[x] = held ? h->m.id : COVIS_NO_ID;
    d.bad[x] = held && (h->m.flags & CORB_KF_BAD) ? 1 : 0;
}
__device__ __forceinline__ void ess_sim3_from_pose(const float* T, S3State& S)
{
    const double R[9] = { T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10] };              // Converter::toMatrix3d / toVector3d (:887-889)
    quat_from_R(R, S.q);
    S.t[0] = T[3]; S.t[1] = T[7]; S.t[2] = T[11]; S.s = 1.0;
}
// a thread per slot: its rank among the held keyframes and among the vertices by counting the smaller ids (tiles of the keys through LDS)
__global__ __launch_bounds__(COVIS_T) void ess_rank_kernel(CovisStores S, EssPlanDev d)
{
    __shared__ unsigned long long sk[COVIS_T];
    __shared__ unsigned char sb[COVIS_T];
    const int x = blockIdx.x * COVIS_T + threadIdx.x;
    const unsigned long long mine = x < S.kf_capacity ? d.key[x] : COVIS_NO_ID;
    int hr = 0, vr = 0, H = 0, K = 0;
    for (int base = 0; base < S.kf_capacity; base += COVIS_T) {
        const int y = base + threadIdx.x;
        sk[threadIdx.x] = y < S.kf_capacity ? d.key[y] : COVIS_NO_ID;
        sb[threadIdx.x] = y < S.kf_capacity ? d.bad[y] : 0;
        __syncthreads();
        const int m = min(COVIS_T, S.kf_capacity - base);
        for (int i = 0; i < m; i++) {
            const unsigned long long k = sk[i];
            if (k == COVIS_NO_ID) continue;
            const int good = sb[i] ? 0 : 1;
            H++; K += good;
            if (k < mine) { hr++; vr += good; }
        }
        __syncthreads();
    }
    if (x >= S.kf_capacity) return;
    if (x == 0) { d.head[ESS_H_VERTICES] = K; d.head[ESS_H_HELD] = H; }
    if (mine == COVIS_NO_ID) { d.hrank[x] = -1; d.vrank[x] = -1; return; }
    d.hrank[x] = hr; d.hslot[hr] = x;
    if (d.bad[x]) { d.vrank[x] = -1; return; }
    d.vrank[x] = vr; d.vslot[vr] = x;
    const KfHeader* h = covis_kf(S, x);
    const int c = d.cpos[x];
    S3State s;
    if (c >= 0) {                                                                               // :880-884
        for (int k = 0; k < 8; k++) { d.S[(size_t)vr * 8 + k] = d.corr[(size_t)c * 8 + k]; d.snc[(size_t)vr * 8 + k] = d.ncorr[(size_t)c * 8 + k]; }
    } else {                                                                                    // :887-891
        float T[16];
#pragma unroll
        for (int k = 0; k < 16; k++) T[k] = h->m.Tcw[k];
        ess_sim3_from_pose(T, s);
        s3_store(s, d.S + (size_t)vr * 8); s3_store(s, d.snc + (size_t)vr * 8);
    }
    d.fixed[vr] = x == d.loop_slot || (h->m.flags & CORB_KF_FIXED) ? 1 : 0;                      // :894
}

// the slot that holds the keyframe `id`, or -1
__device__ __forceinline__ int ess_held(const CovisStores& S, unsigned long long id)
{
    if (id == COVIS_NO_ID) return -1;
    const int x = corb_idtab_find(S.kfid, id);
    return x >= 0 && x < S.kf_capacity ? x : -1;
}
__device__ __forceinline__ bool ess_pair_less(unsigned long long a0, unsigned long long a1, unsigned long long b0, unsigned long long b1) { return a0 < b0 || (a0 == b0 && a1 < b1); }
// Sji = Sjw * Swi (:927, :974, :1001, :1032) from the two 8-double values
__device__ __forceinline__ void ess_measure(const double* Siw, const double* Sjw, double* out)
{
    S3State si, sj, swi, sji;
    s3_load(Siw, si); s3_load(Sjw, sj);
    s3_inv(si, swi);
    s3_mul(sj, swi, sji);
    s3_store(sji, out);
}

// ---- the loop connections (:912-940): one workgroup, a thread takes pairs in strides ----
__global__ __launch_bounds__(COVIS_T) void ess_lc_kernel(CovisRows R, CovisStores S, EssPlanDev d)
{
    __shared__ int sh[4];                                                                       // emitted, dropped, below the weight
    const int tid = threadIdx.x, P = d.n_pairs;
    if (tid < 4) sh[tid] = 0;
    __syncthreads();
    for (int p = tid; p < P; p += COVIS_T) {
        const int i = d.lc_i[p], j = d.lc_j[p];
        int flag;
        if (d.key[i] == COVIS_NO_ID || d.key[j] == COVIS_NO_ID) flag = 2;                         // pKF / *sit is NULL
        else {
            int w = 0;                                                                          // pKF->GetWeight(*sit) (KeyFrame.cc:262-269)
            const int n = min(max(R.n_all[i], 0), R.M);
            for (int k = 0; k < n; k++) if (R.all_id[(size_t)i * R.M + k] == d.key[j]) { w = R.all_w[(size_t)i * R.M + k]; break; }
            if ((i != d.cur_slot || j != d.loop_slot) && w < d.min_weight) flag = 0;            // :923
            else flag = d.vrank[i] < 0 || d.vrank[j] < 0 ? 2 : 1;
        }
        d.lc_flag[p] = flag;
        atomicAdd(&sh[flag == 1 ? 0 : (flag == 2 ? 1 : 2)], 1);
    }
    __threadfence();
    __syncthreads();
    for (int p = tid; p < P; p += COVIS_T) {
        if (d.lc_flag[p] != 1) continue;
        const unsigned long long a0 = d.key[d.lc_i[p]], a1 = d.key[d.lc_j[p]];
        const unsigned long long lo = a0 < a1 ? a0 : a1, hi = a0 < a1 ? a1 : a0;
        int pos = 0, ipos = 0;
        for (int q = 0; q < P; q++) {
            if (d.lc_flag[q] != 1) continue;
            const unsigned long long b0 = d.key[d.lc_i[q]], b1 = d.key[d.lc_j[q]];
            if (ess_pair_less(b0, b1, a0, a1)) pos++;
            const unsigned long long ql = b0 < b1 ? b0 : b1, qh = b0 < b1 ? b1 : b0;
            if (ess_pair_less(ql, qh, lo, hi) || (ql == lo && qh == hi && q < p)) ipos++;
        }
        d.lc_pos[p] = pos;
        d.ins[(size_t)ipos * 2] = lo; d.ins[(size_t)ipos * 2 + 1] = hi;                          // :938
    }
    if (tid == 0) { d.head[ESS_H_KIND] = sh[0]; d.head[ESS_H_DROPPED] = sh[1]; d.head[ESS_H_LC_BELOW] = sh[2]; d.n_ins[0] = sh[0]; }
}
__global__ __launch_bounds__(COVIS_T) void ess_lc_fill_kernel(EssPlanDev d)
{
    const int p = blockIdx.x * COVIS_T + threadIdx.x;
    if (p >= d.n_pairs || d.lc_flag[p] != 1 || d.lc_pos[p] >= d.n_edges) return;
    const int e = d.lc_pos[p], vi = d.vrank[d.lc_i[p]], vj = d.vrank[d.lc_j[p]];
    d.vi[e] = vi; d.vj[e] = vj; d.kind[e] = 0;
    ess_measure(d.S + (size_t)vi * 8, d.S + (size_t)vj * 8, d.meas + (size_t)e * 8);            // the vertex values on both ends (:917-927)
}

// sorted ids a[0 .. n): is `id` among them
__device__ __forceinline__ bool ess_find_sorted(const unsigned long long* a, int n, unsigned long long id)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < id) lo = mid + 1; else hi = mid; }
    return lo < n && a[lo] == id;
}
__device__ __forceinline__ bool ess_find_pair(const unsigned long long* a, int n, unsigned long long k0, unsigned long long k1)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (ess_pair_less(a[(size_t)mid * 2], a[(size_t)mid * 2 + 1], k0, k1)) lo = mid + 1; else hi = mid; }
    return lo < n && a[(size_t)lo * 2] == k0 && a[(size_t)lo * 2 + 1] == k1;
}
__device__ __forceinline__ int ess_lanes_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// ---- the second loop (:943-1043): one wavefront per held keyframe, in ascending id ----
template <bool FILL>
__global__ __launch_bounds__(COVIS_T) void ess_kf_kernel(CovisRows R, CovisTree T, CovisStores S, EssPlanDev d)
{
    const int lane = threadIdx.x & 63, hk = blockIdx.x * (COVIS_T / 64) + (threadIdx.x >> 6);
    if (hk >= d.head[ESS_H_HELD]) return;                                                        // (uniform per wavefront)
    const int x = d.hslot[hk], M = R.M;
    const unsigned long long self = d.key[x];
    const int vself = d.vrank[x];
    int e = FILL ? d.head[ESS_H_KIND] + d.off[hk] : 0;                                           // next edge index (FILL) / edges so far
    int dropped = 0, n1 = 0, n2 = 0, n3 = 0, sup[6] = { 0, 0, 0, 0, 0, 0 };
    // the tree edge (:958-983)
    const unsigned long long parent = T.parent[x];
    const int px = ess_held(S, parent);
    if (px >= 0) {
        if (vself >= 0 && d.vrank[px] >= 0) {
            if (FILL && lane == 0 && e < d.n_edges) {
                d.vi[e] = vself; d.vj[e] = d.vrank[px]; d.kind[e] = 1;
                ess_measure(d.snc + (size_t)vself * 8, d.snc + (size_t)d.vrank[px] * 8, d.meas + (size_t)e * 8);
            }
            e++; n1++;
        } else dropped++;
    }
    // the loop edges (:986-1009): the held ones of smaller id, ascending
    const unsigned long long* lset = d.loops.id + (size_t)x * ESS_LOOP_CAP;
    const int nl = min(max(d.loops.n[x], 0), ESS_LOOP_CAP);
    {
        const unsigned long long lid = lane < nl ? lset[lane] : COVIS_NO_ID;
        const int y = lane < nl && lid < self ? ess_held(S, lid) : -1;
        const bool emit = y >= 0 && vself >= 0 && d.vrank[y] >= 0, drop = y >= 0 && !emit;
        const unsigned long long me = __ballot(emit), md = __ballot(drop);
        if (FILL && emit && e + ess_lanes_below(me, lane) < d.n_edges) {              // (the count made the room: the guard never fires)
            const int k = e + ess_lanes_below(me, lane), vj = d.vrank[y];
            d.vi[k] = vself; d.vj[k] = vj; d.kind[k] = 2;
            ess_measure(d.snc + (size_t)vself * 8, d.snc + (size_t)vj * 8, d.meas + (size_t)k * 8);
        }
        e += __popcll(me); n2 += __popcll(me); dropped += __popcll(md);
    }
    // the covisibility edges (:1012-1042) over GetCovisiblesByWeight(min_weight): the prefix of the ordered list whose weights reach it, nothing when all do
    const int n = min(max(R.n_ord[x], 0), M);
    const size_t row = (size_t)x * M;
    int reach = 0;
    for (int b = 0; b < n; b += 64) reach += __popcll(__ballot(b + lane < n && R.ord_w[row + b + lane] >= d.min_weight));
    const int keep = reach == n ? 0 : reach;
    const unsigned long long* cset = T.child_id + row;
    const int nc = min(max(T.n_child[x], 0), M), ni = d.n_ins[0];
    for (int b = 0; b < keep; b += 64) {
        const int i = b + lane;
        int why = -1; bool cand = false; int y = -1;
        if (i < keep) {
            const unsigned long long nid = R.ord_id[row + i];
            y = ess_held(S, nid);
            if (y >= 0) {                                                                       // pKFn (:1016)
                if (px >= 0 && nid == parent) why = 0;
                else if (ess_find_sorted(cset, nc, nid)) why = 1;
                else if (ess_find_sorted(lset, nl, nid)) why = 2;
                else if (d.bad[y]) why = 3;                                                     // :1018
                else if (!(nid < self)) why = 4;
                else if (ess_find_pair(d.ins, ni, nid, self)) why = 5;                          // :1020
                else cand = true;
            }
        }
        const bool emit = cand && vself >= 0;
        const unsigned long long me = __ballot(emit), md = __ballot(cand && !emit);
        if (FILL && emit && e + ess_lanes_below(me, lane) < d.n_edges) {              // (the count made the room: the guard never fires)
            const int k = e + ess_lanes_below(me, lane), vj = d.vrank[y];
            d.vi[k] = vself; d.vj[k] = vj; d.kind[k] = 3;
            ess_measure(d.snc + (size_t)vself * 8, d.snc + (size_t)vj * 8, d.meas + (size_t)k * 8);
        }
        e += __popcll(me); n3 += __popcll(me); dropped += __popcll(md);
        if (!FILL) {
#pragma unroll
            for (int r = 0; r < 6; r++) sup[r] += __popcll(__ballot(why == r));
        }
    }
    if (!FILL && lane == 0) {
        d.cnt[hk] = e;
        if (n1) atomicAdd(&d.head[ESS_H_KIND + 1], n1);
        if (n2) atomicAdd(&d.head[ESS_H_KIND + 2], n2);
        if (n3) atomicAdd(&d.head[ESS_H_KIND + 3], n3);
        if (dropped) atomicAdd(&d.head[ESS_H_DROPPED], dropped);
#pragma unroll
        for (int r = 0; r < 6; r++) if (sup[r]) atomicAdd(&d.head[ESS_H_SUPPRESSED + r], sup[r]);
    }
}

void ess_launch_count(const CovisRows& R, const CovisTree& T, const CovisStores& S, const EssPlanDev& d, hipStream_t s)
{
    const int blocks = (S.kf_capacity + COVIS_T - 1) / COVIS_T;
    hipLaunchKernelGGL(ess_key_kernel, dim3(blocks), dim3(COVIS_T), 0, s, S, d);
    hipLaunchKernelGGL(ess_rank_kernel, dim3(blocks), dim3(COVIS_T), 0, s, S, d);
    hipLaunchKernelGGL(ess_lc_kernel, dim3(1), dim3(COVIS_T), 0, s, R, S, d);
    hipLaunchKernelGGL(ess_kf_kernel<false>, dim3((S.kf_capacity + COVIS_T / 64 - 1) / (COVIS_T / 64)), dim3(COVIS_T), 0, s, R, T, S, d);
    corb_launch_exclusive_scan(d.cnt, d.off, (size_t)S.kf_capacity, d.scan_scratch, s);
}
void ess_launch_fill(const CovisRows& R, const CovisTree& T, const CovisStores& S, const EssPlanDev& d, hipStream_t s)
{
    if (d.n_pairs > 0) hipLaunchKernelGGL(ess_lc_fill_kernel, dim3((d.n_pairs + COVIS_T - 1) / COVIS_T), dim3(COVIS_T), 0, s, d);
    hipLaunchKernelGGL(ess_kf_kernel<true>, dim3((S.kf_capacity + COVIS_T / 64 - 1) / (COVIS_T / 64)), dim3(COVIS_T), 0, s, R, T, S, d);
}

// ---- the commit ----
// SE3 recovery (:1053-1076): a thread per vertex
__global__ __launch_bounds__(COVIS_T) void ess_pose_kernel(CovisStores S, EssPlanDev d, int K, const double* __restrict__ V)
{
    const int r = blockIdx.x * COVIS_T + threadIdx.x;
    if (r >= K) return;
    KfHeader* h = const_cast<KfHeader*>(covis_kf(S, d.vslot[r]));
    if (h->m.flags & CORB_KF_FIXED) return;                                                     // :1057
    S3State s; s3_load(V + (size_t)r * 8, s);
    double Rm[9]; quat_to_R(s.q, Rm);
    const double is = 1. / s.s;                                                                 // eigt *= (1./s) (:1070)
    float* T = h->m.Tcw;
#pragma unroll
    for (int a = 0; a < 3; a++) { T[a * 4] = (float)Rm[a * 3]; T[a * 4 + 1] = (float)Rm[a * 3 + 1]; T[a * 4 + 2] = (float)Rm[a * 3 + 2]; T[a * 4 + 3] = (float)(s.t[a] * is); }
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
    atomicAdd(&d.head[ESS_H_POSES], 1);
}
struct EssPoseLookup {                                                                          // the committed poses: the records as they stand now
    const CovisStores& S;
    __device__ __forceinline__ int find(unsigned long long id) const { return ess_held(S, id); }
    __device__ __forceinline__ const float* pose(int x) const { return covis_kf(S, x)->m.Tcw; }
    __device__ __forceinline__ const char* record(int x) const { return S.kf_base + (size_t)x * S.kf_bytes; }
};
// the points (:1079-1115): a thread per slot of the map-point index
__global__ __launch_bounds__(COVIS_T) void ess_points_kernel(CovisStores S, EssPlanDev d, const double* __restrict__ V0, const double* __restrict__ V, int mp_first, int mp_n, float scale_factor)
{
    __shared__ int sh[4];
    if (threadIdx.x < 4) sh[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * COVIS_T + threadIdx.x;
    if (i < mp_n) {
        char* rec = const_cast<char*>(S.mp_base) + (size_t)(mp_first + i) * S.mp_bytes;
        CorbMapPointRecord* h = reinterpret_cast<CorbMapPointRecord*>(rec);
        const MpLayout ML(S.O); const RecLayout KL(S.F);
        if (!(h->flags & (CORB_MP_BAD | CORB_MP_FIXED))) {                                      // :1084
            const CorbMapPointScratch* sc = reinterpret_cast<const CorbMapPointScratch*>(rec + ML.scratch);
            const unsigned long long idr = sc->corrected_by_kf == covis_kf(S, d.cur_slot)->m.id ? sc->corrected_reference : h->ref_kf_id;      // :1088-1098
            if (idr == CORB_NO_MAP_POINT) atomicAdd(&sh[2], 1);
            else {
                const int x = ess_held(S, idr);
                const int r = x >= 0 ? d.vrank[x] : -1;
                if (r < 0) atomicAdd(&sh[1], 1);
                else {
                    S3State srw, fin, swr;
                    s3_load(V0 + (size_t)r * 8, srw); s3_load(V + (size_t)r * 8, fin); s3_inv(fin, swr);
                    const double p[3] = { (double)h->world_pos[0], (double)h->world_pos[1], (double)h->world_pos[2] };
                    double a[3], c[3];
                    s3_map(srw, p, a); s3_map(swr, a, c);                                       // correctedSwr.map(Srw.map(eigP3Dw)) (:1106)
                    h->world_pos[0] = (float)c[0]; h->world_pos[1] = (float)c[1]; h->world_pos[2] = (float)c[2];
                    atomicAdd(&sh[0], 1);
                    if (covis_kf(S, x)->m.flags & CORB_KF_FIXED) atomicAdd(&sh[3], 1);
                    if (scale_factor > 0.f)                                                     // :1112
                        corb_update_normal_depth(EssPoseLookup{S}, h, reinterpret_cast<const unsigned long long*>(rec + ML.obs_kf), reinterpret_cast<const uint32_t*>(rec + ML.obs_idx),
                                                 covis_n_obs(S, rec), KL, scale_factor);
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sh[0]) atomicAdd(&d.head[ESS_H_MOVED], sh[0]);
        if (sh[1]) atomicAdd(&d.head[ESS_H_KEPT], sh[1]);
        if (sh[2]) atomicAdd(&d.head[ESS_H_SKIPPED], sh[2]);
        if (sh[3]) atomicAdd(&d.head[ESS_H_FIXED_REF], sh[3]);
    }
}
void ess_launch_commit(const CovisStores& S, const EssPlanDev& d, int K, const double* V0, const double* V, int mp_first, int mp_n, float scale_factor, hipStream_t s)
{
    if (K > 0) hipLaunchKernelGGL(ess_pose_kernel, dim3((K + COVIS_T - 1) / COVIS_T), dim3(COVIS_T), 0, s, S, d, K, V);
    if (mp_n > 0) hipLaunchKernelGGL(ess_points_kernel, dim3((mp_n + COVIS_T - 1) / COVIS_T), dim3(COVIS_T), 0, s, S, d, V0, V, mp_first, mp_n, scale_factor);
}

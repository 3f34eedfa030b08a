// localmap_kernels.hip -- Tracking::UpdateLocalKeyFrames / UpdateLocalPoints (C/src/Tracking.cc:1218-1366) on store records, the covisibility rows and the spanning
// tree.  Integer work; every walk the reference makes over a pointer-keyed container is made in ascending keyframe id, so no result depends on the order the atomics
// land in: the vote is a sum per slot, the voters are sorted by id, and the neighbour walk is sequential on one wavefront.
#include "localmap_internal.h"
#include "covis_device.h"

extern __shared__ unsigned long long localmap_lds[];

size_t localmap_lds_bytes(int M) { const size_t P = (size_t)covis_pow2(M); return P * 8 + 3 * P * 4; }

__device__ __forceinline__ int localmap_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ bool localmap_kf_bad(const CovisStores& S, int x) { return (covis_kf(S, x)->m.flags & CORB_KF_BAD) != 0; }
// the slot of a keyframe the store holds, or -1
__device__ __forceinline__ int localmap_held(const CovisStores& S, unsigned long long id)
{
    if (id == COVIS_NO_ID) return -1;
    const int x = corb_idtab_find(S.kfid, id);
    return x >= 0 && x < S.kf_capacity ? x : -1;
}
// the first lane of the wavefront whose candidate is set: its value to every lane, or -1
__device__ __forceinline__ int localmap_first(bool cand, int value)
{
    const unsigned long long m = __ballot(cand);
    if (!m) return -1;
    return __shfl(value, __ffsll((long long)m) - 1);
}

__global__ __launch_bounds__(COVIS_T) void localmap_vote_walk_kernel(CovisRows R, CovisTree T, CovisStores S, LocalMapDev d)
{
    const int M = R.M, P = covis_pow2(M), tid = threadIdx.x;
    unsigned long long* sid = localmap_lds;                // [P] the voters' ids
    int* sslot = reinterpret_cast<int*>(sid + P);          // [P] their slots
    int* pos = sslot + P;                                  // [P]
    int* good = pos + P;                                   // [P]
    __shared__ int sh_n, sh_cleared, sh_scan[COVIS_T / 64];
    __shared__ unsigned long long sh_best;
    if (tid == 0) { sh_n = 0; sh_cleared = 0; sh_best = 0ull; }
    __syncthreads();
    // ---- the vote (:1262-1281): lanes over the frame's features ----
    const KfHeader* fh = reinterpret_cast<const KfHeader*>(d.frame_rec);
    const int n = min(max(fh->n, 0), d.F_frame);
    const RecLayout FL(d.F_frame); const MpLayout ML(S.O);
    const unsigned long long* mp_id = reinterpret_cast<const unsigned long long*>(d.frame_rec + FL.mp_id);
    int cleared = 0;
    for (int i = tid; i < n; i += COVIS_T) {
        const unsigned long long id = mp_id[i];
        if (id == CORB_NO_MAP_POINT) continue;
        const int ms = corb_idtab_find(S.mpid, id);
        if (ms < 0 || ms >= S.mp_capacity) continue;                                         // getMapPoint() is NULL: the id stays
        const char* r = S.mp_base + (size_t)ms * S.mp_bytes;
        if (reinterpret_cast<const CorbMapPointRecord*>(r)->flags & CORB_MP_BAD) { cleared++; continue; }      // mvpMapPoints[i] = nullptr (:1278), by the finish kernel
        const unsigned long long* okf = reinterpret_cast<const unsigned long long*>(r + ML.obs_kf);
        const int no = covis_n_obs(S, r);
        for (int k = 0; k < no; k++) {                                                       // GetObservations(): the keyframes the store holds
            const int x = localmap_held(S, okf[k]);
            if (x >= 0) atomicAdd(&d.votes[x], 1);                                           // keyframeCounter[it->first]++
        }
    }
    if (cleared) atomicAdd(&sh_cleared, cleared);
    __threadfence();
    __syncthreads();
    LocalMapHead* head = d.head;
    for (int x = tid; x < S.kf_capacity; x += COVIS_T) if (localmap_load(&d.votes[x]) > 0) {
        const int j = atomicAdd(&sh_n, 1);
        if (j < P) { sid[j] = covis_kf(S, x)->m.id; sslot[j] = x; }
    }
    __syncthreads();
    const int nd = sh_n;
    if (nd > M) {                                                                            // uniform
        if (tid == 0) { head->n_kf = 0; head->n_voted = nd; head->n_mp = 0; head->ref_slot = -1; head->ref_id = COVIS_NO_ID; head->counter_empty = 0; head->n_cleared = 0; head->status = 1; head->fail = 0; }
        return;
    }
    if (nd == 0) {                                                                           // if(keyframeCounter.empty()) return; (:1282)
        for (int i = tid; i < d.n_prev; i += COVIS_T) d.kf_out[i] = d.prev[i];
        if (tid == 0) {
            head->n_kf = d.n_prev; head->n_voted = 0; head->n_mp = 0; head->ref_slot = -1; head->ref_id = COVIS_NO_ID; head->counter_empty = 1; head->n_cleared = sh_cleared;
            head->status = 0; head->fail = 0; d.counts[0] = d.n_prev;
        }
        return;
    }
    for (int i = nd + tid; i < P; i += COVIS_T) { sid[i] = COVIS_NO_ID; sslot[i] = -1; }
    __syncthreads();
    covis_sort_by_id(sid, sslot, P);
    // ---- the voters in ascending id (:1292-1307): a bad one is passed over, the rest are listed and marked; pKFmax on a strict `>` ----
    for (int i = tid; i < P; i += COVIS_T) { good[i] = i < nd && !localmap_kf_bad(S, sslot[i]) ? 1 : 0; pos[i] = good[i]; }
    __syncthreads();
    const int n_voted = covis_block_scan(pos, P, sh_scan);
    for (int i = tid; i < nd; i += COVIS_T) if (good[i]) {
        d.kf_out[pos[i]] = sslot[i];
        atomicExch(&d.mark[sslot[i]], 1);
        atomicMax(&sh_best, ((unsigned long long)(unsigned int)localmap_load(&d.votes[sslot[i]]) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)i));
    }
    __threadfence();
    __syncthreads();
    if (tid >= 64) return;
    // ---- the neighbour walk (:1310-1360): one wavefront, sequential over the voted keyframes, lanes over a keyframe's neighbours or children ----
    const int lane = tid;
    int size = n_voted;
    for (int k = 0; k < n_voted; k++) {                                                      // itEndKF is taken before the pushes
        if (size > LOCALMAP_MAX_KFS) break;
        const int x = localmap_load(&d.kf_out[k]);
        {                                                                                    // vNeighs = pKF->GetBestCovisibilityKeyFrames(10): the first 10 held
            const int no = min(max(R.n_ord[x], 0), M);
            const size_t row = (size_t)x * M;
            int held = 0, pick = -1;
            for (int base = 0; base < no && held < LOCALMAP_NEIGHBOURS && pick < 0; base += 64) {
                const int i = base + lane;
                const int xs = i < no ? localmap_held(S, R.ord_id[row + i]) : -1;
                const unsigned long long hm = __ballot(xs >= 0);
                const int rank = held + __popcll(hm & ((1ull << lane) - 1ull));
                const bool c = xs >= 0 && rank < LOCALMAP_NEIGHBOURS && !localmap_kf_bad(S, xs) && !localmap_load(&d.mark[xs]);
                pick = localmap_first(c, xs);
                held += __popcll(hm);
            }
            if (pick >= 0) { if (lane == 0) { d.kf_out[size] = pick; atomicExch(&d.mark[pick], 1); } size++; __threadfence(); }
        }
        {                                                                                    // spChilds = pKF->GetChilds(): ascending id
            const int nc = min(max(T.n_child[x], 0), M);
            const size_t row = (size_t)x * M;
            int pick = -1;
            for (int base = 0; base < nc && pick < 0; base += 64) {
                const int i = base + lane;
                const int xs = i < nc ? localmap_held(S, T.child_id[row + i]) : -1;
                const bool c = xs >= 0 && !localmap_kf_bad(S, xs) && !localmap_load(&d.mark[xs]);
                pick = localmap_first(c, xs);
            }
            if (pick >= 0) { if (lane == 0) { d.kf_out[size] = pick; atomicExch(&d.mark[pick], 1); } size++; __threadfence(); }
        }
        const int px = localmap_held(S, T.parent[x]);                                        // pKF->GetParent(): getKeyFrameInCache()
        if (px >= 0 && !localmap_load(&d.mark[px])) {
            if (lane == 0) { d.kf_out[size] = px; atomicExch(&d.mark[px], 1); }
            size++; __threadfence();
            break;                                                                           // the `break` of :1356 leaves the whole walk
        }
    }
    if (lane == 0) {
        const unsigned long long best = sh_best;
        const int bi = best ? (int)(0xFFFFFFFFu - (unsigned int)(best & 0xFFFFFFFFull)) : -1;
        head->n_kf = size; head->n_voted = n_voted; head->n_mp = 0; head->ref_slot = bi >= 0 ? sslot[bi] : -1; head->ref_id = bi >= 0 ? sid[bi] : COVIS_NO_ID;
        head->counter_empty = 0; head->n_cleared = sh_cleared; head->status = 0; head->fail = 0;
        d.counts[0] = size;
    }
}
void localmap_launch_vote_walk(const CovisRows& R, const CovisTree& T, const CovisStores& S, const LocalMapDev& d, hipStream_t s)
{
    const size_t lds = localmap_lds_bytes(R.M);
    hipLaunchKernelGGL(localmap_vote_walk_kernel, dim3(1), dim3(COVIS_T), lds, s, R, T, S, d);
}

__global__ __launch_bounds__(COVIS_T) void localmap_finish_kernel(CovisStores S, LocalMapDev d, int n_threads)
{
    const int p = blockIdx.x * COVIS_T + threadIdx.x;
    if (p >= n_threads) return;
    const LocalMapHead* head = d.head;
    const int n_kf = head->n_kf, n_mp = d.counts[1];
    const bool ok = head->status == 0 && n_kf <= d.kf_cap && n_mp <= d.mp_cap;
    if (p == 0) { d.head->n_mp = n_mp; d.head->fail = head->status == 0 && !ok ? 1 : 0; }
    if (!ok) return;                                                                         // nothing is written, the frame's record included
    if (p < n_mp) d.mp_ids[p] = reinterpret_cast<const CorbMapPointRecord*>(S.mp_base + (size_t)d.mp_out[p] * S.mp_bytes)->id;
    const int n = min(max(reinterpret_cast<const KfHeader*>(d.frame_rec)->n, 0), d.F_frame);
    if (p < n) {
        const RecLayout FL(d.F_frame);
        unsigned long long* mp_id = reinterpret_cast<unsigned long long*>(d.frame_rec + FL.mp_id);
        const unsigned long long id = mp_id[p];
        if (id != CORB_NO_MAP_POINT) {
            const int ms = corb_idtab_find(S.mpid, id);
            if (ms >= 0 && ms < S.mp_capacity && (reinterpret_cast<const CorbMapPointRecord*>(S.mp_base + (size_t)ms * S.mp_bytes)->flags & CORB_MP_BAD)) mp_id[p] = CORB_NO_MAP_POINT;
        }
    }
}
void localmap_launch_finish(const CovisStores& S, const LocalMapDev& d, int n_threads, hipStream_t s)
{
    if (n_threads < 1) n_threads = 1;
    hipLaunchKernelGGL(localmap_finish_kernel, dim3((n_threads + COVIS_T - 1) / COVIS_T), dim3(COVIS_T), 0, s, S, d, n_threads);
}

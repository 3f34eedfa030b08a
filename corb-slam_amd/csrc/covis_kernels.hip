// covis_kernels.hip -- the covisibility graph on store records (include/corb_accel.h, last section): KeyFrame::UpdateConnections / AddConnection / EraseConnection
// (C/src/KeyFrame.cc:133-168, :404-502, :685-698), the covisibility queries (:199-269), LocalMapping::KeyFrameCulling (C/src/LocalMapping.cc:590-648) and the window
// of Optimizer::LocalBundleAdjustment (C/src/Optimizer.cc:493-544).  Integer work throughout; every result is independent of the order the atomics land in: the vote
// is a sum, a row is a set of distinct ids put into the total (weight, id) order of covis_math.h, and the window lists take the FIRST position of the reference's walk
// (atomicMin) and are placed by an exclusive scan.
#include "covis_internal.h"
#include "covis_device.h"

extern __shared__ unsigned long long covis_lds[];

// sort arrays of P entries (8 + 4 bytes), the vote table of 4 P slots (8 + 4 bytes), P scan entries
size_t covis_lds_bytes(int M) { const size_t P = (size_t)covis_pow2(M); return P * 8 + 4 * P * 8 + P * 4 + 4 * P * 4 + P * 4; }

// P entries (w, id) in LDS -> descending (weight, id) (covis_before); pads carry w = -1 and sort behind every counted entry
__device__ __forceinline__ void covis_sort(unsigned long long* sid, int* sw, int P)
{
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += COVIS_T) {
                const int x = i ^ j;
                if (x > i) {
                    const bool front = (i & k) == 0;
                    const int wa = sw[i], wb = sw[x]; const unsigned long long ia = sid[i], ib = sid[x];
                    const bool swap = front ? covis_before(wb, ib, wa, ia) : covis_before(wa, ia, wb, ib);
                    if (swap) { sw[i] = wb; sw[x] = wa; sid[i] = ib; sid[x] = ia; }
                }
            }
            __syncthreads();
        }
    }
}

// ---- KeyFrame::UpdateConnections, the part that reads only records (:406-482): one workgroup per batch member ----
__global__ __launch_bounds__(COVIS_T) void covis_count_kernel(CovisStores S, const int* __restrict__ slots, int th, int M, CovisStage st)
{
    const int P = covis_pow2(M), T = 4 * P;
    unsigned long long* sid = covis_lds;                  // [P]
    unsigned long long* keys = sid + P;                   // [T]   the vote table: id -> count, open addressing
    int* sw = reinterpret_cast<int*>(keys + T);           // [P]
    int* cnt = sw + P;                                    // [T]
    int* pos = cnt + T;                                   // [P]
    __shared__ int sh_distinct, sh_full, sh_m, sh_scan[COVIS_T / 64];
    const int member = blockIdx.x, slot = slots[member], tid = threadIdx.x;
    for (int i = tid; i < T; i += COVIS_T) { keys[i] = COVIS_NO_ID; cnt[i] = 0; }
    if (tid == 0) { sh_distinct = 0; sh_full = 0; sh_m = 0; }
    __syncthreads();
    const KfHeader* h = covis_kf(S, slot);
    const unsigned long long own = h->m.id;
    const int n = covis_kf_n(S, slot);
    const RecLayout L(S.F); const MpLayout ML(S.O);
    const unsigned long long* mp_id = reinterpret_cast<const unsigned long long*>(S.kf_base + (size_t)slot * S.kf_bytes + L.mp_id);
    for (int i = tid; i < n; i += COVIS_T) {                                                 // vpMP = GetLightMapPointMatches(), :417-435
        int ms;
        const char* r = covis_good_point(S, mp_id[i], &ms);
        if (!r) continue;
        const unsigned long long* okf = reinterpret_cast<const unsigned long long*>(r + ML.obs_kf);
        const int no = covis_n_obs(S, r);
        for (int k = 0; k < no; k++) {
            const unsigned long long kid = okf[k];
            if (kid == own || kid == COVIS_NO_ID) continue;                                  // if (mit->first.mnId == mnId) continue;
            unsigned int hs = corb_idtab_hash(kid) & (unsigned int)(T - 1);
            bool done = false;
            for (int step = 0; step < T && !done; step++) {                                  // KFcounter[mit->first]++
                const unsigned long long prev = atomicCAS(&keys[hs], COVIS_NO_ID, kid);
                if (prev == COVIS_NO_ID) atomicAdd(&sh_distinct, 1);
                if (prev == COVIS_NO_ID || prev == kid) { atomicAdd(&cnt[hs], 1); done = true; }
                hs = (hs + 1) & (unsigned int)(T - 1);
            }
            if (!done) sh_full = 1;
        }
    }
    __syncthreads();
    CovisStageHead* head = st.head + member;
    const int nd = sh_distinct;
    if (nd > M || sh_full) {                                                                 // uniform over the workgroup
        if (tid == 0) { head->n_all = nd; head->n_ord = 0; head->status = 1; head->pad = 0; head->first = COVIS_NO_ID; }
        return;
    }
    for (int i = tid; i < T; i += COVIS_T) if (keys[i] != COVIS_NO_ID) { const int j = atomicAdd(&sh_m, 1); sid[j] = keys[i]; sw[j] = cnt[i]; }
    __syncthreads();
    for (int i = nd + tid; i < P; i += COVIS_T) { sid[i] = 0ull; sw[i] = -1; }
    __syncthreads();
    covis_sort(sid, sw, P);
    // the table's memory is free now: the slot each id resolves to, and the flags of the thresholded list
    int* xs = reinterpret_cast<int*>(keys);
    for (int i = tid; i < P; i += COVIS_T) {
        const int x = i < nd ? corb_idtab_find(S.kfid, sid[i]) : -1;
        xs[i] = x;
        pos[i] = x >= 0 && sw[i] >= th ? 1 : 0;                                              // KeyFrameInCache && mit->second >= th (:451, :456)
        cnt[i] = pos[i];
    }
    __syncthreads();
    const int n_ord = covis_block_scan(pos, P, sh_scan);
    const size_t row = (size_t)member * M;
    for (int i = tid; i < nd; i += COVIS_T) {
        st.all_id[row + i] = sid[i]; st.all_w[row + i] = sw[i];
        if (cnt[i]) { st.ord_id[row + pos[i]] = sid[i]; st.ord_w[row + pos[i]] = sw[i]; st.ord_slot[row + pos[i]] = xs[i]; }
    }
    if (tid == 0) {
        int no = n_ord; unsigned long long first = COVIS_NO_ID;
        if (no > 0) { int f = 0; while (!cnt[f]) f++; first = sid[f]; }                      // the front of the thresholded list: the first flagged entry
        else {                                                                               // vPairs_set.empty(): the keyframe with the maximum counter (:466-469)
            int bw = 0, bx = -1; unsigned long long bid = 0ull;
            for (int i = 0; i < nd; i++) if (xs[i] >= 0 && covis_pick_better(sw[i], sid[i], bw, bid)) { bw = sw[i]; bid = sid[i]; bx = xs[i]; }
            // (no counted keyframe in the store: the reference dereferences a NULL pKFmax here; the row then keeps its weight map and an empty list)
            if (bx >= 0) { st.ord_id[row] = bid; st.ord_w[row] = bw; st.ord_slot[row] = bx; no = 1; first = bid; }
        }
        head->n_all = nd; head->n_ord = no; head->status = 0; head->pad = 0; head->first = first;
    }
}
void covis_launch_count(const CovisStores& S, const int* slots, int n, int th, int M, const CovisStage& st, hipStream_t s)
{
    const size_t lds = covis_lds_bytes(M);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(covis_count_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(covis_count_kernel, dim3(n), dim3(COVIS_T), lds, s, S, slots, th, M, st);
}

// row x <- its entries from LDS: the weight map in order, and the ordered list rebuilt from the whole map (UpdateBestCovisibles, :150-168)
__device__ __forceinline__ void covis_store_everything(const CovisRows& R, int x, const unsigned long long* sid, const int* sw, int n)
{
    const size_t row = (size_t)x * R.M;
    for (int i = threadIdx.x; i < n; i += COVIS_T) { R.all_id[row + i] = sid[i]; R.all_w[row + i] = sw[i]; R.ord_id[row + i] = sid[i]; R.ord_w[row + i] = sw[i]; }
    if (threadIdx.x == 0) { R.n_all[x] = n; R.n_ord[x] = n; }
}
// position of `key` in the weight map of row x, or -1 (every thread gets it)
__device__ __forceinline__ int covis_row_find(const CovisRows& R, int x, int nx, unsigned long long key, int* sh_found)
{
    if (threadIdx.x == 0) *sh_found = -1;
    __syncthreads();
    const size_t row = (size_t)x * R.M;
    for (int i = threadIdx.x; i < nx; i += COVIS_T) if (R.all_id[row + i] == key) *sh_found = i;      // (ids of a row are distinct: one writer)
    __syncthreads();
    return *sh_found;
}

// ---- the spanning tree: mspChildrens is a set of ids in ascending order (std::set<LightKeyFrame>), at most M of them ----
// mspChildrens.insert(id) on slot x by the whole workgroup (sh: two ints of LDS); a full set refuses the id and sets *overflow
__device__ __forceinline__ void covis_child_insert(const CovisTree& T, int M, int x, unsigned long long id, int* overflow, int* sh)
{
    const int tid = threadIdx.x;
    if (tid == 0) { sh[0] = 0; sh[1] = 0; }
    __syncthreads();
    const int n = min(max(T.n_child[x], 0), M);
    unsigned long long* c = T.child_id + (size_t)x * M;
    unsigned long long keep[COVIS_MAX_CONNECTIONS / COVIS_T];
    int below = 0; bool found = false;
#pragma unroll
    for (int r = 0; r < COVIS_MAX_CONNECTIONS / COVIS_T; r++) {
        const int i = tid + r * COVIS_T;
        keep[r] = i < n ? c[i] : COVIS_NO_ID;
        if (i < n) { below += keep[r] < id ? 1 : 0; found = found || keep[r] == id; }
    }
    if (below) atomicAdd(&sh[0], below);
    if (found) sh[1] = 1;
    __syncthreads();
    const int pos = sh[0], present = sh[1];
    __syncthreads();
    if (present) return;
    if (n >= M) { if (tid == 0) *overflow = 1; return; }
#pragma unroll
    for (int r = 0; r < COVIS_MAX_CONNECTIONS / COVIS_T; r++) { const int i = tid + r * COVIS_T; if (i < n && keep[r] > id) c[i + 1] = keep[r]; }
    if (tid == 0) { c[pos] = id; T.n_child[x] = n + 1; }
    __threadfence_block();
    __syncthreads();
}
// mspChildrens.erase(id) on slot x
__device__ __forceinline__ void covis_child_erase(const CovisTree& T, int M, int x, unsigned long long id, int* sh)
{
    const int tid = threadIdx.x;
    if (tid == 0) sh[1] = 0;
    __syncthreads();
    const int n = min(max(T.n_child[x], 0), M);
    unsigned long long* c = T.child_id + (size_t)x * M;
    unsigned long long keep[COVIS_MAX_CONNECTIONS / COVIS_T];
    bool found = false;
#pragma unroll
    for (int r = 0; r < COVIS_MAX_CONNECTIONS / COVIS_T; r++) {
        const int i = tid + r * COVIS_T;
        keep[r] = i < n ? c[i] : COVIS_NO_ID;
        if (i < n) found = found || keep[r] == id;
    }
    if (found) sh[1] = 1;
    __syncthreads();
    const int present = sh[1];
    __syncthreads();
    if (!present) return;
#pragma unroll
    for (int r = 0; r < COVIS_MAX_CONNECTIONS / COVIS_T; r++) { const int i = tid + r * COVIS_T; if (i < n && keep[r] > id) c[i - 1] = keep[r]; }
    if (tid == 0) T.n_child[x] = n - 1;
    __threadfence_block();
    __syncthreads();
}

// ---- the commit of one batch member (:461, :468, :489-491, :493-499): a launch of 2 + (length of its ordered list) workgroups.  Workgroup 0 replaces the member's
// row, workgroup 1 + e runs AddConnection(this, weight) on the e-th keyframe of its ordered list, the last workgroup keeps the spanning tree.  The rows are distinct, so the workgroups of one launch do not meet; the members of a batch are launches in list order. ----
__global__ __launch_bounds__(COVIS_T) void covis_apply_kernel(CovisRows R, CovisTree T, CovisStores S, CovisStage st, int member, int slot, int* overflow)
{
    const int M = R.M, P = covis_pow2(M), tid = threadIdx.x;
    unsigned long long* sid = covis_lds;
    int* sw = reinterpret_cast<int*>(sid + P);
    __shared__ int sh_found;
    const CovisStageHead hd = st.head[member];
    const size_t srow = (size_t)member * M;
    if (blockIdx.x == 0) {
        const size_t row = (size_t)slot * M;
        for (int i = tid; i < hd.n_all; i += COVIS_T) { R.all_id[row + i] = st.all_id[srow + i]; R.all_w[row + i] = st.all_w[srow + i]; }
        for (int i = tid; i < hd.n_ord; i += COVIS_T) { R.ord_id[row + i] = st.ord_id[srow + i]; R.ord_w[row + i] = st.ord_w[srow + i]; }
        if (tid == 0) { R.n_all[slot] = hd.n_all; R.n_ord[slot] = hd.n_ord; }
        return;
    }
    const int e = blockIdx.x - 1;
    if (e == hd.n_ord) {                                                                     // the last workgroup: the spanning tree (:493-499); it touches no row
        __shared__ int sh_ins[2];
        const unsigned long long own = covis_kf(S, slot)->m.id;
        if (hd.n_ord <= 0 || !T.first[slot] || own == 0ull) return;                           // if (mbFirstConnection && mnId != 0)
        // (the front and its slot were staged before the earlier members of the batch were committed; they are still "as if one after the other" because a member's
        // ordered list comes from its own counter over the records alone -- no commit of another member changes it)
        const int px = st.ord_slot[srow];
        if (tid == 0) T.parent[slot] = st.ord_id[srow];                                      // mpParent = mvpOrderedConnectedKeyFrames.front();
        if (px >= 0 && px < S.kf_capacity) {                                                 // if (mpParent.getKeyFrame())
            covis_child_insert(T, M, px, own, overflow, sh_ins);
            if (tid == 0) T.first[slot] = 0;
        }
        return;
    }
    if (e > hd.n_ord) return;
    const int x = st.ord_slot[srow + e], w = st.ord_w[srow + e];
    if (x < 0 || x >= S.kf_capacity || x == slot) return;
    const unsigned long long key = covis_kf(S, slot)->m.id;
    int nx = min(max(R.n_all[x], 0), M);
    const size_t row = (size_t)x * M;
    const int found = covis_row_find(R, x, nx, key, &sh_found);
    if (found >= 0 && R.all_w[row + found] == w) return;                                     // the weight is what it was: the ordered list stays (:141-144)
    if (found < 0 && nx >= M) { if (tid == 0) *overflow = 1; return; }
    for (int i = tid; i < P; i += COVIS_T) { sid[i] = i < nx ? R.all_id[row + i] : 0ull; sw[i] = i < nx ? R.all_w[row + i] : -1; }
    __syncthreads();
    if (tid == 0) { if (found >= 0) sw[found] = w; else { sid[nx] = key; sw[nx] = w; } }
    if (found < 0) nx++;
    __syncthreads();
    covis_sort(sid, sw, P);
    covis_store_everything(R, x, sid, sw, nx);
}
void covis_launch_apply(const CovisRows& R, const CovisTree& T, const CovisStores& S, const CovisStage& st, int member, int slot, int n_ord, int* overflow, hipStream_t s)
{
    const size_t lds = (size_t)covis_pow2(R.M) * 12;
    hipLaunchKernelGGL(covis_apply_kernel, dim3(2 + n_ord), dim3(COVIS_T), lds, s, R, T, S, st, member, slot, overflow);
}

// ---- the connection part of KeyFrame::SetBadFlag (:592-595): EraseConnection(this) on the e-th keyframe of the row's weight map (:685-698) ----
__global__ __launch_bounds__(COVIS_T) void covis_erase_kernel(CovisRows R, CovisStores S, int slot)
{
    const int M = R.M, P = covis_pow2(M), tid = threadIdx.x, e = blockIdx.x;
    unsigned long long* sid = covis_lds;
    int* sw = reinterpret_cast<int*>(sid + P);
    __shared__ int sh_found;
    if (e >= min(max(R.n_all[slot], 0), M)) return;
    const int x = corb_idtab_find(S.kfid, R.all_id[(size_t)slot * M + e]);                   // if ((mit->first).getKeyFrame())
    if (x < 0 || x >= S.kf_capacity || x == slot) return;
    const unsigned long long key = covis_kf(S, slot)->m.id;
    const int nx = min(max(R.n_all[x], 0), M);
    const size_t row = (size_t)x * M;
    const int found = covis_row_find(R, x, nx, key, &sh_found);
    if (found < 0) return;                                                                   // not in the map: bUpdate stays false
    for (int i = tid; i < nx - 1; i += COVIS_T) { const int src = i < found ? i : i + 1; sid[i] = R.all_id[row + src]; sw[i] = R.all_w[row + src]; }
    __syncthreads();
    covis_store_everything(R, x, sid, sw, nx - 1);                                           // (an ordered row without one entry is still ordered)
}
void covis_launch_erase(const CovisRows& R, const CovisStores& S, int slot, hipStream_t s)
{
    const size_t lds = (size_t)covis_pow2(R.M) * 12;
    hipLaunchKernelGGL(covis_erase_kernel, dim3(R.M), dim3(COVIS_T), lds, s, R, S, slot);
}

// ---- GetVectorCovisibleKeyFrames / GetBestCovisibilityKeyFrames(N) (mode 0) and GetCovisiblesByWeight(w) (mode 1), :199-260: one workgroup ----
__global__ __launch_bounds__(COVIS_T) void covis_query_kernel(CovisRows R, CovisStores S, int slot, int N, int min_weight, int mode, int* out_slots, int* out_w, int* out_n)
{
    const int M = R.M, P = covis_pow2(M), tid = threadIdx.x;
    int* pos = reinterpret_cast<int*>(covis_lds);          // [P]
    int* xs = pos + P;                                     // [P]
    __shared__ int sh_scan[COVIS_T / 64];
    const int n = min(max(R.n_ord[slot], 0), M);
    const size_t row = (size_t)slot * M;
    for (int i = tid; i < P; i += COVIS_T) {
        const int x = i < n ? corb_idtab_find(S.kfid, R.ord_id[row + i]) : -1;
        xs[i] = x;
        pos[i] = mode == 0 ? (x >= 0 ? 1 : 0) : (i < n && R.ord_w[row + i] >= min_weight ? 1 : 0);
    }
    __syncthreads();
    const int total = covis_block_scan(pos, P, sh_scan);
    if (mode == 0) {
        const int keep = N > 0 ? min(N, total) : total;
        for (int i = tid; i < n; i += COVIS_T) if (xs[i] >= 0 && pos[i] < keep) { out_slots[pos[i]] = xs[i]; out_w[pos[i]] = R.ord_w[row + i]; }
        if (tid == 0) *out_n = keep;
    } else {
        // upper_bound(mvOrderedWeights, w, weightComp) is the first weight below w; `it == end()` returns the EMPTY vector (:252-255): a list whose every
        // weight reaches w answers nothing, as in the reference.  The list descends, so the entries that reach w are a prefix.
        const int keep = total == n ? 0 : total;
        for (int i = tid; i < keep; i += COVIS_T) { out_slots[i] = xs[i]; out_w[i] = R.ord_w[row + i]; }
        if (tid == 0) *out_n = keep;
    }
}
void covis_launch_query(const CovisRows& R, const CovisStores& S, int slot, int N, int min_weight, int mode, int* out_slots, int* out_w, int* out_n, hipStream_t s)
{
    const size_t lds = (size_t)covis_pow2(R.M) * 8;
    hipLaunchKernelGGL(covis_query_kernel, dim3(1), dim3(COVIS_T), lds, s, R, S, slot, N, min_weight, mode, out_slots, out_w, out_n);
}
// GetWeight (:262-269)
__global__ __launch_bounds__(COVIS_T) void covis_weight_kernel(CovisRows R, CovisStores S, int slot_a, int slot_b, int* out_w)
{
    __shared__ int sh_found;
    const int n = min(max(R.n_all[slot_a], 0), R.M);
    const int found = covis_row_find(R, slot_a, n, covis_kf(S, slot_b)->m.id, &sh_found);
    if (threadIdx.x == 0) *out_w = found >= 0 ? R.all_w[(size_t)slot_a * R.M + found] : 0;
}
void covis_launch_weight(const CovisRows& R, const CovisStores& S, int slot_a, int slot_b, int* out_w, hipStream_t s)
{
    hipLaunchKernelGGL(covis_weight_kernel, dim3(1), dim3(COVIS_T), 0, s, R, S, slot_a, slot_b, out_w);
}

// ---- LocalMapping::KeyFrameCulling (C/src/LocalMapping.cc:597-647): one workgroup per covisible keyframe, lanes over its features ----
__global__ __launch_bounds__(COVIS_T) void covis_culling_kernel(CovisStores S, const int* __restrict__ list, const int* __restrict__ n_list, int monocular, float th_depth,
                                                                int* n_mps, int* n_red, unsigned char* cull)
{
    __shared__ int sh_mps, sh_red;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= *n_list) return;
    if (tid == 0) { sh_mps = 0; sh_red = 0; }
    __syncthreads();
    const int slot = list[b];
    const KfHeader* h = covis_kf(S, slot);
    const RecLayout L(S.F); const MpLayout ML(S.O);
    const char* rec = S.kf_base + (size_t)slot * S.kf_bytes;
    const int n = h->m.id == 0ull ? 0 : covis_kf_n(S, slot);                                 // if (pKF->mnId == 0) continue;
    const unsigned long long* mp_id = reinterpret_cast<const unsigned long long*>(rec + L.mp_id);
    const float* depth = reinterpret_cast<const float*>(rec + L.depth);
    const CorbKeyPoint* kp = reinterpret_cast<const CorbKeyPoint*>(rec + L.kp);
    int mps = 0, red = 0;
    for (int i = tid; i < n; i += COVIS_T) {
        int ms;
        const char* r = covis_good_point(S, mp_id[i], &ms);
        if (!r) continue;
        if (covis_depth_skipped(monocular, depth[i], th_depth)) continue;
        mps++;
        const unsigned long long* okf = reinterpret_cast<const unsigned long long*>(r + ML.obs_kf);
        const uint32_t* oidx = reinterpret_cast<const uint32_t*>(r + ML.obs_idx);
        const int no = covis_n_obs(S, r);
        const int octave = kp[i].octave;
        int observations = 0, others = 0;                                                    // pMP->Observations(); nObs of :621
        for (int k = 0; k < no; k++) {
            const int x = corb_idtab_find(S.kfid, okf[k]);
            const bool held = x >= 0 && (int)oidx[k] < covis_kf_n(S, x);
            const char* xr = S.kf_base + (size_t)(held ? x : 0) * S.kf_bytes;
            observations += covis_obs_weight(held, held ? reinterpret_cast<const float*>(xr + L.ur)[oidx[k]] : -1.0f);
            if (held && x != slot && covis_octave_counts(reinterpret_cast<const CorbKeyPoint*>(xr + L.kp)[oidx[k]].octave, octave)) others++;
        }
        if (observations > COVIS_TH_OBS && others >= COVIS_TH_OBS) red++;
    }
    if (mps) atomicAdd(&sh_mps, mps);
    if (red) atomicAdd(&sh_red, red);
    __syncthreads();
    if (tid == 0) { n_mps[b] = sh_mps; n_red[b] = sh_red; cull[b] = h->m.id != 0ull && covis_cull(sh_red, sh_mps) ? 1 : 0; }
}
void covis_launch_culling(const CovisStores& S, const int* list, const int* n_list, int max_list, int monocular, float th_depth, int* n_mps, int* n_red, unsigned char* cull, hipStream_t s)
{
    hipLaunchKernelGGL(covis_culling_kernel, dim3(max_list), dim3(COVIS_T), 0, s, S, list, n_list, monocular, th_depth, n_mps, n_red, cull);
}

// ---- the window of Optimizer::LocalBundleAdjustment (C/src/Optimizer.cc:493-544) ----
// lLocalKeyFrames (:493-507): pKF, then its covisibles in list order; every one of them carries mnBALocalForKF afterwards, a bad one is not listed.  One workgroup.
__global__ __launch_bounds__(COVIS_T) void covis_window_local_kernel(CovisRows R, CovisStores S, int slot, CovisWindow w)
{
    const int M = R.M, P = covis_pow2(M), tid = threadIdx.x;
    int* pos = reinterpret_cast<int*>(covis_lds);
    int* xs = pos + P;
    __shared__ int sh_scan[COVIS_T / 64];
    const int n = min(max(R.n_ord[slot], 0), M);
    const size_t row = (size_t)slot * M;
    for (int i = tid; i < P; i += COVIS_T) {
        const int x = i < n ? corb_idtab_find(S.kfid, R.ord_id[row + i]) : -1;
        const bool in = x >= 0 && x != slot;
        xs[i] = in ? x : -1;
        if (in) w.first_kf[x] = -1;
        pos[i] = in && !(covis_kf(S, x)->m.flags & CORB_KF_BAD) ? 1 : 0;
    }
    if (tid == 0) { w.first_kf[slot] = -1; if (w.kf_cap > 0) w.kf_out[0] = slot; }
    __syncthreads();
    for (int i = tid; i < P; i += COVIS_T) if (!pos[i]) xs[i] = -1;
    __syncthreads();
    const int total = covis_block_scan(pos, P, sh_scan);
    for (int i = tid; i < n; i += COVIS_T) if (xs[i] >= 0 && 1 + pos[i] < w.kf_cap) w.kf_out[1 + pos[i]] = xs[i];
    if (tid == 0) w.counts[0] = 1 + total;
}
// candidate p = (k-th local keyframe, feature i) in the order of the walk of :511-525; returns the slot of the non-bad point it holds, or -1
__device__ __forceinline__ int covis_window_point(const CovisStores& S, const CovisWindow& w, long long p)
{
    const int k = (int)(p / S.F), i = (int)(p % S.F);
    if (k >= min(w.counts[0], w.kf_cap)) return -1;
    const int slot = w.kf_out[k];
    if (i >= covis_kf_n(S, slot)) return -1;
    const RecLayout L(S.F);
    int ms = -1;
    return covis_good_point(S, reinterpret_cast<const unsigned long long*>(S.kf_base + (size_t)slot * S.kf_bytes + L.mp_id)[i], &ms) ? ms : -1;
}
// candidate q = (j-th local point, o-th observation) in the order of the walk of :529-544; returns the slot of the observing keyframe, or -1 (pKFi is NULL)
__device__ __forceinline__ int covis_window_observer(const CovisStores& S, const CovisWindow& w, long long q)
{
    const int j = (int)(q / S.O), o = (int)(q % S.O);
    if (j >= min(w.counts[1], w.mp_cap)) return -1;
    const char* r = S.mp_base + (size_t)w.mp_out[j] * S.mp_bytes;
    if (o >= covis_n_obs(S, r)) return -1;
    const MpLayout ML(S.O);
    const int x = corb_idtab_find(S.kfid, reinterpret_cast<const unsigned long long*>(r + ML.obs_kf)[o]);
    return x >= 0 && x < S.kf_capacity ? x : -1;
}
// pass 0: every candidate offers its position to what it names (the first one stays); pass 1: flag[c] = the candidate is that first one (and is listed);
// pass 2, after the scan of the flags: the survivors take their places
__global__ __launch_bounds__(COVIS_T) void covis_window_points_kernel(CovisStores S, CovisWindow w, long long n_cand, int pass)
{
    const long long p = (long long)blockIdx.x * COVIS_T + threadIdx.x;
    if (p >= n_cand) return;
    const int ms = covis_window_point(S, w, p);
    if (pass == 0) { if (ms >= 0) atomicMin(&w.first_mp[ms], (int)p); return; }
    const bool first = ms >= 0 && w.first_mp[ms] == (int)p;                                 // pMP->mnBALocalForKF != pKF->mnId
    if (pass == 1) { w.flag[p] = first ? 1 : 0; return; }
    if (first && w.pos[p] < w.mp_cap) w.mp_out[w.pos[p]] = ms;
    if (p == 0) w.counts[1] = w.pos[n_cand];
}
__global__ __launch_bounds__(COVIS_T) void covis_window_fixed_kernel(CovisStores S, CovisWindow w, long long n_cand, int pass)
{
    const long long q = (long long)blockIdx.x * COVIS_T + threadIdx.x;
    if (q >= n_cand) return;
    const int x = covis_window_observer(S, w, q);
    if (pass == 0) { if (x >= 0) atomicMin(&w.first_kf[x], (int)q); return; }               // (a keyframe that carries mnBALocalForKF holds -1: it never matches)
    const bool first = x >= 0 && w.first_kf[x] == (int)q && !(covis_kf(S, x)->m.flags & CORB_KF_BAD);     // marked at its first observation, listed if (!pKFi->isBad())
    if (pass == 1) { w.flag[q] = first ? 1 : 0; return; }
    const int n_local = min(w.counts[0], w.kf_cap);
    if (first && n_local + w.pos[q] < w.kf_cap) w.kf_out[n_local + w.pos[q]] = x;
    if (q == 0) w.counts[2] = w.pos[n_cand];
}
void covis_launch_window(const CovisRows& R, const CovisStores& S, int slot, const CovisWindow& w, hipStream_t s)
{
    hipLaunchKernelGGL(covis_window_local_kernel, dim3(1), dim3(COVIS_T), (size_t)covis_pow2(R.M) * 8, s, R, S, slot, w);
    covis_launch_window_points(S, w, s);
    const long long n2 = (long long)w.mp_bound * S.O;
    if (n2 > 0) {
        const unsigned g2 = (unsigned)((n2 + COVIS_T - 1) / COVIS_T);
        hipLaunchKernelGGL(covis_window_fixed_kernel, dim3(g2), dim3(COVIS_T), 0, s, S, w, n2, 0);
        hipLaunchKernelGGL(covis_window_fixed_kernel, dim3(g2), dim3(COVIS_T), 0, s, S, w, n2, 1);
        corb_launch_exclusive_scan(w.flag, w.pos, (size_t)n2, w.scan_scratch, s);
        hipLaunchKernelGGL(covis_window_fixed_kernel, dim3(g2), dim3(COVIS_T), 0, s, S, w, n2, 2);
    }
}

void covis_launch_window_points(const CovisStores& S, const CovisWindow& w, hipStream_t s)
{
    const long long n1 = (long long)w.local_bound * S.F;
    if (n1 <= 0) return;
    const unsigned g1 = (unsigned)((n1 + COVIS_T - 1) / COVIS_T);
    hipLaunchKernelGGL(covis_window_points_kernel, dim3(g1), dim3(COVIS_T), 0, s, S, w, n1, 0);
    hipLaunchKernelGGL(covis_window_points_kernel, dim3(g1), dim3(COVIS_T), 0, s, S, w, n1, 1);
    corb_launch_exclusive_scan(w.flag, w.pos, (size_t)n1, w.scan_scratch, s);
    hipLaunchKernelGGL(covis_window_points_kernel, dim3(g1), dim3(COVIS_T), 0, s, S, w, n1, 2);
}

// ---- the spanning tree's calls: one workgroup each ----
__global__ __launch_bounds__(COVIS_T) void covis_tree_init_kernel(CovisTree T, int capacity)
{
    const int i = blockIdx.x * COVIS_T + threadIdx.x;
    if (i < capacity) { T.parent[i] = COVIS_NO_ID; T.first[i] = 1; T.n_child[i] = 0; }
}
void covis_launch_tree_init(const CovisTree& T, int capacity, hipStream_t s)
{
    hipLaunchKernelGGL(covis_tree_init_kernel, dim3((capacity + COVIS_T - 1) / COVIS_T), dim3(COVIS_T), 0, s, T, capacity);
}
// AddChild / EraseChild / ChangeParent (KeyFrame.cc:504-521)
__global__ __launch_bounds__(COVIS_T) void covis_tree_op_kernel(CovisRows R, CovisTree T, CovisStores S, int op, int slot, int other, int* overflow)
{
    __shared__ int sh_ins[2];
    const unsigned long long oid = covis_kf(S, other)->m.id;
    if (op == 0) covis_child_insert(T, R.M, slot, oid, overflow, sh_ins);                    // mspChildrens.insert(tLKF)
    else if (op == 1) covis_child_erase(T, R.M, slot, oid, sh_ins);                          // mspChildrens.erase(tLKF)
    else {
        if (threadIdx.x == 0) T.parent[slot] = oid;                                          // mpParent = tLKF;
        covis_child_insert(T, R.M, other, covis_kf(S, slot)->m.id, overflow, sh_ins);        // pKF->AddChild(this);
    }
}
void covis_launch_tree_op(const CovisRows& R, const CovisTree& T, const CovisStores& S, int op, int slot, int other, int* overflow, hipStream_t s)
{
    hipLaunchKernelGGL(covis_tree_op_kernel, dim3(1), dim3(COVIS_T), 0, s, R, T, S, op, slot, other, overflow);
}

// ---- the tree part of KeyFrame::SetBadFlag (:607-668): one workgroup; the rounds are sequential, the (child, connected keyframe) pairs of a round are not ----
size_t covis_reparent_lds_bytes(int M) { const size_t P = (size_t)covis_pow2(M); return P * 8 + (P + 2) * 8 + P * 4 + P * 4; }
__global__ __launch_bounds__(COVIS_T) void covis_reparent_kernel(CovisRows R, CovisTree T, CovisStores S, int slot, int* out)
{
    const int M = R.M, P = covis_pow2(M), tid = threadIdx.x;
    unsigned long long* cid = covis_lds;                       // [P]     mspChildrens of this keyframe
    unsigned long long* cand = cid + P;                        // [P + 2] sParentCandidates, the non-NULL ones
    int* cslot = reinterpret_cast<int*>(cand + P + 2);         // [P]     slot of the child, -1: getKeyFrame() is NULL
    int* remain = cslot + P;                                   // [P]     still in the set
    __shared__ unsigned long long sh_best;
    __shared__ int sh_ins[2], sh_ncand, sh_changed;
    const unsigned long long own = covis_kf(S, slot)->m.id;
    const int nc = min(max(T.n_child[slot], 0), M);
    const unsigned long long par = T.parent[slot];
    int px = par == COVIS_NO_ID ? -1 : corb_idtab_find(S.kfid, par);                         // mpParent.getKeyFrame()
    if (px >= S.kf_capacity) px = -1;
    for (int i = tid; i < nc; i += COVIS_T) {
        const unsigned long long id = T.child_id[(size_t)slot * M + i];
        const int x = corb_idtab_find(S.kfid, id);
        cid[i] = id; cslot[i] = x >= 0 && x < S.kf_capacity ? x : -1; remain[i] = 1;
    }
    if (tid == 0) { sh_ncand = 0; sh_changed = 0; if (px >= 0) { cand[0] = par; sh_ncand = 1; } }
    __syncthreads();
    int left = nc;
    for (int round = 0; round < nc; round++) {                                               // while (!mspChildrens.empty())
        if (tid == 0) sh_best = 0ull;
        __syncthreads();
        const int ncand = sh_ncand;
        for (int ci = 0; ci < nc; ci++) {                                                    // uniform over the workgroup
            if (!remain[ci]) continue;
            const int x = cslot[ci];
            if (x < 0 || (covis_kf(S, x)->m.flags & CORB_KF_BAD)) continue;                  // if (!pKF) continue; if (pKF->isBad()) continue;
            const int no = min(max(R.n_ord[x], 0), M), na = min(max(R.n_all[x], 0), M);
            const size_t row = (size_t)x * M;
            for (int i = tid; i < no; i += COVIS_T) {                                        // vpConnected = pKF->GetVectorCovisibleKeyFrames()
                const unsigned long long id = R.ord_id[row + i];
                if (corb_idtab_find(S.kfid, id) < 0) continue;
                bool is_cand = false;
                for (int k = 0; k < ncand; k++) is_cand = is_cand || cand[k] == id;          // vpConnected[i]->mnId == (*spcit)->mnId
                if (!is_cand) continue;
                int w = 0;                                                                   // pKF->GetWeight(vpConnected[i])
                for (int k = 0; k < na; k++) if (R.all_id[row + k] == id) w = R.all_w[row + k];
                // `w > max` from max = -1, children in ascending id, the list in its order: the greatest weight, of equals the first met
                atomicMax(&sh_best, ((unsigned long long)(unsigned int)(w + 1) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)(ci * M + i)));
            }
        }
        __syncthreads();
        const unsigned long long best = sh_best;
        if (best == 0ull) break;                                                             // !bContinue
        const unsigned int code = 0xFFFFFFFFu - (unsigned int)(best & 0xFFFFFFFFull);
        const int ci = (int)(code / (unsigned int)M), i = (int)(code % (unsigned int)M);
        const int xc = cslot[ci];
        const unsigned long long pid = R.ord_id[(size_t)xc * M + i], child = cid[ci];
        const int xp = corb_idtab_find(S.kfid, pid);
        __syncthreads();
        if (tid == 0) { T.parent[xc] = pid; cand[ncand] = child; sh_ncand = ncand + 1; remain[ci] = 0; sh_changed++; }      // pC->ChangeParent(pP); sParentCandidates.insert(pC); mspChildrens.erase(pC)
        if (xp >= 0 && xp < S.kf_capacity) covis_child_insert(T, M, xp, child, out + 2, sh_ins);
        left--;
        __syncthreads();
    }
    __syncthreads();
    // the set without the re-parented children, written BEFORE the fallback: a keyframe can be its own parent (two keyframes that took each other as parents, one of
    // them culled), and then the fallback's AddChild / EraseChild below work on this very set, as they do in the reference
    if (tid == 0) {
        int n = 0;
        for (int ci = 0; ci < nc; ci++) if (remain[ci]) T.child_id[(size_t)slot * M + n++] = cid[ci];
        T.n_child[slot] = n;
    }
    __threadfence_block();
    __syncthreads();
    if (left > 0 && px >= 0) {                                                               // if (!mspChildrens.empty() && mpParent.getKeyFrame())
        for (int ci = 0; ci < nc; ci++) {
            if (!remain[ci] || cslot[ci] < 0) continue;                                      // if ((*sit).getKeyFrame())
            if (tid == 0) { T.parent[cslot[ci]] = par; sh_changed++; }                       // ->ChangeParent(mpParent.getKeyFrame())
            covis_child_insert(T, M, px, cid[ci], out + 2, sh_ins);
        }
        covis_child_erase(T, M, px, own, sh_ins);                                            // mpParent.getKeyFrame()->EraseChild(this);
        if (tid == 0) out[1] = 1;                                                            // mbBad = true;
    }
    __syncthreads();
    if (tid == 0) out[0] = sh_changed;
}
void covis_launch_reparent(const CovisRows& R, const CovisTree& T, const CovisStores& S, int slot, int* out, hipStream_t s)
{
    const size_t lds = covis_reparent_lds_bytes(R.M);
    hipLaunchKernelGGL(covis_reparent_kernel, dim3(1), dim3(COVIS_T), lds, s, R, T, S, slot, out);
}

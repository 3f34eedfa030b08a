// kfinsert_kernels.hip -- keyframe insertion on store records for gfx950 (include/corb_keyframe_insert.h):
//   kfi_points_kernel : Tracking::CreateNewKeyFrame / StereoInitialization / UpdateLastFrame (C/src/Tracking.cc:1096-1158, 524-540, 830-883).  One workgroup: the
//                       (depth bits, index) keys of the frame are selected and sorted in LDS (positive floats order as unsigned integers), the serial loop's cut is
//                       a closed form of two counts (kfinsert_math.h), the kinds are read from the records, a scan numbers the created points in visit order, and
//                       -- behind a barrier, so every kind is decided from the records as they stood -- the same threads write the new MapPoint records.
//   kfi_counts_kernel : the per-feature counts of Tracking::NeedNewKeyFrame (:1013-1036): integer atomics, any order gives the same sums
//   kfi_assoc_kernel  : the association loop of LocalMapping::ProcessNewKeyFrame (C/src/LocalMapping.cc:132-151) in closed form, one workgroup; then
//   kfi_assoc_apply_kernel, one wavefront per added observation: the list, UpdateNormalAndDepth (normal_depth.h), ComputeDistinctiveDescriptors (distinctive.h)
//   kfi_cull_kernel   : LocalMapping::MapPointCulling (C/src/LocalMapping.cc:161-188).  One workgroup: first occurrences through an id table (lowest position wins),
//                       decisions from the records, an ordered compaction of the survivors, then MapPoint::SetBadFlag on the records.
// The frames are a few thousand features and the lists a few hundred points: the calls are latency bound -- a launch or two behind the keyframe index, one read-back.
#include "kfinsert_internal.h"
#include "kfinsert_math.h"
#include "normal_depth.h"
#include "distinctive.h"

namespace {

// exclusive scan of one count per thread over the workgroup (KFI_THREADS threads); *total = the sum
__device__ __forceinline__ int kfi_block_scan(int cnt, int* part, int* total)
{
    const int t = threadIdx.x;
    part[t] = cnt;
    __syncthreads();
    for (int off = 1; off < KFI_THREADS; off <<= 1) {
        const int v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const int r = part[t] - cnt;
    *total = part[KFI_THREADS - 1];
    __syncthreads();
    return r;
}

// MapPoint::Observations() from the record's list: 2 per observation whose keyframe is at hand and stereo there, 1 otherwise (corb_local_ba_store's rule)
__device__ __forceinline__ int kfi_observations(const char* mrec, int max_obs, const char* kf_base, size_t kf_bytes, const RecLayout& KL, const CorbIdTable& kfid)
{
    const MpLayout ML(max_obs);
    const CorbMapPointRecord* h = reinterpret_cast<const CorbMapPointRecord*>(mrec);
    const unsigned long long* okf = reinterpret_cast<const unsigned long long*>(mrec + ML.obs_kf); const uint32_t* oidx = reinterpret_cast<const uint32_t*>(mrec + ML.obs_idx);
    const int n = min(max(h->n_obs, 0), max_obs);
    int w = 0;
    for (int k = 0; k < n; k++) {
        const int ks = corb_idtab_find(kfid, okf[k]);
        bool at_hand = false; float ur = -1.f;
        if (ks >= 0) {
            const char* kr = kf_base + (size_t)ks * kf_bytes;
            if ((int)oidx[k] < reinterpret_cast<const KfHeader*>(kr)->n) { at_hand = true; ur = reinterpret_cast<const float*>(kr + KL.ur)[oidx[k]]; }
        }
        w += kfi_obs_weight(at_hand, ur);
    }
    return w;
}

extern __shared__ unsigned long long kfi_keys[];

__global__ __launch_bounds__(KFI_THREADS) void kfi_points_kernel(KfiPointsDev d)
{
    __shared__ int part[KFI_THREADS];
    __shared__ int sh_m, sh_near;
    const int t = threadIdx.x;
    const RecLayout KL(d.F);
    const KfHeader* hdr = reinterpret_cast<const KfHeader*>(d.rec);
    const float* depth = reinterpret_cast<const float*>(d.rec + KL.depth);
    if (t == 0) { sh_m = 0; sh_near = 0; }
    __syncthreads();
    // select: key = (z bits, i), mode 0 = feature order; the padding sorts behind every candidate (no candidate has the bits of a NaN)
    int m_loc = 0, near_loc = 0;
    for (int i = t; i < d.P; i += KFI_THREADS) {
        unsigned long long key = ~0ull;
        if (i < d.cap) {
            const float z = depth[i];
            if (kfi_is_candidate(z)) {
                key = ((d.mode == 0 ? 0ull : (unsigned long long)__float_as_uint(z)) << 32) | (unsigned long long)(unsigned int)i;
                m_loc++; near_loc += kfi_is_far(z, d.th_depth) ? 0 : 1;
            }
        }
        kfi_keys[i] = key;
    }
    if (m_loc) { atomicAdd(&sh_m, m_loc); atomicAdd(&sh_near, near_loc); }
    __syncthreads();
    // sort (bitonic network over the padded keys)
    for (int k = 2; k <= d.P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < d.P; i += KFI_THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long a = kfi_keys[i], b = kfi_keys[x];
                    if ((a > b) == ((i & k) == 0)) { kfi_keys[i] = b; kfi_keys[x] = a; }
                }
            }
            __syncthreads();
        }
    const int visited = kfi_n_visited(sh_m, sh_near, d.mode);
    // kinds: a thread owns a contiguous run of the visit order
    const int per = (visited + KFI_THREADS - 1) / KFI_THREADS;
    const int b = min(t * per, visited), e = min(b + per, visited);
    const unsigned long long* mp_id = reinterpret_cast<const unsigned long long*>(d.rec + KL.mp_id);
    int cnt = 0;
    for (int j = b; j < e; j++) {
        const int i = (int)(unsigned int)(kfi_keys[j] & 0xFFFFFFFFull);
        int kind = 1;
        if (d.mode != 0) {
            const unsigned long long id = mp_id[i];
            if (id != CORB_NO_MAP_POINT) {                                                        // MapPoint* pMP = mvpMapPoints[i].getMapPoint(); if(!pMP) bCreateNew = true;
                const int ms = corb_idtab_find(d.idt, id);
                if (ms < 0) kind = 3;
                else kind = reinterpret_cast<const CorbMapPointRecord*>(d.mp_base + (size_t)ms * d.mp_bytes)->n_obs < 1 ? 2 : 0;      // else if(pMP->Observations()<1)
            }
        }
        d.order[j] = i; d.kind[j] = (unsigned char)kind;
        cnt += (kind == 1 || kind == 2) ? 1 : 0;
    }
    int created;
    int k = kfi_block_scan(cnt, part, &created);                                                  // (its barriers stand between the reads above and the writes below)
    const bool full = d.apply && created > d.mp_capacity - d.first_mp_slot;
    if (t == 0) { d.counts[0] = visited; d.counts[1] = created; d.counts[2] = full ? 1 : 0; d.counts[3] = 0; }
    if (cnt == 0) return;
    NpCam c;
#pragma unroll
    for (int q = 0; q < 12; q++) c.T[q] = hdr->m.Tcw[q];
    c.fx = d.fx; c.fy = d.fy; c.cx = d.cx; c.cy = d.cy;
    np_cam_finish(c);
    const CorbKeyPoint* kp = reinterpret_cast<const CorbKeyPoint*>(d.rec + KL.kp);
    const float* ur = reinterpret_cast<const float*>(d.rec + KL.ur);
    const MpLayout ML(d.max_obs);
    const unsigned long long kf_id = hdr->m.id;
    for (int j = b; j < e; j++) {
        const int kind = d.kind[j];
        if (kind != 1 && kind != 2) continue;
        const int i = d.order[j];
        const CorbKeyPoint p = kp[i];
        float X[3]; np_unproject_uv(c, p.x, p.y, depth[i], X);
        d.x3d[3 * (size_t)k] = X[0]; d.x3d[3 * (size_t)k + 1] = X[1]; d.x3d[3 * (size_t)k + 2] = X[2];
        if (d.apply && !full) {
            char* rec = d.mp_base + (size_t)(d.first_mp_slot + k) * d.mp_bytes;
            unsigned long long* w = reinterpret_cast<unsigned long long*>(rec);
            for (int q = 0; q < CORB_MP_HEADER_BYTES / 8; q++) w[q] = 0ull;                       // header and counters
            unsigned long long* okf = reinterpret_cast<unsigned long long*>(rec + ML.obs_kf); uint32_t* oidx = reinterpret_cast<uint32_t*>(rec + ML.obs_idx);
            for (int q = 0; q < d.max_obs; q++) { okf[q] = 0ull; oidx[q] = 0u; }
            unsigned long long* sw = reinterpret_cast<unsigned long long*>(rec + ML.scratch);
            for (int q = 0; q < (int)(sizeof(CorbMapPointScratch) / 8); q++) sw[q] = 0ull;
            CorbMapPointRecord* m = reinterpret_cast<CorbMapPointRecord*>(rec);
            CorbMapPointCounters* ct = reinterpret_cast<CorbMapPointCounters*>(rec + sizeof(CorbMapPointRecord));
            CorbMapPointScratch* sc = reinterpret_cast<CorbMapPointScratch*>(rec + ML.scratch);
            const unsigned long long id = d.first_mp_id + (unsigned long long)k;
            m->id = id; m->client_id = d.client_id; m->flags = 0;
            m->world_pos[0] = X[0]; m->world_pos[1] = X[1]; m->world_pos[2] = X[2];
            const unsigned long long* dsrc = reinterpret_cast<const unsigned long long*>(d.rec + KL.desc) + 4 * (size_t)i;
            unsigned long long* ddst = reinterpret_cast<unsigned long long*>(m->descriptor);
#pragma unroll
            for (int q = 0; q < 4; q++) ddst[q] = dsrc[q];
            float nd[5];
            if (d.mode == 2) {                                                                    // MapPoint(x3D, cacher, pFrame, idxF): no keyframe, no observation
                kfi_temporal_point(c, X, p.octave, d.nlevels, d.scale, nd);
                m->ref_kf_id = 0ull; m->n_obs = 0;
                sc->first_kf_id = -1; sc->track_in_view = 1;
            } else {                                                                              // MapPoint(x3D, pKF, cacher); AddObservation(pKF, i); UpdateNormalAndDepth()
                kfi_single_observation(hdr->m.Tcw, X, p.octave, d.nlevels, d.scale, nd);
                m->ref_kf_id = kf_id;
                if (d.max_obs >= 1) { okf[0] = kf_id; oidx[0] = (uint32_t)i; m->n_obs = 1; }
                sc->first_kf_id = (long long)kf_id; sc->n_obs_weight = kfi_obs_weight(true, ur[i]);
            }
            sc->first_frame = d.frame_id;
            m->normal[0] = nd[0]; m->normal[1] = nd[1]; m->normal[2] = nd[2]; m->min_distance = nd[3]; m->max_distance = nd[4];
            ct->n_visible = 1; ct->n_found = 1;
            // pKF->AddMapPoint(pNewMP, i); mCurrentFrame.mvpMapPoints[i] = pNewMP
            reinterpret_cast<unsigned long long*>(d.rec + KL.mp_id)[i] = id; reinterpret_cast<unsigned char*>(d.rec + KL.flags)[i] |= 1u;
            if (d.mirror) {
                const RecLayout ML2(d.mirror_F);
                reinterpret_cast<unsigned long long*>(d.mirror + ML2.mp_id)[i] = id; reinterpret_cast<unsigned char*>(d.mirror + ML2.flags)[i] |= 1u;
            }
        }
        k++;
    }
}

__global__ __launch_bounds__(256) void kfi_counts_kernel(KfiCountsDev d)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < d.n_cur) {                                                                            // (:1026-1035)
        const RecLayout L(d.cur_F);
        const float z = reinterpret_cast<const float*>(d.cur + L.depth)[i];
        if (z > 0 && z < d.th_depth) {
            const unsigned long long id = reinterpret_cast<const unsigned long long*>(d.cur + L.mp_id)[i];
            const bool outlier = (reinterpret_cast<const unsigned char*>(d.cur + L.flags)[i] & 2u) != 0;
            const bool tracked = id != CORB_NO_MAP_POINT && corb_idtab_find(d.idt, id) >= 0 && !outlier;
            atomicAdd(&d.counts[tracked ? 0 : 1], 1);
        }
    }
    if (d.ref && i < d.n_ref) {                                                                   // KeyFrame::TrackedMapPoints(minObs)
        const RecLayout L(d.ref_F);
        const unsigned long long id = reinterpret_cast<const unsigned long long*>(d.ref + L.mp_id)[i];
        const int ms = id == CORB_NO_MAP_POINT ? -1 : corb_idtab_find(d.idt, id);
        if (ms >= 0) {
            const char* mrec = d.mp_base + (size_t)ms * d.mp_bytes;
            if (!(reinterpret_cast<const CorbMapPointRecord*>(mrec)->flags & CORB_MP_BAD)) {
                const RecLayout KL(d.kf_F);
                if (d.min_obs <= 0 || kfi_observations(mrec, d.max_obs, d.kf_base, d.kf_bytes, KL, d.kfid) >= d.min_obs) atomicAdd(&d.counts[2], 1);
            }
        }
    }
}

// ---- LocalMapping::ProcessNewKeyFrame's association loop (C/src/LocalMapping.cc:132-151) ----
// The serial loop in closed form: a point the keyframe does not observe yet is added by the LOWEST feature that holds it (IsInKeyFrame is true by the time the loop
// reaches the others, which enter the recent list like a point that observed the keyframe from the start).
__global__ __launch_bounds__(KFI_THREADS) void kfi_assoc_kernel(KfiAssocDev d)
{
    __shared__ int part[KFI_THREADS];
    __shared__ int sh_full;
    const int t = threadIdx.x;
    const RecLayout KL(d.F); const MpLayout ML(d.max_obs);
    const unsigned long long kf_id = reinterpret_cast<const KfHeader*>(d.rec)->m.id;
    const unsigned long long* mp_id = reinterpret_cast<const unsigned long long*>(d.rec + KL.mp_id);
    if (t == 0) sh_full = 0;
    // kinds 0, 1, 2 are final here; 4 = the list holds the keyframe; 3 = a candidate for the addition, settled below
    for (int i = t; i < d.n; i += KFI_THREADS) {
        const unsigned long long id = mp_id[i];
        int kind = 0, ms = -1;
        if (id != CORB_NO_MAP_POINT) {
            ms = corb_idtab_find(d.idt, id);
            if (ms < 0) kind = 2;                                                                 // getMapPoint() gives NULL
            else {
                const char* mrec = d.mp_base + (size_t)ms * d.mp_bytes;
                const CorbMapPointRecord* m = reinterpret_cast<const CorbMapPointRecord*>(mrec);
                if (m->flags & CORB_MP_BAD) kind = 1;
                else {
                    const unsigned long long* okf = reinterpret_cast<const unsigned long long*>(mrec + ML.obs_kf);
                    const int no = min(max(m->n_obs, 0), d.max_obs);
                    bool in = false; for (int q = 0; q < no; q++) in = in || okf[q] == kf_id;      // pMP->IsInKeyFrame(mpCurrentKeyFrame)
                    kind = in ? 4 : 3;
                    if (!in) corb_idtab_insert_min(d.first, (unsigned long long)(unsigned int)ms, i);
                }
            }
        }
        d.kind[i] = (unsigned char)kind; d.mslot[i] = ms;
    }
    __threadfence_block();
    __syncthreads();
    const int per = (d.n + KFI_THREADS - 1) / KFI_THREADS;
    const int b = min(t * per, d.n), e = min(b + per, d.n);
    int n4 = 0, n3 = 0;
    for (int i = b; i < e; i++) {
        int kind = d.kind[i];
        if (kind == 3) {
            const int ms = d.mslot[i];
            if (corb_idtab_find(d.first, (unsigned long long)(unsigned int)ms) != i) { kind = 4; d.kind[i] = 4; }
            else if (reinterpret_cast<const CorbMapPointRecord*>(d.mp_base + (size_t)ms * d.mp_bytes)->n_obs >= d.max_obs) sh_full = 1;
        }
        n4 += kind == 4 ? 1 : 0; n3 += kind == 3 ? 1 : 0;
    }
    int n_recent, n_added;
    int k = kfi_block_scan(n4, part, &n_recent);
    (void)kfi_block_scan(n3, part, &n_added);
    for (int i = b; i < e; i++) if (d.kind[i] == 4) d.recent[k++] = d.mslot[i];                     // mlpRecentAddedMapPoints.push_back(pMP), in feature order
    if (t == 0) { d.counts[0] = n_added; d.counts[1] = n_recent; d.counts[2] = sh_full; d.counts[3] = 0; }
}

// the keyframes at hand: records of the named slots, found by id; the pose is the record's
struct KfiLookup {
    const KfiAssocDev& d;
    __device__ __forceinline__ int find(unsigned long long id) const { return corb_idtab_find(d.kfid, id); }
    __device__ __forceinline__ const float* pose(int p) const { return reinterpret_cast<const KfHeader*>(d.kf_base + (size_t)p * d.kf_bytes)->m.Tcw; }
    __device__ __forceinline__ const char* record(int p) const { return d.kf_base + (size_t)p * d.kf_bytes; }
};

// kind 3: pMP->AddObservation(pKF, i); pMP->UpdateNormalAndDepth(); pMP->ComputeDistinctiveDescriptors() (:141-143).  One wavefront per feature: lane 0 the list and
// the normal (a handful of entries, each depending on the one before), all lanes the descriptor distances -- the division of mp_replace_kernel.
__global__ __launch_bounds__(256) void kfi_assoc_apply_kernel(KfiAssocDev d)
{
    __shared__ unsigned short dist_all[4][DD_MAX_OBS];
    __shared__ int sh_n[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wave;
    const bool active = i < d.n && d.counts[2] == 0 && d.kind[i] == 3;
    const RecLayout KL(d.F); const MpLayout ML(d.max_obs);
    char* mrec = active ? d.mp_base + (size_t)d.mslot[i] * d.mp_bytes : nullptr;
    unsigned long long* D = d.desc + (size_t)(i < d.n ? i : 0) * d.max_obs * 4;
    if (lane == 0) {
        int m = -1;
        if (active) {
            CorbMapPointRecord* h = reinterpret_cast<CorbMapPointRecord*>(mrec);
            unsigned long long* okf = reinterpret_cast<unsigned long long*>(mrec + ML.obs_kf); uint32_t* oidx = reinterpret_cast<uint32_t*>(mrec + ML.obs_idx);
            const unsigned long long kf_id = reinterpret_cast<const KfHeader*>(d.rec)->m.id;
            int nb = min(max(h->n_obs, 0), d.max_obs);
            int j = nb;                                                                           // mObservations[pKF] = idx: the list ascends in the keyframe id
            while (j > 0 && okf[j - 1] > kf_id) { okf[j] = okf[j - 1]; oidx[j] = oidx[j - 1]; j--; }
            okf[j] = kf_id; oidx[j] = (uint32_t)i; nb++; h->n_obs = nb;
            corb_update_normal_depth(KfiLookup{d}, h, okf, oidx, nb, KL, d.scale_factor);
            m = 0;                                                                                // (the point is not bad: kind 3)
            for (int q = 0; q < nb; q++) {
                const int ks = corb_idtab_find(d.kfid, okf[q]);
                if (ks < 0) continue;
                const char* kr = d.kf_base + (size_t)ks * d.kf_bytes;
                if ((reinterpret_cast<const KfHeader*>(kr)->m.flags & CORB_KF_BAD) || (int)oidx[q] >= d.F) continue;      // if(!pKF->isBad())
                const unsigned long long* s = reinterpret_cast<const unsigned long long*>(kr + KL.desc) + 4 * (size_t)oidx[q];
                D[4 * m] = s[0]; D[4 * m + 1] = s[1]; D[4 * m + 2] = s[2]; D[4 * m + 3] = s[3]; m++;
            }
        }
        sh_n[wave] = m;
    }
    __threadfence_block();
    __syncthreads();
    const int m = sh_n[wave];
    if (m <= 0 || m > DD_MAX_OBS) return;                                                          // (if(vDescriptors.empty()) return;)
    const int best = distinctive_best(D, m, dist_all[wave], lane);
    if (lane < 4) reinterpret_cast<unsigned long long*>(reinterpret_cast<CorbMapPointRecord*>(mrec)->descriptor)[lane] = D[4 * best + lane];
}

__global__ __launch_bounds__(KFI_THREADS) void kfi_cull_kernel(KfiCullDev d)
{
    __shared__ int part[KFI_THREADS];
    const int t = threadIdx.x;
    const MpLayout ML(d.max_obs); const RecLayout KL(d.kf_F);
    for (int i = t; i < d.n; i += KFI_THREADS) corb_idtab_insert_min(d.first, (unsigned long long)(unsigned int)d.slots[i], i);
    __threadfence_block();
    __syncthreads();
    for (int i = t; i < d.n; i += KFI_THREADS) {
        if (corb_idtab_find(d.first, (unsigned long long)(unsigned int)d.slots[i]) != i) continue;
        const char* rec = d.mp_base + (size_t)d.slots[i] * d.mp_bytes;
        const CorbMapPointRecord* m = reinterpret_cast<const CorbMapPointRecord*>(rec);
        const CorbMapPointCounters* ct = reinterpret_cast<const CorbMapPointCounters*>(rec + sizeof(CorbMapPointRecord));
        const CorbMapPointScratch* sc = reinterpret_cast<const CorbMapPointScratch*>(rec + ML.scratch);
        d.decision[i] = (unsigned char)kfi_cull_decision((m->flags & CORB_MP_BAD) != 0, ct->n_found, ct->n_visible, d.cur_kf_id, sc->first_kf_id,
                                                         kfi_observations(rec, d.max_obs, d.kf_base, d.kf_bytes, KL, d.kfid), d.th_obs);
    }
    __threadfence_block();
    __syncthreads();
    // a later occurrence meets what the first left: a culled point is bad by then, any other decision repeats
    for (int i = t; i < d.n; i += KFI_THREADS) {
        const int f = corb_idtab_find(d.first, (unsigned long long)(unsigned int)d.slots[i]);
        if (f == i) continue;
        const int df = d.decision[f];
        d.decision[i] = (unsigned char)((df == 2 || df == 3) ? 1 : df);
    }
    __threadfence_block();
    __syncthreads();
    const int per = (d.n + KFI_THREADS - 1) / KFI_THREADS;
    const int b = min(t * per, d.n), e = min(b + per, d.n);
    int cnt = 0, cull = 0;
    for (int i = b; i < e; i++) { cnt += d.decision[i] == 0 ? 1 : 0; cull += (d.decision[i] == 2 || d.decision[i] == 3) ? 1 : 0; }
    int n_kept, n_culled;
    int k = kfi_block_scan(cnt, part, &n_kept);
    (void)kfi_block_scan(cull, part, &n_culled);
    for (int i = b; i < e; i++) if (d.decision[i] == 0) d.kept[k++] = d.slots[i];
    if (t == 0) { d.counts[0] = n_kept; d.counts[1] = n_culled; d.counts[2] = 0; d.counts[3] = 0; }
    if (!d.apply) return;
    // MapPoint::SetBadFlag (MapPoint.cc:255-269): every decision above was read before the barriers of the scans
    for (int i = b; i < e; i++) {
        if (d.decision[i] != 2 && d.decision[i] != 3) continue;
        char* rec = d.mp_base + (size_t)d.slots[i] * d.mp_bytes;
        CorbMapPointRecord* m = reinterpret_cast<CorbMapPointRecord*>(rec);
        unsigned long long* okf = reinterpret_cast<unsigned long long*>(rec + ML.obs_kf); uint32_t* oidx = reinterpret_cast<uint32_t*>(rec + ML.obs_idx);
        const int n = min(max(m->n_obs, 0), d.max_obs);
        for (int q = 0; q < n; q++) {                                                             // pKF->EraseMapPointMatch(mit->second)
            const int ks = corb_idtab_find(d.kfid, okf[q]);
            if (ks < 0) continue;
            char* kr = d.kf_base + (size_t)ks * d.kf_bytes;
            if ((int)oidx[q] >= reinterpret_cast<const KfHeader*>(kr)->n) continue;
            reinterpret_cast<unsigned long long*>(kr + KL.mp_id)[oidx[q]] = CORB_NO_MAP_POINT;
            reinterpret_cast<unsigned char*>(kr + KL.flags)[oidx[q]] &= (unsigned char)~1u;
        }
        for (int q = 0; q < d.max_obs; q++) { okf[q] = 0ull; oidx[q] = 0u; }
        m->flags |= CORB_MP_BAD; m->n_obs = 0;
    }
}

}  // namespace

void corb_launch_kfi_points(const KfiPointsDev& d, hipStream_t s)
{
    hipLaunchKernelGGL(kfi_points_kernel, dim3(1), dim3(KFI_THREADS), (size_t)d.P * 8, s, d);
}
void corb_launch_kfi_counts(const KfiCountsDev& d, hipStream_t s)
{
    const int n = d.n_cur > d.n_ref ? d.n_cur : d.n_ref;
    if (n > 0) hipLaunchKernelGGL(kfi_counts_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d);
}
void corb_launch_kfi_assoc(const KfiAssocDev& d, int apply, hipStream_t s)
{
    hipLaunchKernelGGL(kfi_assoc_kernel, dim3(1), dim3(KFI_THREADS), 0, s, d);
    if (apply && d.n > 0) hipLaunchKernelGGL(kfi_assoc_apply_kernel, dim3((d.n + 3) / 4), dim3(256), 0, s, d);
}
void corb_launch_kfi_cull(const KfiCullDev& d, hipStream_t s)
{
    hipLaunchKernelGGL(kfi_cull_kernel, dim3(1), dim3(KFI_THREADS), 0, s, d);
}

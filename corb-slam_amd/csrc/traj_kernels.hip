// traj_kernels.hip -- the camera trajectory on records (include/corb_trajectory.h): the entry Tracking::Track appends (C/src/Tracking.cc:485-504), KeyFrame::mTcp
// (KeyFrame.cc:666), and the loops of System::SaveTrajectoryTUM / SaveTrajectoryKITTI / SaveKeyFrameTrajectoryTUM (System.cc:254-403).  Small kernels in stream
// order, no grid barrier; the arithmetic is traj_math.h's, the same text the host program of the tests runs.  Integer atomics only: no result depends on the order
// they land in.  Every loop's trip count is bounded by a launch argument: ids are resolved by a scan over the slots, not through a probing table.
#include "traj_internal.h"
#include "traj_math.h"
#include "device_util.h"
#include <cstring>

#define TRAJ_NO_ID 0xFFFFFFFFFFFFFFFFull     // "none" in the graph's parent field (covis_math.h: COVIS_NO_ID)

namespace {

__device__ __forceinline__ const KfHeader* tj_header(const TrajDev& d, int slot) { return reinterpret_cast<const KfHeader*>(d.kf_base + (size_t)slot * d.kf_bytes); }
// a slot without features is not a keyframe, as the id index of the stores has it (map_kernels.hip)
__device__ __forceinline__ bool tj_held(const KfHeader* h) { return h->n > 0; }

// the lowest slot that holds `id` (n_slots if none), found by the whole workgroup; sh is one int of LDS
__device__ __forceinline__ int tj_block_find(const TrajDev& d, unsigned long long id, int* sh)
{
    if (threadIdx.x == 0) *sh = d.n_slots;
    __syncthreads();
    if (id != TRAJ_NO_ID)
        for (int s = threadIdx.x; s < d.n_slots; s += TRAJ_T) { const KfHeader* h = tj_header(d, s); if (tj_held(h) && h->m.id == id) atomicMin(sh, s); }
    __syncthreads();
    return *sh;
}

// mlRelativeFramePoses / mlpReferences / mlFrameTimes / mlbLost .push_back (Tracking.cc:491-495), or the copy of back() (:500-503)
__global__ __launch_bounds__(64) void traj_append_kernel(TrajDev d, int kind, int n, const char* cur, int ref_slot, CorbTrajEntry given)
{
    __shared__ float Twc[16];
    CorbTrajEntry* e = d.entries + n;
    const int l = threadIdx.x;
    if (kind == 2) {
        const CorbTrajEntry* b = d.entries + (n - 1);
        if (l < 16) e->Tcr[l] = b->Tcr[l];
        if (l == 16) { e->ref_id = b->ref_id; e->timestamp = b->timestamp; e->ref_slot = b->ref_slot; e->lost = given.lost; }
        return;
    }
    const KfHeader* ref = tj_header(d, ref_slot);
    if (kind == 1) {                                                                 // Tcr = mCurrentFrame.mTcw*mCurrentFrame.mpReferenceKF->GetPoseInverse(), as trackframe_finish_kernel
        if (l == 0) tfm_pose_inverse(ref->m.Tcw, Twc);
        __syncthreads();
        if (l < 16) e->Tcr[l] = tfm_gemm4_at(reinterpret_cast<const KfHeader*>(cur)->m.Tcw, Twc, l >> 2, l & 3);
    } else if (l < 16) e->Tcr[l] = given.Tcr[l];
    if (l == 16) { e->ref_id = ref->m.id; e->timestamp = given.timestamp; e->ref_slot = ref_slot; e->lost = given.lost; }
}

// mTcp = Tcw*mpParent->GetPoseInverse() (KeyFrame.cc:666)
__global__ __launch_bounds__(TRAJ_T) void traj_set_bad_pose_kernel(TrajDev d, int slot)
{
    __shared__ int found;
    __shared__ float Twc[16];
    const KfHeader* h = tj_header(d, slot);
    const bool held = tj_held(h);
    const int p = tj_block_find(d, held ? d.parent[slot] : TRAJ_NO_ID, &found);
    if (p >= d.n_slots) { if (threadIdx.x == 0) d.status[0] = 1; return; }
    if (threadIdx.x == 0) { d.status[0] = 0; tfm_pose_inverse(tj_header(d, p)->m.Tcw, Twc); }
    __syncthreads();
    if (threadIdx.x < 16) d.Tcp[(size_t)slot * 16 + threadIdx.x] = tfm_gemm4_at(h->m.Tcw, Twc, threadIdx.x >> 2, threadIdx.x & 3);
}

// the store as plain arrays: a thread per slot.  parent_slot: the lowest held slot of the parent's id, -1 for "none" or a parent the store does not hold
__global__ __launch_bounds__(TRAJ_T) void traj_gather_kernel(TrajDev d)
{
    const int s = blockIdx.x * TRAJ_T + threadIdx.x;
    if (s >= d.n_slots) return;
    const KfHeader* h = tj_header(d, s);
    const bool held = tj_held(h);
    d.held[s] = held ? 1 : 0; d.flags[s] = h->m.flags; d.id[s] = h->m.id;
    for (int e = 0; e < 16; e++) d.Tcw[(size_t)s * 16 + e] = h->m.Tcw[e];
    int ps = -1;
    const unsigned long long pid = d.parent[s];
    if (held && pid != TRAJ_NO_ID)
        for (int o = 0; o < d.n_slots; o++) { const KfHeader* ho = tj_header(d, o); if (tj_held(ho) && ho->m.id == pid) { ps = o; break; } }
    d.parent_slot[s] = ps;
}

// Two = vpKFs[0]->GetPoseInverse() (System.cc:266 = :362).  origin_slot = -1: vpKFs sorted by KeyFrame::lId, so the smallest id among the held records without
// CORB_KF_BAD -- a min-reduction over (id, slot) by one workgroup.  Also zeroes the head
__global__ __launch_bounds__(TRAJ_T) void traj_origin_kernel(TrajDev d, int origin_slot, int n_entries)
{
    __shared__ unsigned long long best_id;
    __shared__ int best_slot;
    if (threadIdx.x == 0) { best_id = TRAJ_NO_ID; best_slot = d.n_slots; }
    __syncthreads();
    if (origin_slot < 0) {
        for (int s = threadIdx.x; s < d.n_slots; s += TRAJ_T) if (d.held[s] && !(d.flags[s] & TJM_KF_BAD)) atomicMin(&best_id, d.id[s]);
        __syncthreads();
        for (int s = threadIdx.x; s < d.n_slots; s += TRAJ_T) if (d.held[s] && !(d.flags[s] & TJM_KF_BAD) && d.id[s] == best_id) atomicMin(&best_slot, s);
        __syncthreads();
    } else if (threadIdx.x == 0 && origin_slot < d.n_slots && d.held[origin_slot]) best_slot = origin_slot;
    __syncthreads();
    if (threadIdx.x == 0) {
        TrajHead* H = d.head;
        const bool ok = best_slot < d.n_slots;
        H->status = ok ? 0 : 1; H->origin = ok ? best_slot : -1; H->n_rows = 0;
        H->stats.n_entries = n_entries; H->stats.n_rows = 0; H->stats.n_lost_skipped = 0; H->stats.n_ref_gone = 0; H->stats.n_chain_broken = 0; H->stats.max_chain = 0;
        if (ok) tfm_pose_inverse(d.Tcw + (size_t)best_slot * 16, H->Two);
        else for (int e = 0; e < 16; e++) H->Two[e] = 0.f;
    }
}

// Trw of every held slot: a thread per slot runs traj_math.h's walk
__global__ __launch_bounds__(TRAJ_T) void traj_walk_kernel(TrajDev d)
{
    const int s = blockIdx.x * TRAJ_T + threadIdx.x;
    if (s >= d.n_slots) return;
    if (!d.held[s] || d.head->status) { d.chain[s] = TJM_CHAIN_BROKEN; return; }
    float Trw[16];
    const int c = tjm_walk(s, d.flags, d.parent_slot, d.Tcp, d.Tcw, d.n_slots, d.head->Two, Trw);
    d.chain[s] = c;
    if (c >= 0) for (int e = 0; e < 16; e++) d.Trw[(size_t)s * 16 + e] = Trw[e];
}

// which entries give a row, and why the others do not: a thread per entry
__global__ __launch_bounds__(TRAJ_T) void traj_valid_kernel(TrajDev d, int n_entries, int format)
{
    const int i = blockIdx.x * TRAJ_T + threadIdx.x;
    if (i >= n_entries) return;
    const CorbTrajEntry& e = d.entries[i];
    int v = 0;
    if (d.head->status) v = 0;
    else if (format == 1 && e.lost) atomicAdd(&d.head->stats.n_lost_skipped, 1);                        // if(*lbL) continue; (System.cc:283)
    else if (e.ref_slot < 0 || e.ref_slot >= d.n_slots || !d.held[e.ref_slot] || d.id[e.ref_slot] != e.ref_id) atomicAdd(&d.head->stats.n_ref_gone, 1);
    else if (d.chain[e.ref_slot] < 0) atomicAdd(&d.head->stats.n_chain_broken, 1);
    else { v = 1; atomicMax(&d.head->stats.max_chain, d.chain[e.ref_slot]); }
    d.valid[i] = v;
}

// the rows in log order: entry i's row at pos[i]
__global__ __launch_bounds__(TRAJ_T) void traj_rows_kernel(TrajDev d, int n_entries, int format)
{
    const int i = blockIdx.x * TRAJ_T + threadIdx.x;
    if (i == 0) { d.head->n_rows = d.pos[n_entries]; d.head->stats.n_rows = d.pos[n_entries]; }
    if (i >= n_entries || !d.valid[i]) return;
    const CorbTrajEntry& e = d.entries[i];
    const int r = d.pos[i];
    const float* Trw = d.Trw + (size_t)e.ref_slot * 16;
    if (format == 0) tjm_row_kitti(e.Tcr, Trw, d.rows + (size_t)r * 12);
    else tjm_row_tum(e.Tcr, Trw, d.rows + (size_t)r * 7);
    d.times[r] = e.timestamp; d.index[r] = i;
}

// SaveKeyFrameTrajectoryTUM: a thread per slot; its rank among the held records without CORB_KF_BAD in ascending (id, slot) is its row
__global__ __launch_bounds__(TRAJ_T) void traj_keyframes_kernel(TrajDev d)
{
    const int s = blockIdx.x * TRAJ_T + threadIdx.x;
    if (s >= d.n_slots || !d.held[s] || (d.flags[s] & TJM_KF_BAD)) return;
    const unsigned long long id = d.id[s];
    int rank = 0;
    for (int o = 0; o < d.n_slots; o++)
        if (d.held[o] && !(d.flags[o] & TJM_KF_BAD) && (d.id[o] < id || (d.id[o] == id && o < s))) rank++;
    tjm_row_keyframe(d.Tcw + (size_t)s * 16, d.rows + (size_t)rank * 7);
    d.times[rank] = d.time[s];
    reinterpret_cast<unsigned long long*>(d.index)[rank] = id;
    atomicAdd(&d.head->n_rows, 1);
}
__global__ void traj_head_clear_kernel(TrajDev d) { d.head->status = 0; d.head->origin = -1; d.head->n_rows = 0; }

}  // namespace

void traj_launch_append(const TrajDev& d, int kind, int n, const char* cur, int ref_slot, const float* Tcr, double timestamp, int lost, hipStream_t s)
{
    CorbTrajEntry given; memset(&given, 0, sizeof(given));
    if (Tcr) memcpy(given.Tcr, Tcr, sizeof(given.Tcr));
    given.timestamp = timestamp; given.lost = lost ? 1 : 0;
    hipLaunchKernelGGL(traj_append_kernel, dim3(1), dim3(64), 0, s, d, kind, n, cur, ref_slot, given);
}
void traj_launch_set_bad_pose(const TrajDev& d, int slot, hipStream_t s) { hipLaunchKernelGGL(traj_set_bad_pose_kernel, dim3(1), dim3(TRAJ_T), 0, s, d, slot); }
void traj_launch_frames(const TrajDev& d, int n_entries, int origin_slot, int format, hipStream_t s)
{
    const dim3 slots((d.n_slots + TRAJ_T - 1) / TRAJ_T), entries((n_entries + TRAJ_T - 1) / TRAJ_T);
    hipLaunchKernelGGL(traj_gather_kernel, slots, dim3(TRAJ_T), 0, s, d);
    hipLaunchKernelGGL(traj_origin_kernel, dim3(1), dim3(TRAJ_T), 0, s, d, origin_slot, n_entries);
    if (n_entries <= 0) return;
    hipLaunchKernelGGL(traj_walk_kernel, slots, dim3(TRAJ_T), 0, s, d);
    hipLaunchKernelGGL(traj_valid_kernel, entries, dim3(TRAJ_T), 0, s, d, n_entries, format);
    corb_launch_exclusive_scan(d.valid, d.pos, (size_t)n_entries, d.scan_scratch, s);
    hipLaunchKernelGGL(traj_rows_kernel, entries, dim3(TRAJ_T), 0, s, d, n_entries, format);
}
void traj_launch_keyframes(const TrajDev& d, hipStream_t s)
{
    const dim3 slots((d.n_slots + TRAJ_T - 1) / TRAJ_T);
    hipLaunchKernelGGL(traj_gather_kernel, slots, dim3(TRAJ_T), 0, s, d);
    hipLaunchKernelGGL(traj_head_clear_kernel, dim3(1), dim3(1), 0, s, d);
    hipLaunchKernelGGL(traj_keyframes_kernel, slots, dim3(TRAJ_T), 0, s, d);
}

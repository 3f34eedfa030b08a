// publish_kernels.hip -- the map publish on records (include/corb_map_publish.h): the pose / position packets of a pack, and an apply -- what the four
// subscriber callbacks of C/src/Cache.cc:446-634 do with a message -- as a chain of short kernels on one stream.  Memory-bound scatter / gather work:
//   classify   one lane per entry; an id-table probe is bounded by the table's size
//   compact    order-preserving, in two passes: per-workgroup counts, a scan of the counts that crosses workgroups (device_util.hip), a scatter.  No kernel waits
//              on another workgroup: a verdict passes from one kernel to the next through PubState in device memory, ordered by the stream
//   copy       16 bytes per lane to the destination slot of each accepted record
//   update     adjacent lanes read adjacent packets (whole cache lines are used), header writes are scattered
// "lowest position wins" / "highest position wins" are atomicMin on the position / on n - 1 - position, so every output is independent of the launch order.
// Arithmetic as rebase_records_kernel: exact float products summed in double, left to right, one rounding (-ffp-contract=off; the fused forms are spelled out).
#include "publish_internal.h"
#include "lane_exchange.h"

namespace {
// ---- id tables with bounded probes (device_util.h's layout; a table is at most half full, so the bound is never the reason a probe ends) ----
__device__ __forceinline__ int pub_find(const CorbIdTable& t, unsigned long long key)
{
    unsigned int h = corb_idtab_hash(key) & t.mask;
    for (unsigned int step = 0; step <= t.mask; step++) {
        const unsigned long long k = t.keys[h];
        if (k == key) return t.vals[h];
        if (k == CORB_IDTAB_EMPTY) return -1;
        h = (h + 1) & t.mask;
    }
    return -1;
}
__device__ __forceinline__ void pub_insert_min(const CorbIdTable& t, unsigned long long key, int val)
{
    unsigned int h = corb_idtab_hash(key) & t.mask;
    for (unsigned int step = 0; step <= t.mask; step++) {
        const unsigned long long prev = atomicCAS(&t.keys[h], CORB_IDTAB_EMPTY, key);
        if (prev == CORB_IDTAB_EMPTY || prev == key) { atomicMin(&t.vals[h], val); return; }
        h = (h + 1) & t.mask;
    }
}
// first writer's value stays; false: the key was there
__device__ __forceinline__ bool pub_insert(const CorbIdTable& t, unsigned long long key, int val)
{
    unsigned int h = corb_idtab_hash(key) & t.mask;
    for (unsigned int step = 0; step <= t.mask; step++) {
        const unsigned long long prev = atomicCAS(&t.keys[h], CORB_IDTAB_EMPTY, key);
        if (prev == CORB_IDTAB_EMPTY) { t.vals[h] = val; return true; }
        if (prev == key) return false;
        h = (h + 1) & t.mask;
    }
    return false;
}

// o <- a * M (row-major 4x4): cv::gemm of two float matrices
__device__ __forceinline__ void pub_mul44(const float* a, const float* M, float* o)
{
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            double s = __dmul_rn((double)a[r * 4], (double)M[c]);
            s = __fma_rn((double)a[r * 4 + 1], (double)M[4 + c], s);
            s = __fma_rn((double)a[r * 4 + 2], (double)M[8 + c], s);
            s = __fma_rn((double)a[r * 4 + 3], (double)M[12 + c], s);
            o[r * 4 + c] = (float)s;
        }
}
// o <- R p + t with R, t of T: one gemm row each -- the double row sum plus (double)t, rounded once
__device__ __forceinline__ void pub_point(const float* T, const float* p, float* o)
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double s = __dmul_rn((double)T[r * 4], (double)p[0]);
        s = __fma_rn((double)T[r * 4 + 1], (double)p[1], s);
        s = __fma_rn((double)T[r * 4 + 2], (double)p[2], s);
        s = __dadd_rn(s, (double)T[r * 4 + 3]);
        o[r] = (float)s;
    }
}

// id, client id and flags of a record header, keyframe or map point
template <bool KF> __device__ __forceinline__ unsigned long long rec_id(const char* rec)
{
    return KF ? reinterpret_cast<const KfHeader*>(rec)->m.id : reinterpret_cast<const CorbMapPointRecord*>(rec)->id;
}
template <bool KF> __device__ __forceinline__ int rec_client(const char* rec)
{
    return KF ? reinterpret_cast<const KfHeader*>(rec)->m.client_id : reinterpret_cast<const CorbMapPointRecord*>(rec)->client_id;
}
template <bool KF> __device__ __forceinline__ bool rec_fixed(const char* rec)
{
    return KF ? (reinterpret_cast<const KfHeader*>(rec)->m.flags & CORB_KF_FIXED) != 0 : (reinterpret_cast<const CorbMapPointRecord*>(rec)->flags & CORB_MP_FIXED) != 0;
}

// sum / exclusive prefix over the workgroup, thread order
__device__ __forceinline__ int wg_excl_scan(int v, int* sh, int* total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int inc = lx_wave_incl_scan_i(v);
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < PUB_WG / 64; i++) { if (i < w) base += sh[i]; tot += sh[i]; }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}
}  // namespace

// ------------------------------------------------------------------------------------------------ pack: sections C and D
// one lane per 4-byte word of a packet: the stores are contiguous over the workgroup, the loads touch one header per packet
__global__ __launch_bounds__(256) void pub_pack_poses_kernel(PubPackDev d)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nc = (size_t)d.n_upd_kf * 18, nd = (size_t)d.n_upd_mp * 6;
    if (t < nc) {
        const size_t i = t / 18; const int w = (int)(t - i * 18);
        const KfHeader* h = reinterpret_cast<const KfHeader*>(d.kf_base + (size_t)d.upd_kf[i] * d.kf_bytes);
        uint32_t v;
        if (w < 2) v = (uint32_t)(h->m.id >> (32 * w)); else v = __float_as_uint(h->m.Tcw[w - 2]);
        reinterpret_cast<uint32_t*>(d.sec_c)[t] = v;
    } else if (t - nc < nd) {
        const size_t u = t - nc, i = u / 6; const int w = (int)(u - i * 6);
        const CorbMapPointRecord* h = reinterpret_cast<const CorbMapPointRecord*>(d.mp_base + (size_t)d.upd_mp[i] * d.mp_bytes);
        uint32_t v = 0;
        if (w < 2) v = (uint32_t)(h->id >> (32 * w)); else if (w < 5) v = __float_as_uint(h->world_pos[w - 2]);
        reinterpret_cast<uint32_t*>(d.sec_d)[u] = v;
    }
}
void pub_launch_pack_poses(const PubPackDev& d, hipStream_t s)
{
    const size_t total = (size_t)d.n_upd_kf * 18 + (size_t)d.n_upd_mp * 6;
    if (total > 0) hipLaunchKernelGGL(pub_pack_poses_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d);
}

// ------------------------------------------------------------------------------------------------ apply
// the client's entry of section E (the lowest position that names it): found, T, Tinv -> PubState.  One wavefront.
__global__ __launch_bounds__(64) void pub_setup_kernel(PubApplyDev d)
{
    const int lane = threadIdx.x;
    int best = 0x7FFFFFFF;
    for (int k = lane; k < d.n_trans; k += 64) if (d.sec_e[k].client_id == d.client_id) { best = k; break; }
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
    if (best == 0x7FFFFFFF) return;                                    // (PubState was cleared by the call: found = 0)
    if (lane < 16) { d.st->T[lane] = d.sec_e[best].T[lane]; d.st->Tinv[lane] = d.sec_e[best].Tinv[lane]; }
    if (lane == 0) d.st->found = 1;
}

// A / B, pass 1: kind 1 (the client's own), 2 (held), or a candidate (3) that enters `first` with its position
template <bool KF> __global__ __launch_bounds__(PUB_WG) void pub_classify_new_kernel(PubApplyDev d)
{
    const PubSide& S = d.s[KF ? 0 : 1];
    const int i = blockIdx.x * PUB_WG + threadIdx.x;
    if (i >= S.n_new) return;
    unsigned char kind = 0;
    if (d.st->found) {
        const char* rec = S.sec_new + (size_t)i * S.rec_bytes;
        const unsigned long long id = rec_id<KF>(rec);
        if (rec_client<KF>(rec) == d.client_id) kind = 1;
        else if (pub_find(S.held, id) >= 0) kind = 2;
        else { kind = 3; pub_insert_min(S.first, id, i); }
    }
    S.kind_new[i] = kind;
}
// pass 2: of the candidates with one id the lowest position stays 3; the workgroup's count of them
template <bool KF> __global__ __launch_bounds__(PUB_WG) void pub_count_new_kernel(PubApplyDev d)
{
    __shared__ int sh[PUB_WG / 64];
    const PubSide& S = d.s[KF ? 0 : 1];
    const int i = blockIdx.x * PUB_WG + threadIdx.x;
    int flag = 0;
    if (i < S.n_new && S.kind_new[i] == 3) {
        const char* rec = S.sec_new + (size_t)i * S.rec_bytes;
        if (pub_find(S.first, rec_id<KF>(rec)) == i) flag = 1; else S.kind_new[i] = 2;
    }
    int total;
    (void)wg_excl_scan(flag, sh, &total);
    if (threadIdx.x == 0) S.wg_cnt[blockIdx.x] = total;
}
// pass 3 (behind the scan of the counts): rank of every accepted entry, the message position of the k-th accepted, its slot
template <bool KF> __global__ __launch_bounds__(PUB_WG) void pub_scatter_new_kernel(PubApplyDev d)
{
    __shared__ int sh[PUB_WG / 64];
    const PubSide& S = d.s[KF ? 0 : 1];
    const int i = blockIdx.x * PUB_WG + threadIdx.x;
    const int flag = (i < S.n_new && S.kind_new[i] == 3) ? 1 : 0;
    int total;
    const int k = S.wg_off[blockIdx.x] + wg_excl_scan(flag, sh, &total);
    if (i >= S.n_new) return;
    S.rank[i] = flag ? k : -1;
    if (!flag) return;
    S.src[k] = i;
    if (k < S.room) {                                                  // (the slot lists hold min(n_new, room) entries; beyond: the call answers CORB_ERR_CAPACITY)
        S.new_slots[k] = S.free_first + k;
        if (KF) {
            const int* h = reinterpret_cast<const int*>(S.sec_new + (size_t)i * S.rec_bytes);
            int* o = d.kf_hdr + 4 * (size_t)k;
            o[0] = h[0]; o[1] = h[1]; o[2] = h[2]; o[3] = h[3];
        }
    }
}
// the totals, and whether the write phases run
__global__ __launch_bounds__(64) void pub_gate_kernel(PubApplyDev d, int n_wg_kf, int n_wg_mp)
{
    if (threadIdx.x != 0) return;
    const int a = n_wg_kf > 0 ? d.s[0].wg_off[n_wg_kf] : 0, b = n_wg_mp > 0 ? d.s[1].wg_off[n_wg_mp] : 0;
    const int over = (a > d.s[0].room ? 1 : 0) | (b > d.s[1].room ? 2 : 0);
    d.st->n_ins[0] = a; d.st->n_ins[1] = b; d.st->overflow = over;
    d.st->go = (d.st->found && d.apply && !over) ? 1 : 0;
}
// C / D: kind and target slot per entry; the kind-2 entries enter `last` with n - 1 - position
template <bool KF> __global__ __launch_bounds__(PUB_WG) void pub_classify_upd_kernel(PubApplyDev d)
{
    __shared__ int sh[PUB_WG / 64];
    const PubSide& S = d.s[KF ? 0 : 1];
    const int i = blockIdx.x * PUB_WG + threadIdx.x;
    const size_t packet = KF ? sizeof(CorbKeyFramePosePacket) : sizeof(CorbMapPointPosePacket);
    int two = 0;
    if (i < S.n_upd) {
        unsigned char kind = 0; int target = -1;
        if (d.st->found) {
            const unsigned long long id = *reinterpret_cast<const unsigned long long*>(S.sec_upd + (size_t)i * packet);
            const int slot = pub_find(S.held, id);
            if (slot >= 0 && slot < S.capacity) {
                kind = rec_fixed<KF>(S.base + (size_t)slot * S.rec_bytes) ? 2 : 1; target = slot;
            } else if (S.n_new > 0) {
                const int p = pub_find(S.first, id);                   // accepted by phase A / B of this call: held by now, and fixed
                if (p >= 0 && p < S.n_new && S.kind_new[p] == 3) { kind = 2; target = S.free_first + S.rank[p]; }
            }
            if (kind == 2) { two = 1; pub_insert_min(S.last, id, S.n_upd - 1 - i); }
        }
        S.kind_upd[i] = kind; S.target[i] = target;
    }
    int total;
    (void)wg_excl_scan(two, sh, &total);
    if (threadIdx.x == 0 && total) atomicAdd(&d.st->n_upd[KF ? 0 : 1], total);
}

// ---- the write phases: every kernel below returns at once unless PubState::go ----
template <bool KF> __global__ __launch_bounds__(256) void pub_copy_new_kernel(PubApplyDev d)
{
    if (!d.st->go) return;
    const PubSide& S = d.s[KF ? 0 : 1];
    const size_t per = S.rec_bytes / 16, total = per * (size_t)d.st->n_ins[KF ? 0 : 1];
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t k = t / per, w = t - k * per;
        reinterpret_cast<uint4*>(S.base + (size_t)(S.free_first + k) * S.rec_bytes)[w] = reinterpret_cast<const uint4*>(S.sec_new + (size_t)S.src[k] * S.rec_bytes)[w];
    }
}
template <bool KF> __global__ __launch_bounds__(256) void pub_fix_new_kernel(PubApplyDev d)
{
    if (!d.st->go) return;
    const PubSide& S = d.s[KF ? 0 : 1];
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= d.st->n_ins[KF ? 0 : 1]) return;
    char* rec = S.base + (size_t)(S.free_first + k) * S.rec_bytes;
    if (KF) {
        KfHeader* h = reinterpret_cast<KfHeader*>(rec);
        float t[16], o[16];
#pragma unroll
        for (int q = 0; q < 16; q++) t[q] = h->m.Tcw[q];
        pub_mul44(t, d.st->Tinv, o);                                   // Tcw = Tcw * Ttrans.inv() (Cache.cc:478-480)
#pragma unroll
        for (int q = 0; q < 16; q++) h->m.Tcw[q] = o[q];
        h->m.flags |= CORB_KF_FIXED;                                   // tKF->setFixed() (:482)
    } else {
        CorbMapPointRecord* h = reinterpret_cast<CorbMapPointRecord*>(rec);
        const float p[3] = {h->world_pos[0], h->world_pos[1], h->world_pos[2]};
        float o[3];
        pub_point(d.st->T, p, o);                                      // tPose = Rcw * tPose + tcw (:528-532); the normal and the distances stay as sent
        h->world_pos[0] = o[0]; h->world_pos[1] = o[1]; h->world_pos[2] = o[2];
        h->flags |= CORB_MP_FIXED;
    }
}
// the map's id index over the old range and the new slots, if phase B accepted anything
__global__ __launch_bounds__(256) void pub_index_clear_kernel(PubApplyDev d)
{
    if (!d.st->go || d.st->n_ins[1] <= 0) return;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t <= d.new_index.mask; t += (size_t)gridDim.x * 256) d.new_index.keys[t] = CORB_IDTAB_EMPTY;
}
__global__ __launch_bounds__(256) void pub_index_fill_kernel(PubApplyDev d)
{
    if (!d.st->go || d.st->n_ins[1] <= 0) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.mp_n + d.st->n_ins[1]) return;
    const CorbMapPointRecord* r = reinterpret_cast<const CorbMapPointRecord*>(d.s[1].base + (size_t)(d.mp_first + i) * d.s[1].rec_bytes);
    if (!pub_insert(d.new_index, r->id, d.mp_first + i)) d.st->dup = 1;
}
template <bool KF> __global__ __launch_bounds__(PUB_WG) void pub_update_kernel(PubApplyDev d)
{
    if (!d.st->go) return;
    const PubSide& S = d.s[KF ? 0 : 1];
    const int i = blockIdx.x * PUB_WG + threadIdx.x;
    if (i >= S.n_upd || S.kind_upd[i] != 2) return;
    const int slot = S.target[i];
    if (slot < 0 || slot >= S.capacity) return;
    if (KF) {
        const CorbKeyFramePosePacket* p = reinterpret_cast<const CorbKeyFramePosePacket*>(S.sec_upd) + i;
        if (pub_find(S.last, p->id) != S.n_upd - 1 - i) return;        // a later entry names the same keyframe: its value stays
        float t[16], o[16];
#pragma unroll
        for (int q = 0; q < 16; q++) t[q] = p->Tcw[q];
        pub_mul44(t, d.st->Tinv, o);                                   // Tcw = KFPose * Ttrans.inv() (Cache.cc:575-577)
        float* T = reinterpret_cast<KfHeader*>(S.base + (size_t)slot * S.rec_bytes)->m.Tcw;
#pragma unroll
        for (int q = 0; q < 16; q++) T[q] = o[q];
    } else {
        const CorbMapPointPosePacket* p = reinterpret_cast<const CorbMapPointPosePacket*>(S.sec_upd) + i;
        if (pub_find(S.last, p->id) != S.n_upd - 1 - i) return;
        const float q[3] = {p->pos[0], p->pos[1], p->pos[2]};
        float o[3];
        pub_point(d.st->T, q, o);                                      // (:620-624)
        float* w = reinterpret_cast<CorbMapPointRecord*>(S.base + (size_t)slot * S.rec_bytes)->world_pos;
        w[0] = o[0]; w[1] = o[1]; w[2] = o[2];
    }
}

static unsigned wgs(int n) { return (unsigned)((n + PUB_WG - 1) / PUB_WG); }
static unsigned copy_blocks(size_t words) { const size_t b = (words + 255) / 256; return (unsigned)(b < 1 ? 1 : (b < 65536 ? b : 65536)); }

void pub_launch_apply(const PubApplyDev& d, hipStream_t s)
{
    const int na = d.s[0].n_new, nb = d.s[1].n_new, nc = d.s[0].n_upd, nd = d.s[1].n_upd;
    hipLaunchKernelGGL(pub_setup_kernel, dim3(1), dim3(64), 0, s, d);
    if (na > 0) {
        hipLaunchKernelGGL(pub_classify_new_kernel<true>, dim3(wgs(na)), dim3(PUB_WG), 0, s, d);
        hipLaunchKernelGGL(pub_count_new_kernel<true>, dim3(wgs(na)), dim3(PUB_WG), 0, s, d);
        corb_launch_exclusive_scan(d.s[0].wg_cnt, d.s[0].wg_off, wgs(na), d.s[0].scan_scratch, s);
        hipLaunchKernelGGL(pub_scatter_new_kernel<true>, dim3(wgs(na)), dim3(PUB_WG), 0, s, d);
    }
    if (nb > 0) {
        hipLaunchKernelGGL(pub_classify_new_kernel<false>, dim3(wgs(nb)), dim3(PUB_WG), 0, s, d);
        hipLaunchKernelGGL(pub_count_new_kernel<false>, dim3(wgs(nb)), dim3(PUB_WG), 0, s, d);
        corb_launch_exclusive_scan(d.s[1].wg_cnt, d.s[1].wg_off, wgs(nb), d.s[1].scan_scratch, s);
        hipLaunchKernelGGL(pub_scatter_new_kernel<false>, dim3(wgs(nb)), dim3(PUB_WG), 0, s, d);
    }
    hipLaunchKernelGGL(pub_gate_kernel, dim3(1), dim3(64), 0, s, d, (int)(na > 0 ? wgs(na) : 0), (int)(nb > 0 ? wgs(nb) : 0));
    if (nc > 0) hipLaunchKernelGGL(pub_classify_upd_kernel<true>, dim3(wgs(nc)), dim3(PUB_WG), 0, s, d);
    if (nd > 0) hipLaunchKernelGGL(pub_classify_upd_kernel<false>, dim3(wgs(nd)), dim3(PUB_WG), 0, s, d);
    if (!d.apply) return;
    // phases A, B, C, D in the publication order (MapFusion.cpp:352-358)
    const int ua = na < d.s[0].room ? na : d.s[0].room, ub = nb < d.s[1].room ? nb : d.s[1].room;
    if (ua > 0) {
        hipLaunchKernelGGL(pub_copy_new_kernel<true>, dim3(copy_blocks(d.s[0].rec_bytes / 16 * (size_t)ua)), dim3(256), 0, s, d);
        hipLaunchKernelGGL(pub_fix_new_kernel<true>, dim3((ua + 255) / 256), dim3(256), 0, s, d);
    }
    if (ub > 0) {
        hipLaunchKernelGGL(pub_copy_new_kernel<false>, dim3(copy_blocks(d.s[1].rec_bytes / 16 * (size_t)ub)), dim3(256), 0, s, d);
        hipLaunchKernelGGL(pub_fix_new_kernel<false>, dim3((ub + 255) / 256), dim3(256), 0, s, d);
        hipLaunchKernelGGL(pub_index_clear_kernel, dim3(copy_blocks((size_t)d.new_index.mask + 1)), dim3(256), 0, s, d);
        hipLaunchKernelGGL(pub_index_fill_kernel, dim3((d.mp_n + ub + 255) / 256), dim3(256), 0, s, d);
    }
    if (nc > 0) hipLaunchKernelGGL(pub_update_kernel<true>, dim3(wgs(nc)), dim3(PUB_WG), 0, s, d);
    if (nd > 0) hipLaunchKernelGGL(pub_update_kernel<false>, dim3(wgs(nd)), dim3(PUB_WG), 0, s, d);
}

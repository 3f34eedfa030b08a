// loopfix_kernels.hip -- a loop event on store records and the covisibility graph.  First the map update of RunGlobalBundleAdjustment (corbslam_server/src/
// GlobalOptimize.cpp:463-532, corbslam_client/src/LoopClosing.cc:684-753) over the spanning tree; CorrectLoop's propagation follows below.  The reference's queue is reproduced exactly: gather (poses, marks and the held children of every slot
// into compact arrays, so that the walk never touches the records' stride), fill (the children as slots), walk (ONE workgroup, generation by generation), commit, points.
// The arithmetic convention is stated in loopfix_internal.h.
#include "loopfix_internal.h"
#include "covis_device.h"
#include "sim3_math.h"
#include "normal_depth.h"

// o = A * B, 4x4 row-major
__device__ __forceinline__ void loopfix_mul44(const float* A, const float* B, float* o)
{
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            double s = __dmul_rn((double)A[r * 4], (double)B[c]);
            s = __fma_rn((double)A[r * 4 + 1], (double)B[4 + c], s);
            s = __fma_rn((double)A[r * 4 + 2], (double)B[8 + c], s);
            s = __fma_rn((double)A[r * 4 + 3], (double)B[12 + c], s);
            o[r * 4 + c] = (float)s;
        }
}
// (float)(R[r] . x) for a 3x3 R given by its entries
__device__ __forceinline__ float loopfix_dot3(float a, float b, float c, const float* x)
{
    double s = __dmul_rn((double)a, (double)x[0]);
    s = __fma_rn((double)b, (double)x[1], s);
    s = __fma_rn((double)c, (double)x[2], s);
    return (float)s;
}
// Twc as KeyFrame::SetPose leaves it (KeyFrame.cc:78-94): Rwc = Rcw^T, Ow = -(Rwc*tcw), Twc = [Rwc | Ow] over 0 0 0 1
__device__ __forceinline__ void loopfix_pose_inverse(const float* T, float* W)
{
    const float t[3] = { T[3], T[7], T[11] };
#pragma unroll
    for (int r = 0; r < 3; r++) {
        W[r * 4] = T[r]; W[r * 4 + 1] = T[4 + r]; W[r * 4 + 2] = T[8 + r];
        W[r * 4 + 3] = -loopfix_dot3(T[r], T[4 + r], T[8 + r], t);
    }
    W[12] = 0.f; W[13] = 0.f; W[14] = 0.f; W[15] = 1.f;
}
// pChild->mTcwGBA = (pChild->GetPose() * Twc) * pKF->mTcwGBA (:476-477)
__device__ __forceinline__ void loopfix_compose(const GbaDev& d, const float* Twc, int x, int ch)
{
    float Tc[16], G[16], A[16], o[16];
#pragma unroll
    for (int k = 0; k < 16; k++) { Tc[k] = d.Tcw[(size_t)ch * 16 + k]; G[k] = d.GBA[(size_t)x * 16 + k]; }
    loopfix_mul44(Tc, Twc, A);
    loopfix_mul44(A, G, o);
#pragma unroll
    for (int k = 0; k < 16; k++) d.GBA[(size_t)ch * 16 + k] = o[k];
}
__device__ __forceinline__ int loopfix_held(const CovisStores& S, unsigned long long id)
{
    if (id == COVIS_NO_ID) return -1;
    const int x = corb_idtab_find(S.kfid, id);
    return x >= 0 && x < S.kf_capacity ? x : -1;
}

// 16 lanes per slot: the three poses, the mark, the count of the children the store holds
__global__ __launch_bounds__(COVIS_T) void loopfix_gather_kernel(CovisTree T, int M, CovisStores S, const float* __restrict__ bef, GbaDev d)
{
    const int x = (blockIdx.x * COVIS_T + threadIdx.x) >> 4, l = threadIdx.x & 15;
    int c = 0;
    if (x < S.kf_capacity) {
        const KfHeader* h = covis_kf(S, x);
        d.Tcw[(size_t)x * 16 + l] = h->m.Tcw[l]; d.GBA[(size_t)x * 16 + l] = h->m.TcwGBA[l]; d.Bef[(size_t)x * 16 + l] = bef[(size_t)x * 16 + l];
        const int nc = min(max(T.n_child[x], 0), M);
        for (int i = l; i < nc; i += 16) if (loopfix_held(S, T.child_id[(size_t)x * M + i]) >= 0) c++;
    }
    c += __shfl_xor(c, 1); c += __shfl_xor(c, 2); c += __shfl_xor(c, 4); c += __shfl_xor(c, 8);      // the 16 lanes of a slot are neighbours in a wavefront
    if (x < S.kf_capacity && l == 0) {
        d.mark[x] = covis_kf(S, x)->m.ba_global_for_kf == d.loop_kf ? 1 : 0;
        d.cnt[x] = c;
        if (c) atomicAdd(&d.total[0], c);
    }
}
void loopfix_launch_gather(const CovisTree& T, int M, const CovisStores& S, const float* bef, const GbaDev& d, hipStream_t s)
{
    const long long n = (long long)S.kf_capacity * 16;
    hipLaunchKernelGGL(loopfix_gather_kernel, dim3((unsigned int)((n + COVIS_T - 1) / COVIS_T)), dim3(COVIS_T), 0, s, T, M, S, bef, d);
}

// a thread per slot: its stretch of `child` (where it lies depends on the order the cursor's atomics land in; what it holds does not), the set's order kept
__global__ __launch_bounds__(COVIS_T) void loopfix_fill_kernel(CovisTree T, int M, CovisStores S, GbaDev d)
{
    const int x = blockIdx.x * COVIS_T + threadIdx.x;
    if (x >= S.kf_capacity) return;
    const int c = d.cnt[x];
    if (c == 0) { d.off[x] = 0; return; }
    const int o = atomicAdd(&d.total[1], c);
    d.off[x] = o;
    const int nc = min(max(T.n_child[x], 0), M);
    int k = 0;
    for (int i = 0; i < nc && k < c; i++) {
        const int ch = loopfix_held(S, T.child_id[(size_t)x * M + i]);
        if (ch >= 0) d.child[o + k++] = ch;
    }
}
void loopfix_launch_fill(const CovisTree& T, int M, const CovisStores& S, const GbaDev& d, hipStream_t s)
{
    hipLaunchKernelGGL(loopfix_fill_kernel, dim3((S.kf_capacity + COVIS_T - 1) / COVIS_T), dim3(COVIS_T), 0, s, T, M, S, d);
}

// The queue of :464-488 on one workgroup.  A generation = the entries the previous generation pushed; a lane takes one entry (a wider generation goes in strides):
//   push     a workgroup prefix sum over the child counts gives every push its exact queue position; an unmarked child records the lowest position that lists it
//   compose  (after a barrier) the lister at that position computes the child's mTcwGBA and marks it -- the reference's first-come rule
//   pop      the first entry of a keyframe in the generation does mTcwBefGBA = Tcw, Tcw = mTcwGBA; a further entry of the same keyframe finds Tcw == mTcwGBA already
// A generation without unmarked children and without repeated keyframes -- the usual one -- passes three barriers.
// This equals the sequential walk whenever every entry of the generation is marked: then no entry's pose or mTcwGBA is written by another entry of the generation, and the
// composing entry is never a repeated one.  Every pushed entry is marked, so only the origins can fail that; a generation 0 with an unmarked origin is walked by one
// lane, literally.  A walk that needs more than queue_cap entries stops with status 1; the state it worked on is scratch, so nothing has been committed.
__global__ __launch_bounds__(COVIS_T) void loopfix_walk_kernel(CovisStores S, GbaDev d)
{
    __shared__ int sh_scan[COVIS_T / 64], sh_tail, sh_status, sh_prop, sh_reached, sh_flags[2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    GbaHead* head = d.head;
    int front = 0, tail = d.n_origins;
    if (tid == 0) { sh_tail = tail; sh_status = 0; sh_prop = 0; sh_reached = 0; sh_flags[0] = 0; sh_flags[1] = 0; }
    int unmarked = 0;
    for (int e = tid; e < tail; e += COVIS_T) if (!d.mark[d.queue[e]]) unmarked = 1;
    if (__syncthreads_or(unmarked)) {
        if (tid == 0) {
            int t = tail, prop = 0, status = 0;
            for (int e = 0; e < tail && !status; e++) {
                const int x = d.queue[e];
                float Twc[16], P[16];
#pragma unroll
                for (int k = 0; k < 16; k++) P[k] = d.Tcw[(size_t)x * 16 + k];
                loopfix_pose_inverse(P, Twc);
                const int c = d.cnt[x], o = d.off[x];
                if (t > d.queue_cap - c) { status = 1; break; }
                for (int i = 0; i < c; i++) {
                    const int ch = d.child[o + i];
                    if (!d.mark[ch]) { loopfix_compose(d, Twc, x, ch); d.mark[ch] = 1; prop++; }
                    d.queue[t++] = ch;
                }
#pragma unroll
                for (int k = 0; k < 16; k++) { d.Bef[(size_t)x * 16 + k] = d.Tcw[(size_t)x * 16 + k]; d.Tcw[(size_t)x * 16 + k] = d.GBA[(size_t)x * 16 + k]; }
                d.npop[x]++;
            }
            sh_tail = t; sh_prop = prop; sh_status = status;
        }
        __threadfence();
        __syncthreads();
        front = tail; tail = sh_tail;
    }
    // What a generation needs beyond push and pop is told by two flags the push pass raises (bit 0: an unmarked child was listed, bit 1: a keyframe has two entries in
    // the generation).  Every thread reads them after the barrier that ends the push, so every branch on them is uniform; the flags of the two parities of the
    // generation count alternate, and a slot is cleared one generation before it is raised again, behind a barrier every reader has passed.
    int gen = 0;
    while (front < tail && !sh_status) {
        const int gsize = tail - front;
        // ---- push ----
        int run = tail, raise = 0;
        bool full = false;
        for (int base = 0; base < gsize; base += COVIS_T) {
            const int e = base + tid;
            const int x = e < gsize ? d.queue[front + e] : -1;
            const int c = x >= 0 ? d.cnt[x] : 0;
            const int inc = lx_wave_incl_scan_i(c);
            if (lane == 63) sh_scan[w] = inc;
            __syncthreads();
            int before = 0, total = 0;
            for (int i = 0; i < COVIS_T / 64; i++) { if (i < w) before += sh_scan[i]; total += sh_scan[i]; }
            if (base + COVIS_T < gsize) __syncthreads();                                       // (sh_scan is written again by the next stride only; uniform)
            if (run > d.queue_cap - total) { full = true; break; }                             // uniform
            if (x >= 0) {
                const int pos = run + before + inc - c, o = d.off[x];
                for (int i = 0; i < c; i++) {
                    const int ch = d.child[o + i];
                    d.queue[pos + i] = ch;
                    if (!d.mark[ch]) { atomicMin(&d.winner[ch], front + e); raise |= 1; }
                }
                if (atomicMin(&d.first[x], front + e) != LOOPFIX_UNSEEN) raise |= 2;              // the later of two entries of one keyframe sees the earlier one's mark
                atomicAdd(&d.npop[x], 1);
            }
            run += total;
        }
        if (full) { if (tid == 0) sh_status = 1; __syncthreads(); break; }
        if (raise) atomicOr(&sh_flags[gen & 1], raise);
        __threadfence();
        __syncthreads();
        const int flags = sh_flags[gen & 1];
        // ---- compose ----
        int prop = 0;
        if (flags & 1) for (int e = tid; e < gsize; e += COVIS_T) {
            const int x = d.queue[front + e], c = d.cnt[x], o = d.off[x];
            bool have = false;
            float Twc[16];
            for (int i = 0; i < c; i++) {
                const int ch = d.child[o + i];
                if (__hip_atomic_load(&d.winner[ch], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != front + e) continue;
                if (!have) {
                    float P[16];
#pragma unroll
                    for (int k = 0; k < 16; k++) P[k] = d.Tcw[(size_t)x * 16 + k];
                    loopfix_pose_inverse(P, Twc); have = true;
                }
                loopfix_compose(d, Twc, x, ch);
                d.mark[ch] = 1; prop++;
            }
        }
        if (prop) atomicAdd(&sh_prop, prop);
        if (flags & 1) { __threadfence(); __syncthreads(); }                                   // the pops below write the poses the compositions read
        // ---- pop: the first entry of a keyframe in this generation ----
        for (int e = tid; e < gsize; e += COVIS_T) {
            const int x = d.queue[front + e];
            if (__hip_atomic_load(&d.first[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != front + e) continue;
#pragma unroll
            for (int k = 0; k < 16; k++) { d.Bef[(size_t)x * 16 + k] = d.Tcw[(size_t)x * 16 + k]; d.Tcw[(size_t)x * 16 + k] = d.GBA[(size_t)x * 16 + k]; }
            if (!(flags & 2)) d.first[x] = LOOPFIX_UNSEEN;                                     // every keyframe has one entry: its thread is the only reader
        }
        if (tid == 0) sh_flags[(gen + 1) & 1] = 0;
        gen++;
        __threadfence();
        __syncthreads();
        if (!(flags & 2)) { front = tail; tail = run; continue; }                              // uniform
        // ---- pop: its further entries (several of them write the same values) ----
        for (int e = tid; e < gsize; e += COVIS_T) {
            const int x = d.queue[front + e];
            if (__hip_atomic_load(&d.first[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == front + e) continue;
#pragma unroll
            for (int k = 0; k < 16; k++) d.Bef[(size_t)x * 16 + k] = d.Tcw[(size_t)x * 16 + k];
        }
        __threadfence();
        __syncthreads();
        for (int e = tid; e < gsize; e += COVIS_T) d.first[d.queue[front + e]] = LOOPFIX_UNSEEN;
        __threadfence();
        __syncthreads();
        front = tail; tail = run;
    }
    __syncthreads();
    int reached = 0;
    for (int x = tid; x < S.kf_capacity; x += COVIS_T) if (__hip_atomic_load(&d.npop[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0) reached++;
    if (reached) atomicAdd(&sh_reached, reached);
    __syncthreads();
    if (tid == 0) {
        head->status = sh_status;
        head->n_popped = sh_status ? 0 : tail; head->n_reached = sh_status ? 0 : sh_reached; head->n_propagated = sh_status ? 0 : sh_prop;
        head->n_revisited = sh_status ? 0 : tail - sh_reached;
    }
}
void loopfix_launch_walk(const CovisStores& S, const GbaDev& d, hipStream_t s)
{
    hipLaunchKernelGGL(loopfix_walk_kernel, dim3(1), dim3(COVIS_T), 0, s, S, d);
}

// 16 lanes per slot the walk popped
__global__ __launch_bounds__(COVIS_T) void loopfix_commit_kernel(CovisStores S, float* __restrict__ bef, GbaDev d)
{
    if (d.head->status) return;
    const int x = (blockIdx.x * COVIS_T + threadIdx.x) >> 4, l = threadIdx.x & 15;
    if (x >= S.kf_capacity || d.npop[x] <= 0) return;
    KfHeader* h = const_cast<KfHeader*>(covis_kf(S, x));
    h->m.Tcw[l] = d.Tcw[(size_t)x * 16 + l]; h->m.TcwGBA[l] = d.GBA[(size_t)x * 16 + l]; bef[(size_t)x * 16 + l] = d.Bef[(size_t)x * 16 + l];
    if (l == 0 && d.mark[x]) h->m.ba_global_for_kf = d.loop_kf;
}
void loopfix_launch_commit(const CovisStores& S, float* bef, const GbaDev& d, hipStream_t s)
{
    const long long n = (long long)S.kf_capacity * 16;
    hipLaunchKernelGGL(loopfix_commit_kernel, dim3((unsigned int)((n + COVIS_T - 1) / COVIS_T)), dim3(COVIS_T), 0, s, S, bef, d);
}

// :492-532, a thread per slot of the map-point index; the keyframes' state is read from the walk's compact arrays
__global__ __launch_bounds__(COVIS_T) void loopfix_points_kernel(CovisStores S, int mp_first, int mp_n, GbaDev d)
{
    __shared__ int sh[3];
    if (d.head->status) return;
    if (threadIdx.x < 3) sh[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * COVIS_T + threadIdx.x;
    if (i < mp_n) {
        CorbMapPointRecord* r = reinterpret_cast<CorbMapPointRecord*>(const_cast<char*>(S.mp_base) + (size_t)(mp_first + i) * S.mp_bytes);
        if (!(r->flags & CORB_MP_BAD)) {                                                       // :498
            if (r->ba_global_for_kf == d.loop_kf) {                                            // :501-506
                r->world_pos[0] = r->pos_gba[0]; r->world_pos[1] = r->pos_gba[1]; r->world_pos[2] = r->pos_gba[2];
                atomicAdd(&sh[0], 1);
            } else {
                const int x = loopfix_held(S, r->ref_kf_id);                                   // :510-515
                if (x < 0 || !d.mark[x]) atomicAdd(&sh[2], 1);
                else {
                    float B[16], P[16], W[16];
#pragma unroll
                    for (int k = 0; k < 16; k++) { B[k] = d.Bef[(size_t)x * 16 + k]; P[k] = d.Tcw[(size_t)x * 16 + k]; }
                    loopfix_pose_inverse(P, W);                                                // pRefKF->GetPoseInverse()
                    const float p[3] = { r->world_pos[0], r->world_pos[1], r->world_pos[2] };
                    float Xc[3];
#pragma unroll
                    for (int k = 0; k < 3; k++) Xc[k] = __fadd_rn(loopfix_dot3(B[k * 4], B[k * 4 + 1], B[k * 4 + 2], p), B[k * 4 + 3]);      // Rcw*p + tcw (:518-520)
#pragma unroll
                    for (int k = 0; k < 3; k++) r->world_pos[k] = __fadd_rn(loopfix_dot3(W[k * 4], W[k * 4 + 1], W[k * 4 + 2], Xc), W[k * 4 + 3]);   // Rwc*Xc + twc (:527)
                    atomicAdd(&sh[1], 1);
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sh[0]) atomicAdd(&d.head->n_points_set, sh[0]);
        if (sh[1]) atomicAdd(&d.head->n_points_moved, sh[1]);
        if (sh[2]) atomicAdd(&d.head->n_points_skipped, sh[2]);
    }
}
void loopfix_launch_points(const CovisStores& S, int mp_first, int mp_n, const GbaDev& d, hipStream_t s)
{
    if (mp_n > 0) hipLaunchKernelGGL(loopfix_points_kernel, dim3((mp_n + COVIS_T - 1) / COVIS_T), dim3(COVIS_T), 0, s, S, mp_first, mp_n, d);
}

// ------------------------------------------------------------------------------------------------
// CorrectLoop's propagation (GlobalOptimize.cpp:253-338 = LoopClosing.cc:436-522).  CorrectedSim3 is a pointer-keyed std::map in the reference; the walk here is in
// ascending keyframe id.  A point is corrected by the first member in walk order that holds it: a min-reduction of the walk position per point.
extern __shared__ unsigned long long loopfix_lds[];
size_t loopfix_set_lds_bytes(int M) { return (size_t)covis_pow2(M + 1) * 12; }

__device__ __forceinline__ void loopfix_sim3_from_pose(const float* T, S3State& S)
{
    const double R[9] = { T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10] };              // Converter::toMatrix3d / toVector3d
    quat_from_R(R, S.q);
    S.t[0] = T[3]; S.t[1] = T[7]; S.t[2] = T[11]; S.s = 1.0;
}

__global__ __launch_bounds__(COVIS_T) void loopfix_set_kernel(CovisStores S, LcDev d, int P)
{
    unsigned long long* sid = loopfix_lds;
    int* sslot = reinterpret_cast<int*>(sid + P);
    const int tid = threadIdx.x;
    const int nq = min(max(d.q_n[0], 0), P - 1), n = nq + 1;
    for (int i = tid; i < P; i += COVIS_T) {                                                    // mvpCurrentConnectedKFs.push_back(mpCurrentKF) (:255)
        const int x = i < nq ? d.q_slots[i] : (i == nq ? d.cur_slot : -1);
        sslot[i] = x; sid[i] = x >= 0 ? covis_kf(S, x)->m.id : COVIS_NO_ID;
    }
    __syncthreads();
    covis_sort_by_id(sid, sslot, P);
    if (tid == 0) d.count[0] = n;
    if (n > d.cap) return;
    float Tc[16], Twc[16];
#pragma unroll
    for (int k = 0; k < 16; k++) Tc[k] = covis_kf(S, d.cur_slot)->m.Tcw[k];
    loopfix_pose_inverse(Tc, Twc);                                                              // mpCurrentKF->GetPoseInverse() (:259)
    S3State scw; s3_load(d.Scw, scw);
    for (int i = tid; i < n; i += COVIS_T) {
        const int x = sslot[i];
        d.set[i] = x; d.pos[x] = i;
        float Tiw[16];
#pragma unroll
        for (int k = 0; k < 16; k++) Tiw[k] = covis_kf(S, x)->m.Tcw[k];
        S3State non, cor, inv;
        loopfix_sim3_from_pose(Tiw, non);                                                       // :282-286
        if (x != d.cur_slot) {                                                                  // :271-280
            float Tic[16]; S3State sic;
            loopfix_mul44(Tiw, Twc, Tic);
            loopfix_sim3_from_pose(Tic, sic);
            s3_mul(sic, scw, cor);
        } else cor = scw;                                                                       // :258
        s3_inv(cor, inv);                                                                       // :294
        double* o = d.sim3 + (size_t)i * LOOPFIX_SIM3_DOUBLES;
        s3_store(cor, o); s3_store(non, o + 8); s3_store(inv, o + 16);
        double R[9]; quat_to_R(cor.q, R);                                                       // :324-330: [R | t * (1./s)]
        const double k = 1. / cor.s;
        float* T = d.newT + (size_t)i * 16;
#pragma unroll
        for (int r = 0; r < 3; r++) { T[r * 4] = (float)R[r * 3]; T[r * 4 + 1] = (float)R[r * 3 + 1]; T[r * 4 + 2] = (float)R[r * 3 + 2]; T[r * 4 + 3] = (float)(cor.t[r] * k); }
        T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
    }
}
void loopfix_launch_set(const CovisStores& S, int M, const LcDev& d, hipStream_t s)
{
    hipLaunchKernelGGL(loopfix_set_kernel, dim3(1), dim3(COVIS_T), loopfix_set_lds_bytes(M), s, S, d, covis_pow2(M + 1));
}

// blockIdx.y = position in the walk, threads over that keyframe's features
__global__ __launch_bounds__(COVIS_T) void loopfix_corrector_kernel(CovisStores S, LcDev d)
{
    const int n = d.count[0], w = blockIdx.y;
    if (n > d.cap || w >= n) return;
    const int x = d.set[w], f = blockIdx.x * COVIS_T + threadIdx.x;
    if (f >= covis_kf_n(S, x)) return;
    const RecLayout KL(S.F); const MpLayout ML(S.O);
    int ms = -1;
    const char* r = covis_good_point(S, reinterpret_cast<const unsigned long long*>(S.kf_base + (size_t)x * S.kf_bytes + KL.mp_id)[f], &ms);      // :302-305
    if (!r) return;
    if (reinterpret_cast<const CorbMapPointScratch*>(r + ML.scratch)->corrected_by_kf == covis_kf(S, d.cur_slot)->m.id) return;                      // :306, as on entry
    atomicMin(&d.corrector[ms], w);
}
// the poses UpdateNormalAndDepth (:320) meets in the middle of the walk: a member before the corrector has its corrected pose, everybody else the record's
struct LcPoseLookup {
    const CovisStores& S; const LcDev& d; int w;
    __device__ __forceinline__ int find(unsigned long long id) const { return loopfix_held(S, id); }
    __device__ __forceinline__ const float* pose(int x) const { const int pw = d.pos[x]; return pw < w ? d.newT + (size_t)pw * 16 : covis_kf(S, x)->m.Tcw; }
    __device__ __forceinline__ const char* record(int x) const { return S.kf_base + (size_t)x * S.kf_bytes; }
};
__global__ __launch_bounds__(COVIS_T) void loopfix_move_kernel(CovisStores S, LcDev d)
{
    const int ms = blockIdx.x * COVIS_T + threadIdx.x;
    if (ms >= S.mp_capacity) return;
    const int w = d.corrector[ms];
    if (w == LOOPFIX_UNSEEN) return;
    char* rec = const_cast<char*>(S.mp_base) + (size_t)ms * S.mp_bytes;
    CorbMapPointRecord* h = reinterpret_cast<CorbMapPointRecord*>(rec);
    const MpLayout ML(S.O); const RecLayout KL(S.F);
    S3State non, inv;
    s3_load(d.sim3 + (size_t)w * LOOPFIX_SIM3_DOUBLES + 8, non); s3_load(d.sim3 + (size_t)w * LOOPFIX_SIM3_DOUBLES + 16, inv);
    const double p[3] = { h->world_pos[0], h->world_pos[1], h->world_pos[2] };
    double a[3], b[3];
    s3_map(non, p, a); s3_map(inv, a, b);                                                       // g2oCorrectedSwi.map(g2oSiw.map(eigP3Dw)) (:312)
    h->world_pos[0] = (float)b[0]; h->world_pos[1] = (float)b[1]; h->world_pos[2] = (float)b[2];
    CorbMapPointScratch* sc = reinterpret_cast<CorbMapPointScratch*>(rec + ML.scratch);
    sc->corrected_by_kf = covis_kf(S, d.cur_slot)->m.id;                                        // :318-319
    sc->corrected_reference = covis_kf(S, d.set[w])->m.id;
    atomicAdd(&d.count[1], 1);
    if (d.scale_factor > 0.f)
        corb_update_normal_depth(LcPoseLookup{S, d, w}, h, reinterpret_cast<const unsigned long long*>(rec + ML.obs_kf), reinterpret_cast<const uint32_t*>(rec + ML.obs_idx),
                                 covis_n_obs(S, rec), KL, d.scale_factor);
}
// pKFi->SetPose(correctedTiw) (:332): 16 lanes per member, after every point has been moved
__global__ __launch_bounds__(COVIS_T) void loopfix_setpose_kernel(CovisStores S, LcDev d)
{
    const int n = d.count[0], i = (blockIdx.x * COVIS_T + threadIdx.x) >> 4, l = threadIdx.x & 15;
    if (n > d.cap || i >= n) return;
    const_cast<KfHeader*>(covis_kf(S, d.set[i]))->m.Tcw[l] = d.newT[(size_t)i * 16 + l];
}
void loopfix_launch_correct(const CovisStores& S, int M, const LcDev& d, hipStream_t s)
{
    hipLaunchKernelGGL(loopfix_corrector_kernel, dim3((S.F + COVIS_T - 1) / COVIS_T, M + 1), dim3(COVIS_T), 0, s, S, d);
    hipLaunchKernelGGL(loopfix_move_kernel, dim3((S.mp_capacity + COVIS_T - 1) / COVIS_T), dim3(COVIS_T), 0, s, S, d);
    hipLaunchKernelGGL(loopfix_setpose_kernel, dim3(((M + 1) * 16 + COVIS_T - 1) / COVIS_T), dim3(COVIS_T), 0, s, S, d);
}

// loopdetect_kernels.hip -- LoopClosing::DetectLoop on records for gfx950 (include/corb_loop_detect.h; definition: tests/loopdetect_reference.py).  Per keyframe, in
// stream order, every kernel a no-op once the queue's stop flag is set:
//   ld_begin_kernel      : one workgroup.  mnId from the record header and the gap test (LoopClosing.cc:111); GetVectorCovisibleKeyFrames() of the row without the bad
//                          records as database entries for the minScore loop (:122-137); GetConnectedKeyFrames() as the database's connected flags (:141).  An
//                          unbound covisible slot ends the queue before anything has changed.  Fills the BowLoopQuery the database's kernels read
//   (kfdb_*_q_kernel)    : bow_kernels.hip: the scores, their minimum, DetectLoopCandidates with it
//   ld_cand_kernel       : one workgroup per candidate: its group -- the held ids of its row's weight map and itself -- as a bit set over the store's slots
//   ld_consistent_kernel : one wavefront per (candidate, previous group): lanes over the 64-bit words of the two sets, a ballot over "the words share a bit"
//   ld_close_kernel      : one workgroup: the serial loop of :157-212 in closed form.  Previous group iG gives one new group, that of the FIRST candidate consistent with
//                          it (a minimum per group); a candidate consistent with none gives its own with counter 0; a candidate's new groups are counted, the counts
//                          scanned into offsets, so the new vector stands in (candidate, iG, counter-0 last) order without a replay; "enough" is a flag per candidate,
//                          scanned into the list.  Then the groups' bits are copied into the other buffer, the buffers swap, the keyframe's entry goes live (:217)
//                          and the outcome is written.  A capacity error leaves all of that undone and sets the stop flag
// All bounds come from the handle (max_candidates, max_groups, the store's slots, the database's entries); ids and entries read from memory are range-checked
// before they index anything.  No scalar memory writes, no device-side printf / assert; every launch is on the caller's stream.
#include "loopdetect_internal.h"
#include "covis_device.h"
#include <climits>

namespace {

__device__ __forceinline__ const KfHeader* ld_kf(const LdDev& d, int slot) { return reinterpret_cast<const KfHeader*>(d.kf_base + (size_t)slot * d.kf_bytes); }
// the slot that holds the id, or -1 (Cache::KeyFrameInCache)
__device__ __forceinline__ int ld_slot_of(const LdDev& d, unsigned long long id)
{
    const int x = corb_idtab_find(d.kfid, id);
    return (x >= 0 && x < d.n_slots) ? x : -1;
}
__device__ __forceinline__ int ld_entry_of(const LdDev& d, int slot)
{
    const int e = d.slot_entry[slot];
    return (e >= 0 && e < d.n_entries) ? e : -1;
}

__global__ __launch_bounds__(LD_T) void ld_begin_kernel(LdDev d, BowDbDev db, int k, int slot)
{
    __shared__ int sh_err, sh_ns, sh_nc;
    const int tid = threadIdx.x, M = d.R.M;
    const int stop = d.head()->stop;
    if (tid == 0) { sh_err = 0; sh_ns = 0; sh_nc = 0; }
    __syncthreads();
    if (stop) { if (tid == 0) d.q->skip = 1; return; }
    const unsigned long long id = ld_kf(d, slot)->m.id;
    if (id < d.st->last_loop + 10ull) {                                                         // :111
        if (tid == 0) { d.q->skip = 1; d.st->mode = LD_MODE_GAP; }
        return;
    }
    // :122-137 vpConnectedKeyFrames = GetVectorCovisibleKeyFrames(); isBad() is skipped.  The minimum does not depend on the order the scores are listed in
    const size_t row = (size_t)slot * M;
    const int n_ord = min(max(d.R.n_ord[slot], 0), M);
    for (int i = tid; i < n_ord; i += LD_T) {
        const int x = ld_slot_of(d, d.R.ord_id[row + i]);
        if (x < 0 || (ld_kf(d, x)->m.flags & CORB_KF_BAD)) continue;
        const int e = ld_entry_of(d, x);
        if (e < 0 || db.n_words[e] < 0) { sh_err = 1; continue; }
        d.score_list[atomicAdd(&sh_ns, 1)] = e;
    }
    __syncthreads();
    if (sh_err) {                                                                               // nothing has changed yet
        if (tid == 0) { d.q->skip = 1; d.st->mode = LD_MODE_ERR; d.item(k)->status = CORB_ERR_ARG; d.head()->stop = 1; }
        return;
    }
    // :141 spConnectedKeyFrames = GetConnectedKeyFrames(): the whole weight map; a keyframe without an entry cannot be in the database
    const int n_all = min(max(d.R.n_all[slot], 0), M);
    for (int i = tid; i < n_all; i += LD_T) {
        const int x = ld_slot_of(d, d.R.all_id[row + i]);
        const int e = x >= 0 ? ld_entry_of(d, x) : -1;
        if (e < 0) continue;
        const int at = atomicAdd(&sh_nc, 1);
        if (at < db.capacity) { db.conn_list[at] = e; db.conn[e] = 1; }
    }
    __syncthreads();
    if (tid == 0) {
        BowLoopQuery* q = d.q;
        q->skip = 0; q->n_score = sh_ns; q->n_conn = min(sh_nc, db.capacity); q->min_score = 1.0f; q->id = id;
        d.st->mode = LD_MODE_FULL;
    }
}

// this keyframe's candidates, or -1 when the keyframe takes no consistency pass (stopped, gap, error, more candidates than there is room for)
__device__ __forceinline__ int ld_candidates(const LdDev& d, const BowDbDev& db)
{
    if (d.head()->stop || d.st->mode != LD_MODE_FULL) return -1;
    const int n = db.out[0];
    return (n > d.max_cand || n < 0) ? -1 : n;
}

__global__ __launch_bounds__(LD_T) void ld_cand_kernel(LdDev d, BowDbDev db, int k)
{
    const int c = blockIdx.x, tid = threadIdx.x, M = d.R.M, W = d.W;
    if (c >= ld_candidates(d, db)) return;
    const int e = db.out[1 + c];
    const int x = (e >= 0 && e < d.n_entries) ? d.entry_slot[e] : -1;
    const int slot = (x >= 0 && x < d.n_slots) ? x : -1;
    unsigned long long* bits = d.cand_bits + (size_t)c * W;
    for (int w = tid; w < W; w += LD_T) bits[w] = 0ull;
    __syncthreads();
    if (tid == 0) { d.item_ints(k, 0)[c] = e; d.item_ints(k, 1)[c] = slot; }
    if (slot < 0) return;
    if (tid == 0) atomicOr(&bits[slot >> 6], 1ull << (slot & 63));                              // spCandidateGroup.insert(pCandidateKF) (:166)
    const size_t row = (size_t)slot * M;
    const int n_all = min(max(d.R.n_all[slot], 0), M);
    for (int i = tid; i < n_all; i += LD_T) {                                                   // GetConnectedKeyFrames() (:165)
        const int y = ld_slot_of(d, d.R.all_id[row + i]);
        if (y >= 0) atomicOr(&bits[y >> 6], 1ull << (y & 63));
    }
}

__global__ __launch_bounds__(LD_T) void ld_consistent_kernel(LdDev d, BowDbDev db)
{
    const int pair = blockIdx.x * (LD_T / 64) + (int)threadIdx.x / 64, lane = threadIdx.x & 63;
    const int i = pair / d.max_groups, g = pair % d.max_groups;
    const int n_cand = ld_candidates(d, db);
    if (i >= n_cand || g >= d.st->n_groups) return;
    const unsigned long long* a = d.cand_bits + (size_t)i * d.W;
    const unsigned long long* b = d.grp_bits + ((size_t)d.st->cur * d.max_groups + g) * d.W;
    bool share = false;
    for (int w = lane; w < d.W; w += 64) share = share || (a[w] & b[w]) != 0ull;
    const unsigned long long m = __ballot(share);
    if (lane == 0) d.cons[(size_t)i * d.max_groups + g] = m != 0ull ? 1 : 0;
}

__global__ __launch_bounds__(LD_T) void ld_close_kernel(LdDev d, BowDbDev db, int k, int entry, unsigned int seq)
{
    __shared__ int sh_scan[LD_T / 64];
    const int tid = threadIdx.x, W = d.W, MG = d.max_groups;
    LdHead* H = d.head(); LdState* st = d.st; LdItem* it = d.item(k);
    const int stop = H->stop, mode = st->mode;
    const int n_cand = (!stop && mode == LD_MODE_FULL) ? db.out[0] : 0;
    const int G = min(max(st->n_groups, 0), MG), cur = st->cur & 1, th = st->th;
    __syncthreads();
    if (stop || mode == LD_MODE_ERR) return;
    // :113, :147, :217 mpKeyFrameDB->add(mpCurrentKF), and what the caller reads
    auto finish = [&](int outcome, int n_enough, int n_groups) {
        db.live[entry] = 1; db.seq[entry] = seq;
        it->r.outcome = outcome; it->r.min_score_bits = mode == LD_MODE_GAP ? 0u : __float_as_uint(d.q->min_score);
        it->r.n_candidates = n_cand; it->r.n_enough = n_enough; it->r.n_groups = n_groups; it->status = CORB_OK;
        H->consumed = k + 1;
        if (outcome == CORB_LOOP_DETECTED) H->stop = 1;
    };
    auto refuse = [&](int which) {
        it->r.n_candidates = n_cand; it->r.n_groups = G; it->r.min_score_bits = __float_as_uint(d.q->min_score); it->status = CORB_ERR_CAPACITY; it->pad[0] = which;
        H->stop = 1;
    };
    if (mode == LD_MODE_GAP) { if (tid == 0) finish(CORB_LOOP_GAP, 0, G); return; }
    if (n_cand > d.max_cand || n_cand < 0) { if (tid == 0) refuse(1); return; }
    if (n_cand == 0) { if (tid == 0) { st->n_groups = 0; finish(CORB_LOOP_NONE, 0, 0); } return; }      // :144-151 mvConsistentGroups.clear()

    const int* cnt = d.grp_cnt + (size_t)cur * MG;
    for (int g = tid; g < G; g += LD_T) {                                                       // vbConsistentGroup[iG]: set by the first consistent candidate (:189-194)
        int f = INT_MAX;
        for (int i = 0; i < n_cand; i++) if (d.cons[(size_t)i * MG + g]) { f = i; break; }
        d.first[g] = f;
    }
    __syncthreads();
    for (int i = tid; i < n_cand; i += LD_T) {
        int groups = 0, any = 0, en = 0;
        for (int g = 0; g < G; g++) if (d.cons[(size_t)i * MG + g]) {
            any = 1;                                                                            // bConsistentForSomeGroup
            if (cnt[g] + 1 >= th) en = 1;                                                       // nCurrentConsistency >= mnCovisibilityConsistencyTh (:195)
            if (d.first[g] == i) groups++;
        }
        d.pos[i] = groups + (any ? 0 : 1); d.any[i] = any; d.en[i] = en; d.epos[i] = en;       // :204-208 the counter-0 group
    }
    __syncthreads();
    const int total = covis_block_scan(d.pos, n_cand, sh_scan);
    const int n_enough = covis_block_scan(d.epos, n_cand, sh_scan);
    if (total > MG) { if (tid == 0) refuse(2); return; }
    const int nb = cur ^ 1;
    int* ncnt = d.grp_cnt + (size_t)nb * MG;
    int* enough = d.item_ints(k, 2);
    for (int i = tid; i < n_cand; i += LD_T) {
        int p = d.pos[i];
        for (int g = 0; g < G; g++) if (d.first[g] == i) { d.src[p] = i; ncnt[p] = cnt[g] + 1; p++; }
        if (!d.any[i]) { d.src[p] = i; ncnt[p] = 0; }
        if (d.en[i]) enough[d.epos[i]] = i;                                                     // mvpEnoughConsistentCandidates, once per candidate (:195-199)
    }
    __syncthreads();
    unsigned long long* nbits = d.grp_bits + (size_t)nb * MG * W;
    for (int j = tid; j < total * W; j += LD_T) nbits[j] = d.cand_bits[(size_t)d.src[j / W] * W + j % W];
    __syncthreads();
    if (tid == 0) {                                                                             // :212 mvConsistentGroups = vCurrentConsistentGroups
        st->cur = nb; st->n_groups = total;
        finish(n_enough > 0 ? CORB_LOOP_DETECTED : CORB_LOOP_NOT_ENOUGH, n_enough, total);
    }
}

__global__ __launch_bounds__(LD_T) void ld_drop_slot_kernel(LdDev d, int slot)
{
    const int g = blockIdx.x * LD_T + threadIdx.x;
    if (g < 2 * d.max_groups) d.grp_bits[(size_t)g * d.W + (slot >> 6)] &= ~(1ull << (slot & 63));
}

}  // namespace

void ld_launch_begin(const LdDev& d, const BowDbDev& db, int k, int slot, hipStream_t s)
{
    hipLaunchKernelGGL(ld_begin_kernel, dim3(1), dim3(LD_T), 0, s, d, db, k, slot);
}
void ld_launch_groups(const LdDev& d, const BowDbDev& db, int k, hipStream_t s)
{
    hipLaunchKernelGGL(ld_cand_kernel, dim3(d.max_cand), dim3(LD_T), 0, s, d, db, k);
    const long long pairs = (long long)d.max_cand * d.max_groups;
    hipLaunchKernelGGL(ld_consistent_kernel, dim3((unsigned)((pairs + LD_T / 64 - 1) / (LD_T / 64))), dim3(LD_T), 0, s, d, db);
}
void ld_launch_close(const LdDev& d, const BowDbDev& db, int k, int entry, unsigned int seq, hipStream_t s)
{
    hipLaunchKernelGGL(ld_close_kernel, dim3(1), dim3(LD_T), 0, s, d, db, k, entry, seq);
}
void ld_launch_drop_slot(const LdDev& d, int slot, hipStream_t s)
{
    hipLaunchKernelGGL(ld_drop_slot_kernel, dim3((2 * d.max_groups + LD_T - 1) / LD_T), dim3(LD_T), 0, s, d, slot);
}

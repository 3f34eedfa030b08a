// corb_localmap.cpp -- Tracking::UpdateLocalMap on the device-resident stores (include/corb_accel.h, last section): host side of localmap_kernels.hip.
// One vote-and-walk workgroup, the ordered unique compaction of the local points (the window's, covis_kernels.hip), a finish launch and ONE read-back; the true counts
// stay on the device until then, so the launch sizes come from the caller's caps.
#include "localmap_internal.h"
#include "covis_host.h"
#include <vector>
#include <algorithm>

static_assert(sizeof(CorbLocalMap) == 32 && offsetof(LocalMapHead, status) == 32, "LocalMapHead starts with CorbLocalMap");

extern "C" int corb_track_update_local_map(CorbCovis* g, CorbKfStore* frames, int slot, const int32_t* prev_kf_slots, int n_prev, int32_t* kf_slots, int kf_cap,
                                           int32_t* mp_slots, uint64_t* mp_ids, int mp_cap, CorbLocalMap* out)
{
    const char* who = "corb_track_update_local_map";
    if (!g || !frames || !out || slot < 0 || slot >= frames->capacity || n_prev < 0 || (n_prev > 0 && !prev_kf_slots) || kf_cap < 0 || mp_cap < 0 || (kf_cap > 0 && !kf_slots) ||
        (mp_cap > 0 && (!mp_slots || !mp_ids))) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    if (frames->device != g->kf->device) { corb_set_error("%s: the stores live on different devices", who); return CORB_ERR_ARG; }
    for (int i = 0; i < n_prev; i++) if (prev_kf_slots[i] < 0 || prev_kf_slots[i] >= g->kf->capacity) { corb_set_error("%s: previous local keyframe %d is not a slot of the graph's store", who, i); return CORB_ERR_ARG; }
    int rc = corb_select_device(g->kf->device); if (rc) return rc;
    CovisCall c; rc = c.begin(g, who, true, frames); if (rc) return rc;
    // under the locks: the frame's slot and the previous local keyframes hold filled records (as the other calls on records ask of their slots)
    if (record_slot_count(who, frames, slot) < 0) return CORB_ERR_ARG;
    for (int i = 0; i < n_prev; i++) if (g->kf->host[prev_kf_slots[i]].n < 0) { corb_set_error("%s: previous local keyframe %d (slot %d) is an empty slot", who, i, prev_kf_slots[i]); return CORB_ERR_ARG; }
    CorbScratch& pool = *c.scratch;
    const int M = g->R.M, K = g->kf->capacity;
    LocalMapDev d{};
    d.frame_rec = frames->rec(slot); d.F_frame = frames->F; d.n_prev = n_prev; d.kf_cap = kf_cap; d.mp_cap = mp_cap;
    d.list_cap = std::max(std::max(M, LOCALMAP_MAX_KFS + 3), n_prev);
    CovisWindow w{};
    w.kf_cap = d.list_cap; w.mp_cap = mp_cap;
    w.local_bound = std::min(d.list_cap, kf_cap);
    const long long n1 = (long long)w.local_bound * g->kf->F;
    if (n1 >= COVIS_UNSEEN) { corb_set_error("%s: the caps allow %lld candidates, more than a 32-bit position holds", who, n1); return CORB_ERR_ARG; }
    w.mp_bound = (int)std::min<long long>(std::min<long long>(mp_cap, n1), g->mp->capacity);
    int* dprev = nullptr;
    if (n_prev > 0) HIPCHK(pool.upload(&dprev, prev_kf_slots, (size_t)n_prev)); else HIPCHK(pool.alloc(&dprev, 1));
    d.prev = dprev;
    HIPCHK(pool.alloc(&d.votes, (size_t)2 * K)); d.mark = d.votes + K;
    HIPCHK(pool.alloc(&d.kf_out, (size_t)d.list_cap)); HIPCHK(pool.alloc(&d.mp_out, (size_t)mp_cap)); HIPCHK(pool.alloc(&d.mp_ids, (size_t)mp_cap));
    HIPCHK(pool.alloc(&d.counts, 4)); HIPCHK(pool.alloc(&d.head, 1));
    HIPCHK(pool.alloc(&w.first_mp, (size_t)g->mp->capacity));
    HIPCHK(pool.alloc(&w.flag, (size_t)n1 + 1)); HIPCHK(pool.alloc(&w.pos, (size_t)n1 + 1)); HIPCHK(pool.alloc(&w.scan_scratch, corb_scan_scratch_ints((size_t)std::max<long long>(n1, 1))));
    w.kf_out = d.kf_out; w.mp_out = d.mp_out; w.counts = d.counts;
    HIPCHK(hipMemsetAsync(d.votes, 0, (size_t)2 * K * 4, pool.stream));
    HIPCHK(hipMemsetAsync(d.counts, 0, 16, pool.stream));
    HIPCHK(hipMemsetAsync(d.head, 0, sizeof(LocalMapHead), pool.stream));
    HIPCHK(hipMemsetAsync(w.first_mp, 0x7F, (size_t)g->mp->capacity * 4, pool.stream));
    localmap_launch_vote_walk(g->R, g->T, c.S, d, pool.stream);                                   // UpdateLocalKeyFrames
    covis_launch_window_points(c.S, w, pool.stream);                                              // UpdateLocalPoints: first occurrence in (list order, feature order)
    localmap_launch_finish(c.S, d, std::max(frames->F, w.mp_bound), pool.stream);
    HIPCHK(hipGetLastError());
    // the one read-back: the head and the lists up to the caps -- 4 bytes per keyframe of kf_cap and 12 per point of mp_cap travel whatever the lists hold, so a
    // caller sizes mp_cap for its local map (a few thousand points), not for the store
    LocalMapHead head{};
    const int kf_read = std::min(d.list_cap, kf_cap), mp_read = w.mp_bound;
    std::vector<int32_t> h_kf((size_t)kf_read), h_mp((size_t)mp_read); std::vector<uint64_t> h_id((size_t)mp_read);
    HIPCHK(pool.d2h(&head, d.head, sizeof(head)));
    HIPCHK(pool.d2h(h_kf.data(), d.kf_out, (size_t)kf_read * 4)); HIPCHK(pool.d2h(h_mp.data(), d.mp_out, (size_t)mp_read * 4)); HIPCHK(pool.d2h(h_id.data(), d.mp_ids, (size_t)mp_read * 8));
    HIPCHK(pool.fetch_finish());
    if (head.status) { corb_set_error("%s: %d distinct keyframes vote, more than max_connections = %d; nothing was written", who, head.n_voted, M); return CORB_ERR_CAPACITY; }
    if (head.fail) {
        corb_set_error("%s: %d local keyframes and %d local points, more than the caps (kf_cap = %d, mp_cap = %d); nothing was written", who, head.n_kf, head.n_mp, kf_cap, mp_cap);
        return CORB_ERR_CAPACITY;
    }
    if (head.n_kf > 0) memcpy(kf_slots, h_kf.data(), (size_t)head.n_kf * 4);
    if (head.n_mp > 0) { memcpy(mp_slots, h_mp.data(), (size_t)head.n_mp * 4); memcpy(mp_ids, h_id.data(), (size_t)head.n_mp * 8); }
    memcpy(out, &head, sizeof(CorbLocalMap));
    return CORB_OK;
}

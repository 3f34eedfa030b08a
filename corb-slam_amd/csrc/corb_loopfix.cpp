// corb_loopfix.cpp -- a loop event on the device-resident stores (include/corb_accel.h, last section): CorrectLoop's propagation and the map update that follows a
// global bundle adjustment; host side of loopfix_kernels.hip.  corb_loop_correct_store reads back once (the set, its Sim3s, the counts); corb_gba_propagate_store
// twice: the number of held children (it sizes the compact child array) and the counts.
#include "loopfix_internal.h"
#include "covis_host.h"
#include <vector>
#include <algorithm>

static_assert(sizeof(CorbGbaPropagation) == 28 && offsetof(GbaHead, status) == 28, "GbaHead starts with CorbGbaPropagation");

extern "C" int corb_loop_correct_store(CorbCovis* g, int cur_slot, const double* Scw, float scale_factor, int32_t* kf_slots, double* corrected, double* non_corrected,
                                       int cap, int* n, int* n_points_corrected)
{
    const char* who = "corb_loop_correct_store";
    int rc = covis_slot_ok(g, cur_slot, who); if (rc) return rc;
    if (!Scw || !n || cap < 0 || (cap > 0 && (!kf_slots || !corrected || !non_corrected))) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    CovisCall c; rc = c.begin(g, who, true); if (rc) return rc;
    if (g->kf->host[cur_slot].n < 0) { corb_set_error("%s: slot %d is empty", who, cur_slot); return CORB_ERR_ARG; }
    CorbScratch& pool = *c.scratch;
    const int M = g->R.M, K = g->kf->capacity, N = M + 1;
    int* dq = nullptr; double* dscw = nullptr;
    LcDev d{};
    d.cur_slot = cur_slot; d.cap = cap; d.scale_factor = scale_factor;
    HIPCHK(pool.alloc(&dq, (size_t)2 * M + 1)); HIPCHK(pool.upload(&dscw, Scw, 8));
    d.q_slots = dq; d.q_n = dq + 2 * M; d.Scw = dscw;
    HIPCHK(pool.alloc(&d.set, (size_t)N)); HIPCHK(pool.alloc(&d.count, 2)); HIPCHK(pool.alloc(&d.pos, (size_t)K));
    HIPCHK(pool.alloc(&d.sim3, (size_t)N * LOOPFIX_SIM3_DOUBLES)); HIPCHK(pool.alloc(&d.newT, (size_t)N * 16)); HIPCHK(pool.alloc(&d.corrector, (size_t)g->mp->capacity));
    HIPCHK(hipMemsetAsync(d.count, 0, 8, pool.stream));
    HIPCHK(hipMemsetAsync(d.pos, 0x7F, (size_t)K * 4, pool.stream));
    HIPCHK(hipMemsetAsync(d.corrector, 0x7F, (size_t)g->mp->capacity * 4, pool.stream));
    covis_launch_query(g->R, c.S, cur_slot, 0, 0, 0, dq, dq + M, dq + 2 * M, pool.stream);       // mpCurrentKF->GetVectorCovisibleKeyFrames() (:254)
    loopfix_launch_set(c.S, M, d, pool.stream);
    loopfix_launch_correct(c.S, M, d, pool.stream);
    HIPCHK(hipGetLastError());
    int cnt[2] = {0, 0};
    const int n_read = std::min(N, cap);
    std::vector<int32_t> h_set((size_t)n_read); std::vector<double> h_s((size_t)n_read * LOOPFIX_SIM3_DOUBLES);
    HIPCHK(pool.d2h(cnt, d.count, 8));
    HIPCHK(pool.d2h(h_set.data(), d.set, (size_t)n_read * 4)); HIPCHK(pool.d2h(h_s.data(), d.sim3, h_s.size() * 8));
    HIPCHK(pool.fetch_finish());
    *n = cnt[0];
    if (cnt[0] > cap) { corb_set_error("%s: the set holds %d keyframes, cap = %d; nothing was written", who, cnt[0], cap); return CORB_ERR_CAPACITY; }
    for (int i = 0; i < cnt[0]; i++) {
        kf_slots[i] = h_set[i];
        memcpy(corrected + (size_t)i * 8, &h_s[(size_t)i * LOOPFIX_SIM3_DOUBLES], 64); memcpy(non_corrected + (size_t)i * 8, &h_s[(size_t)i * LOOPFIX_SIM3_DOUBLES + 8], 64);
    }
    if (n_points_corrected) *n_points_corrected = cnt[1];
    return CORB_OK;
}

extern "C" int corb_gba_propagate_store(CorbCovis* g, const int32_t* origin_slots, int n_origins, uint64_t loop_kf, int queue_cap, CorbGbaPropagation* out)
{
    const char* who = "corb_gba_propagate_store";
    if (!g || !out || n_origins < 0 || (n_origins > 0 && !origin_slots)) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    const int K = g->kf->capacity;
    const long long qcap = queue_cap > 0 ? (long long)queue_cap : 4ll * K + 64;
    if (qcap >= LOOPFIX_UNSEEN) { corb_set_error("%s: queue_cap %lld is more than a 32-bit queue position holds", who, qcap); return CORB_ERR_ARG; }
    for (int i = 0; i < n_origins; i++) if (origin_slots[i] < 0 || origin_slots[i] >= K) { corb_set_error("%s: origin %d is not a slot of the graph's store", who, i); return CORB_ERR_ARG; }
    int rc = corb_select_device(g->kf->device); if (rc) return rc;
    CovisCall c; rc = c.begin(g, who, true); if (rc) return rc;
    for (int i = 0; i < n_origins; i++) if (g->kf->host[origin_slots[i]].n < 0) { corb_set_error("%s: origin %d (slot %d) is an empty slot", who, i, origin_slots[i]); return CORB_ERR_ARG; }
    if (n_origins > qcap) { corb_set_error("%s: %d origins, queue_cap = %lld; nothing was written", who, n_origins, qcap); return CORB_ERR_CAPACITY; }
    CorbScratch& pool = *c.scratch;
    GbaDev d{};
    d.queue_cap = (int)qcap; d.n_origins = n_origins; d.loop_kf = loop_kf;
    HIPCHK(pool.alloc(&d.Tcw, (size_t)K * 48)); d.GBA = d.Tcw + (size_t)K * 16; d.Bef = d.GBA + (size_t)K * 16;
    HIPCHK(pool.alloc(&d.mark, (size_t)K * 6)); d.cnt = d.mark + K; d.off = d.cnt + K; d.npop = d.off + K; d.winner = d.npop + K; d.first = d.winner + K;
    HIPCHK(pool.alloc(&d.total, 2)); HIPCHK(pool.alloc(&d.head, 1)); HIPCHK(pool.alloc(&d.queue, (size_t)qcap));
    HIPCHK(hipMemsetAsync(d.total, 0, 8, pool.stream));
    HIPCHK(hipMemsetAsync(d.head, 0, sizeof(GbaHead), pool.stream));
    HIPCHK(hipMemsetAsync(d.npop, 0, (size_t)K * 4, pool.stream));
    HIPCHK(hipMemsetAsync(d.winner, 0x7F, (size_t)K * 8, pool.stream));                           // winner and first
    if (n_origins > 0) HIPCHK(pool.h2d(d.queue, origin_slots, (size_t)n_origins * 4));
    loopfix_launch_gather(g->T, g->R.M, c.S, g->bef(), d, pool.stream);
    HIPCHK(hipGetLastError());
    int total = 0;
    HIPCHK(pool.d2h(&total, d.total, 4));
    HIPCHK(pool.fetch_finish());
    HIPCHK(pool.alloc(&d.child, (size_t)std::max(total, 1)));
    loopfix_launch_fill(g->T, g->R.M, c.S, d, pool.stream);
    loopfix_launch_walk(c.S, d, pool.stream);
    loopfix_launch_commit(c.S, g->bef(), d, pool.stream);
    loopfix_launch_points(c.S, g->mp->idt_first, g->mp->idt_n, d, pool.stream);
    HIPCHK(hipGetLastError());
    GbaHead head{};
    HIPCHK(pool.d2h(&head, d.head, sizeof(head)));
    HIPCHK(pool.fetch_finish());
    if (head.status) { corb_set_error("%s: the walk needs more than queue_cap = %lld queue entries (a cyclic child set never ends); nothing was written", who, qcap); return CORB_ERR_CAPACITY; }
    memcpy(out, &head, sizeof(*out));
    return CORB_OK;
}

extern "C" int corb_covis_set_pose_before_gba(CorbCovis* g, int slot, const float* T)
{
    int rc = covis_slot_ok(g, slot, "corb_covis_set_pose_before_gba"); if (rc) return rc;
    if (!T) { corb_set_error("corb_covis_set_pose_before_gba: bad argument"); return CORB_ERR_ARG; }
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    HIPCHK(hipMemcpy(g->bef() + (size_t)slot * 16, T, 64, hipMemcpyHostToDevice));
    return CORB_OK;
}

extern "C" int corb_covis_get_pose_before_gba(CorbCovis* g, int slot, float* T)
{
    int rc = covis_slot_ok(g, slot, "corb_covis_get_pose_before_gba"); if (rc) return rc;
    if (!T) { corb_set_error("corb_covis_get_pose_before_gba: bad argument"); return CORB_ERR_ARG; }
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    HIPCHK(hipMemcpy(T, g->bef() + (size_t)slot * 16, 64, hipMemcpyDeviceToHost));
    return CORB_OK;
}

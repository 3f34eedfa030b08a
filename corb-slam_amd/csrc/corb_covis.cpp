// corb_covis.cpp -- the covisibility graph over the device-resident stores (include/corb_accel.h, last section): host side of covis_kernels.hip.
// The graph keeps one row per slot of the keyframe store (the weight map and the ordered list of C/include/KeyFrame.h:291-293) in device memory.  Every call locks the
// graph and the two stores (keyframes, then map points: the stores' documented order), waits for the stores' pending fills, rebuilds the keyframe id -> slot table
// (the records' headers may have changed since the last call) and runs on the short-call lane of the per-device workspace, whose arena holds the call's scratch.
#include "covis_internal.h"
#include "store_host.h"
#include "corb_workspace.h"
#include <memory>
#include <mutex>
#include <vector>
#include <algorithm>

void corb_set_error(const char* fmt, ...);
int corb_select_device(int device);
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { corb_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); return CORB_ERR_HIP; } } while (0)

struct CorbCovis {
    CorbKfStore* kf = nullptr; CorbMpStore* mp = nullptr;
    CovisRows R{};
    char* mem = nullptr;
    std::mutex mu;
};

extern "C" int corb_covis_create(CorbKfStore* kf, CorbMpStore* mp, int max_connections, CorbCovis** out)
{
    if (!out || !kf || !mp || max_connections > COVIS_MAX_CONNECTIONS) { corb_set_error("corb_covis_create: bad argument (max_connections <= %d)", COVIS_MAX_CONNECTIONS); return CORB_ERR_ARG; }
    *out = nullptr;
    if (kf->device != mp->device) { corb_set_error("corb_covis_create: the stores live on different devices"); return CORB_ERR_ARG; }
    int rc = corb_select_device(kf->device); if (rc) return rc;
    const int M = max_connections > 0 ? max_connections : COVIS_DEFAULT_CONNECTIONS;
    const size_t cells = (size_t)kf->capacity * M, heads = ((size_t)kf->capacity * 4 + 255) & ~(size_t)255;
    const size_t bytes = cells * 24 + 2 * heads;
    CorbCovis* g = new CorbCovis();
    g->kf = kf; g->mp = mp;
    if (hipMalloc((void**)&g->mem, bytes) != hipSuccess) { corb_set_error("corb_covis_create: %d rows x %d connections: allocation failed", kf->capacity, M); delete g; return CORB_ERR_HIP; }
    g->R.M = M;
    g->R.all_id = reinterpret_cast<unsigned long long*>(g->mem); g->R.ord_id = g->R.all_id + cells;
    g->R.all_w = reinterpret_cast<int*>(g->R.ord_id + cells); g->R.ord_w = g->R.all_w + cells;
    g->R.n_all = reinterpret_cast<int*>(g->mem + cells * 24); g->R.n_ord = reinterpret_cast<int*>(g->mem + cells * 24 + heads);
    if (hipMemset(g->mem, 0, bytes) != hipSuccess) { corb_set_error("corb_covis_create: hipMemset failed"); (void)hipFree(g->mem); delete g; return CORB_ERR_HIP; }
    *out = g;
    return CORB_OK;
}
extern "C" void corb_covis_destroy(CorbCovis* g)
{
    if (!g) return;
    (void)hipSetDevice(g->kf->device);
    if (g->mem) (void)hipFree(g->mem);
    delete g;
}

namespace {
// one call's hold on the graph and the stores, and the stores as the kernels read them
struct CovisCall {
    std::unique_lock<std::mutex> lk_g, lk_kf, lk_mp;
    std::unique_ptr<CorbScratch> scratch;            // taken after the stores' locks, as every store call does
    CovisStores S{};
    int begin(CorbCovis* g, const char* who, bool need_points)
    {
        CorbKfStore* kf = g->kf; CorbMpStore* mp = g->mp;
        lk_g = std::unique_lock<std::mutex>(g->mu); lk_kf = std::unique_lock<std::mutex>(kf->mu); lk_mp = std::unique_lock<std::mutex>(mp->mu);
        scratch.reset(new CorbScratch(0));
        CorbScratch& pool = *scratch;
        if (!pool.stream) { corb_set_error("%s: no workspace stream", who); return CORB_ERR_HIP; }
        if (need_points && (!mp->idt.keys || !mp->idt_valid)) { corb_set_error("%s: the map-point store has no current id index (corb_mp_store_build_index after the last put / push)", who); return CORB_ERR_ARG; }
        HIPCHK(hipStreamSynchronize(kf->stream)); HIPCHK(hipStreamSynchronize(mp->stream));
        S.kf_base = kf->base; S.kf_bytes = kf->L.bytes; S.F = kf->F; S.kf_capacity = kf->capacity;
        S.mp_base = mp->base; S.mp_bytes = mp->L.bytes; S.O = mp->O; S.mp_capacity = mp->capacity; S.mpid = mp->idt;
        unsigned int cap = 64; while (cap < 2u * (unsigned int)kf->capacity) cap <<= 1;
        HIPCHK(pool.alloc(&S.kfid.keys, (size_t)cap)); HIPCHK(pool.alloc(&S.kfid.vals, (size_t)cap)); S.kfid.mask = cap - 1;
        HIPCHK(hipMemsetAsync(S.kfid.keys, 0xFF, (size_t)cap * 8, pool.stream));
        HIPCHK(hipMemsetAsync(S.kfid.vals, 0x7F, (size_t)cap * 4, pool.stream));              // (corb_idtab_insert_min)
        corb_launch_kf_index(S.kf_base, S.kf_bytes, 0, S.kf_capacity, S.kfid, pool.stream);        // "in the cache" (Cache::KeyFrameInCache) means: found in this table
        HIPCHK(hipGetLastError());
        return CORB_OK;
    }
};
int slot_ok(CorbCovis* g, int slot, const char* who)
{
    if (!g || slot < 0 || slot >= g->kf->capacity) { corb_set_error("%s: bad graph / slot", who); return CORB_ERR_ARG; }
    return CORB_OK;
}
}

extern "C" int corb_covis_update(CorbCovis* g, const int32_t* slots, int n, int th, uint64_t* first_parent)
{
    if (!g || n < 0 || (n > 0 && !slots)) { corb_set_error("corb_covis_update: bad argument"); return CORB_ERR_ARG; }
    if (n == 0) return CORB_OK;
    std::vector<char> seen((size_t)g->kf->capacity, 0);
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= g->kf->capacity || seen[slots[i]]) { corb_set_error("corb_covis_update: slot %d of the batch is out of range or listed twice", i); return CORB_ERR_ARG; }
        seen[slots[i]] = 1;
    }
    int rc = corb_select_device(g->kf->device); if (rc) return rc;
    CovisCall c; rc = c.begin(g, "corb_covis_update", true); if (rc) return rc;
    CorbScratch& pool = *c.scratch; const int M = g->R.M; const size_t cells = (size_t)n * M;
    CovisStage st; int *dslots = nullptr, *dover = nullptr;
    HIPCHK(pool.alloc(&st.all_id, cells)); HIPCHK(pool.alloc(&st.ord_id, cells)); HIPCHK(pool.alloc(&st.all_w, cells)); HIPCHK(pool.alloc(&st.ord_w, cells));
    HIPCHK(pool.alloc(&st.ord_slot, cells)); HIPCHK(pool.alloc(&st.head, (size_t)n)); HIPCHK(pool.alloc(&dover, 1));
    HIPCHK(pool.upload(&dslots, slots, (size_t)n));
    HIPCHK(hipMemsetAsync(dover, 0, 4, pool.stream));
    // count first: the counters depend on the records alone, so the whole batch is one launch
    covis_launch_count(c.S, dslots, n, th, M, st, pool.stream);
    HIPCHK(hipGetLastError());
    std::vector<CovisStageHead> head((size_t)n);
    HIPCHK(pool.d2h(head.data(), st.head, (size_t)n * sizeof(CovisStageHead)));
    HIPCHK(pool.fetch_finish());
    for (int i = 0; i < n; i++) if (head[i].status) {
        corb_set_error("corb_covis_update: keyframe %d of the batch (slot %d) is connected to more than max_connections = %d keyframes; the graph is unchanged", i, slots[i], M);
        return CORB_ERR_CAPACITY;
    }
    // commit after: the members in list order, a launch each, nothing between them but the stream's order
    for (int i = 0; i < n; i++) if (head[i].n_all > 0) covis_launch_apply(g->R, c.S, st, i, slots[i], head[i].n_ord, dover, pool.stream);
    HIPCHK(hipGetLastError());
    int over = 0;
    HIPCHK(pool.d2h(&over, dover, 4));
    HIPCHK(pool.fetch_finish());
    if (first_parent) for (int i = 0; i < n; i++) first_parent[i] = head[i].first;
    if (over) { corb_set_error("corb_covis_update: AddConnection found the row of a neighbour full (max_connections = %d); that connection is missing", M); return CORB_ERR_OVERFLOW; }
    return CORB_OK;
}

extern "C" int corb_covis_erase(CorbCovis* g, int slot)
{
    int rc = slot_ok(g, slot, "corb_covis_erase"); if (rc) return rc;
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    CovisCall c; rc = c.begin(g, "corb_covis_erase", false); if (rc) return rc;
    covis_launch_erase(g->R, c.S, slot, c.scratch->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(g->R.n_all + slot, 0, 4, c.scratch->stream));                           // mConnectedKeyFrameWeights.clear(); mvpOrderedConnectedKeyFrames.clear() (:604-605)
    HIPCHK(hipMemsetAsync(g->R.n_ord + slot, 0, 4, c.scratch->stream));
    HIPCHK(hipStreamSynchronize(c.scratch->stream));
    return CORB_OK;
}

extern "C" int corb_covis_get(CorbCovis* g, int slot, uint64_t* all_id, int32_t* all_w, int* n_all, uint64_t* ord_id, int32_t* ord_w, int* n_ord, int cap)
{
    int rc = slot_ok(g, slot, "corb_covis_get"); if (rc) return rc;
    if (!n_all || !n_ord || cap < 0) { corb_set_error("corb_covis_get: bad argument"); return CORB_ERR_ARG; }
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    int na = 0, no = 0;
    HIPCHK(hipMemcpy(&na, g->R.n_all + slot, 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(&no, g->R.n_ord + slot, 4, hipMemcpyDeviceToHost));
    *n_all = na; *n_ord = no;
    if (na > cap || no > cap) { corb_set_error("corb_covis_get: the row holds %d / %d entries, cap = %d", na, no, cap); return CORB_ERR_CAPACITY; }
    const size_t row = (size_t)slot * g->R.M;
    if (all_id && na) HIPCHK(hipMemcpy(all_id, g->R.all_id + row, (size_t)na * 8, hipMemcpyDeviceToHost));
    if (all_w && na) HIPCHK(hipMemcpy(all_w, g->R.all_w + row, (size_t)na * 4, hipMemcpyDeviceToHost));
    if (ord_id && no) HIPCHK(hipMemcpy(ord_id, g->R.ord_id + row, (size_t)no * 8, hipMemcpyDeviceToHost));
    if (ord_w && no) HIPCHK(hipMemcpy(ord_w, g->R.ord_w + row, (size_t)no * 4, hipMemcpyDeviceToHost));
    return CORB_OK;
}

extern "C" int corb_covis_query(CorbCovis* g, int slot, int N, int min_weight, int32_t* out_slots, int32_t* out_w, int cap, int* n)
{
    int rc = slot_ok(g, slot, "corb_covis_query"); if (rc) return rc;
    if (!n || cap < 0 || (N > 0 && min_weight > 0)) { corb_set_error("corb_covis_query: bad argument (N and min_weight exclude each other)"); return CORB_ERR_ARG; }
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    CovisCall c; rc = c.begin(g, "corb_covis_query", false); if (rc) return rc;
    const int M = g->R.M;
    int* d = nullptr;                                                                        // [M] slots, [M] weights, the count
    HIPCHK(c.scratch->alloc(&d, (size_t)2 * M + 1));
    covis_launch_query(g->R, c.S, slot, N, min_weight, min_weight > 0 ? 1 : 0, d, d + M, d + 2 * M, c.scratch->stream);
    HIPCHK(hipGetLastError());
    std::vector<int> h((size_t)2 * M + 1);
    HIPCHK(c.scratch->d2h(h.data(), d, h.size() * 4));
    HIPCHK(c.scratch->fetch_finish());
    *n = h[2 * M];
    if (*n > cap) { corb_set_error("corb_covis_query: %d keyframes, cap = %d", *n, cap); return CORB_ERR_CAPACITY; }
    for (int i = 0; i < *n; i++) { if (out_slots) out_slots[i] = h[i]; if (out_w) out_w[i] = h[M + i]; }
    return CORB_OK;
}

extern "C" int corb_covis_weight(CorbCovis* g, int slot_a, int slot_b, int* w)
{
    int rc = slot_ok(g, slot_a, "corb_covis_weight"); if (rc) return rc;
    rc = slot_ok(g, slot_b, "corb_covis_weight"); if (rc) return rc;
    if (!w) { corb_set_error("corb_covis_weight: bad argument"); return CORB_ERR_ARG; }
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    CovisCall c; rc = c.begin(g, "corb_covis_weight", false); if (rc) return rc;
    int* d = nullptr;
    HIPCHK(c.scratch->alloc(&d, 1));
    covis_launch_weight(g->R, c.S, slot_a, slot_b, d, c.scratch->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(c.scratch->d2h(w, d, 4));
    HIPCHK(c.scratch->fetch_finish());
    return CORB_OK;
}

extern "C" int corb_covis_keyframe_culling(CorbCovis* g, int cur_slot, int monocular, float th_depth, int32_t* kf_slots, int32_t* n_mps, int32_t* n_redundant, uint8_t* cull, int cap, int* n)
{
    int rc = slot_ok(g, cur_slot, "corb_covis_keyframe_culling"); if (rc) return rc;
    if (!n || cap < 0) { corb_set_error("corb_covis_keyframe_culling: bad argument"); return CORB_ERR_ARG; }
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    CovisCall c; rc = c.begin(g, "corb_covis_keyframe_culling", true); if (rc) return rc;
    const int M = g->R.M;
    int* d = nullptr; unsigned char* dc = nullptr;                                           // [M] slots, [M] weights, the count, [M] nMPs, [M] nRedundantObservations
    HIPCHK(c.scratch->alloc(&d, (size_t)4 * M + 1)); HIPCHK(c.scratch->alloc(&dc, (size_t)M));
    covis_launch_query(g->R, c.S, cur_slot, 0, 0, 0, d, d + M, d + 2 * M, c.scratch->stream);     // vpLocalKeyFrames = mpCurrentKeyFrame->GetVectorCovisibleKeyFrames()
    covis_launch_culling(c.S, d, d + 2 * M, M, monocular ? 1 : 0, th_depth, d + 2 * M + 1, d + 3 * M + 1, dc, c.scratch->stream);
    HIPCHK(hipGetLastError());
    std::vector<int> h((size_t)4 * M + 1); std::vector<unsigned char> hc((size_t)M);
    HIPCHK(c.scratch->d2h(h.data(), d, h.size() * 4)); HIPCHK(c.scratch->d2h(hc.data(), dc, (size_t)M));
    HIPCHK(c.scratch->fetch_finish());
    *n = h[2 * M];
    if (*n > cap) { corb_set_error("corb_covis_keyframe_culling: %d covisible keyframes, cap = %d", *n, cap); return CORB_ERR_CAPACITY; }
    for (int i = 0; i < *n; i++) {
        if (kf_slots) kf_slots[i] = h[i];
        if (n_mps) n_mps[i] = h[2 * M + 1 + i];
        if (n_redundant) n_redundant[i] = h[3 * M + 1 + i];
        if (cull) cull[i] = hc[i];
    }
    return CORB_OK;
}

extern "C" int corb_covis_local_window(CorbCovis* g, int slot, int32_t* kf_slots, int kf_cap, int* n_local, int* n_kf, int32_t* mp_slots, int mp_cap, int* n_mp)
{
    int rc = slot_ok(g, slot, "corb_covis_local_window"); if (rc) return rc;
    if (!n_local || !n_kf || !n_mp || kf_cap < 0 || mp_cap < 0 || (kf_cap > 0 && !kf_slots) || (mp_cap > 0 && !mp_slots)) { corb_set_error("corb_covis_local_window: bad argument"); return CORB_ERR_ARG; }
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    CovisCall c; rc = c.begin(g, "corb_covis_local_window", true); if (rc) return rc;
    CorbScratch& pool = *c.scratch;
    CovisWindow w{};
    w.kf_cap = kf_cap; w.mp_cap = mp_cap;
    w.local_bound = std::max(1, std::min(std::min(g->R.M + 1, kf_cap), g->kf->capacity));
    const long long n1 = (long long)w.local_bound * g->kf->F;
    w.mp_bound = (int)std::min<long long>(std::min<long long>(mp_cap, n1), g->mp->capacity);
    const long long n2 = (long long)w.mp_bound * g->mp->O, nc = std::max(n1, n2);
    if (nc >= COVIS_UNSEEN) { corb_set_error("corb_covis_local_window: the caps allow %lld candidates, more than a 32-bit position holds", nc); return CORB_ERR_ARG; }
    HIPCHK(pool.alloc(&w.kf_out, (size_t)kf_cap)); HIPCHK(pool.alloc(&w.mp_out, (size_t)mp_cap)); HIPCHK(pool.alloc(&w.counts, 4));
    HIPCHK(pool.alloc(&w.first_kf, (size_t)g->kf->capacity)); HIPCHK(pool.alloc(&w.first_mp, (size_t)g->mp->capacity));
    HIPCHK(pool.alloc(&w.flag, (size_t)nc + 1)); HIPCHK(pool.alloc(&w.pos, (size_t)nc + 1)); HIPCHK(pool.alloc(&w.scan_scratch, corb_scan_scratch_ints((size_t)nc)));
    HIPCHK(hipMemsetAsync(w.counts, 0, 16, pool.stream));
    HIPCHK(hipMemsetAsync(w.first_kf, 0x7F, (size_t)g->kf->capacity * 4, pool.stream));
    HIPCHK(hipMemsetAsync(w.first_mp, 0x7F, (size_t)g->mp->capacity * 4, pool.stream));
    covis_launch_window(g->R, c.S, slot, w, pool.stream);
    HIPCHK(hipGetLastError());
    int cnt[4] = {0, 0, 0, 0};
    HIPCHK(pool.d2h(cnt, w.counts, 16));
    HIPCHK(pool.fetch_finish());
    if (cnt[0] > kf_cap || cnt[1] > mp_cap || (long long)cnt[0] + cnt[2] > kf_cap) {
        corb_set_error("corb_covis_local_window: the window is larger than the caps (kf_cap = %d, mp_cap = %d); nothing was written", kf_cap, mp_cap);
        return CORB_ERR_CAPACITY;
    }
    if (cnt[0] + cnt[2] > 0) HIPCHK(hipMemcpyAsync(kf_slots, w.kf_out, (size_t)(cnt[0] + cnt[2]) * 4, hipMemcpyDeviceToHost, pool.stream));
    if (cnt[1] > 0) HIPCHK(hipMemcpyAsync(mp_slots, w.mp_out, (size_t)cnt[1] * 4, hipMemcpyDeviceToHost, pool.stream));
    HIPCHK(hipStreamSynchronize(pool.stream));
    *n_local = cnt[0]; *n_kf = cnt[0] + cnt[2]; *n_mp = cnt[1];
    return CORB_OK;
}

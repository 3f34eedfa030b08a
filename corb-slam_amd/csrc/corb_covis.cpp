// corb_covis.cpp -- the covisibility graph over the device-resident stores (include/corb_accel.h, last section): host side of covis_kernels.hip.
// The graph keeps one row per slot of the keyframe store (the weight map and the ordered list of C/include/KeyFrame.h:291-293) in device memory.  Every call locks the
// graph and the two stores (keyframes, then map points: the stores' documented order), waits for the stores' pending fills, rebuilds the keyframe id -> slot table
// (the records' headers may have changed since the last call) and runs on the short-call lane of the per-device workspace, whose arena holds the call's scratch.
#include "covis_host.h"
#include <vector>
#include <algorithm>

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
    g->kf = kf; g->mp = mp; g->device = kf->device;
    if (g->mem.room(bytes) != hipSuccess) { corb_set_error("corb_covis_create: %d rows x %d connections: allocation failed", kf->capacity, M); delete g; return CORB_ERR_HIP; }
    char* const mem = g->mem.as<char>();
    g->R.M = M;
    g->R.all_id = reinterpret_cast<unsigned long long*>(mem); g->R.ord_id = g->R.all_id + cells;
    g->R.all_w = reinterpret_cast<int*>(g->R.ord_id + cells); g->R.ord_w = g->R.all_w + cells;
    g->R.n_all = reinterpret_cast<int*>(mem + cells * 24); g->R.n_ord = reinterpret_cast<int*>(mem + cells * 24 + heads);
    if (hipMemset(mem, 0, bytes) != hipSuccess) { corb_set_error("corb_covis_create: hipMemset failed"); delete g; return CORB_ERR_HIP; }
    // the spanning tree beside the rows: parent ids, child sets, then the two per-slot ints
    const size_t tree_bytes = (((size_t)kf->capacity * 8 + 255) & ~(size_t)255) + cells * 8 + 2 * heads;
    if (g->tree_mem.room(tree_bytes) != hipSuccess) { corb_set_error("corb_covis_create: %d child sets x %d ids: allocation failed", kf->capacity, M); delete g; return CORB_ERR_HIP; }
    char* const tree_mem = g->tree_mem.as<char>();
    g->T.parent = reinterpret_cast<unsigned long long*>(tree_mem); g->T.child_id = reinterpret_cast<unsigned long long*>(tree_mem + (((size_t)kf->capacity * 8 + 255) & ~(size_t)255));
    g->T.first = reinterpret_cast<int*>(g->T.child_id + cells); g->T.n_child = reinterpret_cast<int*>(reinterpret_cast<char*>(g->T.first) + heads);
    covis_launch_tree_init(g->T, kf->capacity, nullptr);                                          // none / first connection / no children
    // (a wait for the stream of the launch alone: the device's other streams, other clients' stores among them, are not waited for)
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) { corb_set_error("corb_covis_create: the tree's initialisation failed"); delete g; return CORB_ERR_HIP; }
    // mTcwBefGBA beside the tree (the record's header has no room for it).  The reference leaves the matrix uninitialised (KeyFrame.cc:62); here it starts as the identity
    std::vector<float> eye((size_t)kf->capacity * 16, 0.f);
    for (size_t i = 0; i < (size_t)kf->capacity; i++) eye[i * 16] = eye[i * 16 + 5] = eye[i * 16 + 10] = eye[i * 16 + 15] = 1.f;
    if (g->bef_mem.room(eye.size() * 4 + 256) != hipSuccess || hipMemcpy(g->bef(), eye.data(), eye.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        corb_set_error("corb_covis_create: %d poses before the global BA: allocation failed", kf->capacity); delete g; return CORB_ERR_HIP;
    }
    if (essgraph_loop_sets_create(g) != CORB_OK) { delete g; return CORB_ERR_HIP; }
    *out = g;
    return CORB_OK;
}
extern "C" void corb_covis_destroy(CorbCovis* g) { handle_destroy(g); }

namespace {
int slot_ok(CorbCovis* g, int slot, const char* who) { return covis_slot_ok(g, slot, who); }
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
    for (int i = 0; i < n; i++) if (head[i].n_all > 0) covis_launch_apply(g->R, g->T, c.S, st, i, slots[i], head[i].n_ord, dover, pool.stream);
    HIPCHK(hipGetLastError());
    int over = 0;
    HIPCHK(pool.d2h(&over, dover, 4));
    HIPCHK(pool.fetch_finish());
    if (first_parent) for (int i = 0; i < n; i++) first_parent[i] = head[i].first;
    if (over) { corb_set_error("corb_covis_update: AddConnection / AddChild found the row or the child set of a neighbour full (max_connections = %d); that entry is missing", M); return CORB_ERR_OVERFLOW; }
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

// ---- the spanning tree ----
extern "C" int corb_covis_set_tree(CorbCovis* g, int slot, uint64_t parent_id, int first_connection, const uint64_t* children, int n)
{
    int rc = slot_ok(g, slot, "corb_covis_set_tree"); if (rc) return rc;
    if (n < 0 || (n > 0 && !children)) { corb_set_error("corb_covis_set_tree: bad argument"); return CORB_ERR_ARG; }
    if (n > g->R.M) { corb_set_error("corb_covis_set_tree: %d children, max_connections = %d", n, g->R.M); return CORB_ERR_OVERFLOW; }
    std::vector<unsigned long long> ids(children, children + n);
    std::sort(ids.begin(), ids.end());
    if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) { corb_set_error("corb_covis_set_tree: a child is listed twice"); return CORB_ERR_ARG; }
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    CorbScratch pool(0);                                                                        // the short-call lane: staged copies on its stream, one synchronisation
    if (!pool.stream) { corb_set_error("corb_covis_set_tree: no workspace stream"); return CORB_ERR_HIP; }
    const unsigned long long p = parent_id; const int f = first_connection ? 1 : 0;
    HIPCHK(pool.h2d(g->T.parent + slot, &p, 8)); HIPCHK(pool.h2d(g->T.first + slot, &f, 4)); HIPCHK(pool.h2d(g->T.n_child + slot, &n, 4));
    if (n) HIPCHK(pool.h2d(g->T.child_id + (size_t)slot * g->R.M, ids.data(), (size_t)n * 8));
    HIPCHK(hipStreamSynchronize(pool.stream));
    return CORB_OK;
}

extern "C" int corb_covis_get_tree(CorbCovis* g, int slot, uint64_t* parent_id, int* first_connection, uint64_t* children, int cap, int* n)
{
    int rc = slot_ok(g, slot, "corb_covis_get_tree"); if (rc) return rc;
    if (!n || cap < 0) { corb_set_error("corb_covis_get_tree: bad argument"); return CORB_ERR_ARG; }
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    CorbScratch pool(0);
    if (!pool.stream) { corb_set_error("corb_covis_get_tree: no workspace stream"); return CORB_ERR_HIP; }
    unsigned long long p = 0; int f = 0, nc = 0;
    std::vector<unsigned long long> ch((size_t)g->R.M);                                         // the whole set's room (at most 8 KiB): the count comes back with it
    HIPCHK(pool.d2h(&p, g->T.parent + slot, 8)); HIPCHK(pool.d2h(&f, g->T.first + slot, 4)); HIPCHK(pool.d2h(&nc, g->T.n_child + slot, 4));
    if (children) HIPCHK(pool.d2h(ch.data(), g->T.child_id + (size_t)slot * g->R.M, ch.size() * 8));
    HIPCHK(pool.fetch_finish());
    if (parent_id) *parent_id = p;
    if (first_connection) *first_connection = f;
    nc = std::min(std::max(nc, 0), g->R.M);
    *n = nc;
    if (nc > cap) { corb_set_error("corb_covis_get_tree: the set holds %d children, cap = %d", nc, cap); return CORB_ERR_CAPACITY; }
    if (children && nc) memcpy(children, ch.data(), (size_t)nc * 8);
    return CORB_OK;
}

namespace {
int tree_op(CorbCovis* g, int op, int slot, int other, const char* who)
{
    int rc = slot_ok(g, slot, who); if (rc) return rc;
    rc = slot_ok(g, other, who); if (rc) return rc;
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    CovisCall c; rc = c.begin(g, who, false); if (rc) return rc;
    int* dover = nullptr;
    HIPCHK(c.scratch->alloc(&dover, 1));
    HIPCHK(hipMemsetAsync(dover, 0, 4, c.scratch->stream));
    covis_launch_tree_op(g->R, g->T, c.S, op, slot, other, dover, c.scratch->stream);
    HIPCHK(hipGetLastError());
    int over = 0;
    HIPCHK(c.scratch->d2h(&over, dover, 4));
    HIPCHK(c.scratch->fetch_finish());
    if (over) { corb_set_error("%s: the child set is full (max_connections = %d); the child is missing", who, g->R.M); return CORB_ERR_OVERFLOW; }
    return CORB_OK;
}
}
extern "C" int corb_covis_add_child(CorbCovis* g, int slot, int child_slot) { return tree_op(g, 0, slot, child_slot, "corb_covis_add_child"); }
extern "C" int corb_covis_erase_child(CorbCovis* g, int slot, int child_slot) { return tree_op(g, 1, slot, child_slot, "corb_covis_erase_child"); }
extern "C" int corb_covis_change_parent(CorbCovis* g, int slot, int other_slot) { return tree_op(g, 2, slot, other_slot, "corb_covis_change_parent"); }

extern "C" int corb_covis_reparent_children(CorbCovis* g, int slot, int* n_changed, int* reference_sets_bad)
{
    int rc = slot_ok(g, slot, "corb_covis_reparent_children"); if (rc) return rc;
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    CovisCall c; rc = c.begin(g, "corb_covis_reparent_children", false); if (rc) return rc;
    int* d = nullptr;
    HIPCHK(c.scratch->alloc(&d, 4));
    HIPCHK(hipMemsetAsync(d, 0, 16, c.scratch->stream));
    covis_launch_reparent(g->R, g->T, c.S, slot, d, c.scratch->stream);
    HIPCHK(hipGetLastError());
    int h[4] = {0, 0, 0, 0};
    HIPCHK(c.scratch->d2h(h, d, 16));
    HIPCHK(c.scratch->fetch_finish());
    if (n_changed) *n_changed = h[0];
    if (reference_sets_bad) *reference_sets_bad = h[1];
    if (h[2]) { corb_set_error("corb_covis_reparent_children: the child set of a new parent is full (max_connections = %d); that child is missing from it", g->R.M); return CORB_ERR_OVERFLOW; }
    return CORB_OK;
}

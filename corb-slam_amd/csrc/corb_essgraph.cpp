// corb_essgraph.cpp -- Optimizer::OptimizeEssentialGraph on device-resident records (include/corb_essential_graph.h): host side of essgraph_kernels.hip.  The
// loop-edge sets live in the graph beside the rows and the tree.  A plan reads back once (the counts) before its fill; corb_essential_graph_store reads back the
// counts, then (vi, vj, fixed) for the accumulation lists of corb_graph.cpp, the solver's scalars, and the commit's counts.
#include "essgraph_internal.h"
#include "covis_host.h"
#include "dense_chol.h"
#include <vector>
#include <algorithm>

namespace {
EssLoopSets loop_sets(CorbCovis* g)
{
    EssLoopSets L;
    L.id = g->loop_mem.as<unsigned long long>();
    L.n = reinterpret_cast<int*>(L.id + (size_t)g->kf->capacity * ESS_LOOP_CAP);
    return L;
}
}

int essgraph_loop_sets_create(CorbCovis* g)
{
    const size_t bytes = (size_t)g->kf->capacity * (ESS_LOOP_CAP * 8 + 4) + 256;
    if (g->loop_mem.room(bytes) != hipSuccess || hipMemset(g->loop_mem.as<char>(), 0, bytes) != hipSuccess) {
        corb_set_error("corb_covis_create: %d loop-edge sets: allocation failed", g->kf->capacity); return CORB_ERR_HIP;
    }
    return CORB_OK;
}

namespace {
int loop_op(CorbCovis* g, int op, int slot, int other, const char* who)
{
    int rc = covis_slot_ok(g, slot, who); if (rc) return rc;
    rc = covis_slot_ok(g, other, who); if (rc) return rc;
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    CovisCall c; rc = c.begin(g, who, false); if (rc) return rc;
    int* dst = nullptr;
    HIPCHK(c.scratch->alloc(&dst, 1));
    ess_launch_loop_op(loop_sets(g), c.S, op, slot, other, dst, c.scratch->stream);
    HIPCHK(hipGetLastError());
    int status = 0;
    HIPCHK(c.scratch->d2h(&status, dst, 4));
    HIPCHK(c.scratch->fetch_finish());
    if (status == 1) { corb_set_error("%s: the set of slot %d holds %d ids already; nothing was written", who, slot, ESS_LOOP_CAP); return CORB_ERR_CAPACITY; }
    if (status == 2) { corb_set_error("%s: slot %d holds no keyframe", who, other); return CORB_ERR_ARG; }
    return CORB_OK;
}
}

namespace {
int loop_get(CorbCovis* g, int slot, uint64_t* ids, int cap, int* n)
{
    int rc = covis_slot_ok(g, slot, "corb_covis_get_loop_edges"); if (rc) return rc;
    if (!n || cap < 0 || (cap > 0 && !ids)) { corb_set_error("corb_covis_get_loop_edges: bad argument"); return CORB_ERR_ARG; }
    rc = corb_select_device(g->kf->device); if (rc) return rc;
    std::lock_guard<std::mutex> lk(g->mu);
    CorbScratch pool(0);
    if (!pool.stream) { corb_set_error("corb_covis_get_loop_edges: no workspace stream"); return CORB_ERR_HIP; }
    const EssLoopSets L = loop_sets(g);
    unsigned long long set[ESS_LOOP_CAP]; int k = 0;
    HIPCHK(pool.d2h(&k, L.n + slot, 4)); HIPCHK(pool.d2h(set, L.id + (size_t)slot * ESS_LOOP_CAP, sizeof(set)));
    HIPCHK(pool.fetch_finish());
    k = std::min(std::max(k, 0), ESS_LOOP_CAP);
    *n = k;
    if (k > cap) { corb_set_error("corb_covis_get_loop_edges: the set holds %d ids, cap = %d", k, cap); return CORB_ERR_CAPACITY; }
    for (int i = 0; i < k; i++) ids[i] = set[i];
    return CORB_OK;
}
}
extern "C" int corb_covis_add_loop_edge(CorbCovis* g, int slot, int other_slot) { return loop_op(g, 0, slot, other_slot, "corb_covis_add_loop_edge"); }
extern "C" int corb_covis_clear_loop_edges(CorbCovis* g, int slot) { return loop_op(g, 1, slot, slot, "corb_covis_clear_loop_edges"); }
extern "C" int corb_covis_get_loop_edges(CorbCovis* g, int slot, uint64_t* ids, int cap, int* n) { return loop_get(g, slot, ids, cap, n); }

namespace {
// one plan on the device: the call's hold, the argument block, the counts.  run() leaves the vertices and the edge counts in scratch; fill() the edges
struct EssPlan {
    CovisCall call;
    EssPlanDev d{};
    int head[ESS_H_INTS] = {};
    int K = 0, E = 0;
    int run(CorbCovis* g, const CorbEssentialGraphInput* in, const char* who)
    {
        if (!g || !in || in->n_corr < 0 || in->n_lc < 0 || (in->n_corr > 0 && (!in->corr_slots || !in->corrected || !in->non_corrected)) ||
            (in->n_lc > 0 && (!in->lc_kf || !in->lc_offset))) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
        const int cap = g->kf->capacity;
        int rc = covis_slot_ok(g, in->loop_slot, who); if (rc) return rc;
        rc = covis_slot_ok(g, in->cur_slot, who); if (rc) return rc;
        std::vector<int> cpos((size_t)cap, -1), lci, lcj;
        for (int i = 0; i < in->n_corr; i++) {
            const int s = in->corr_slots[i];
            if (s < 0 || s >= cap || cpos[s] >= 0) { corb_set_error("%s: corr_slots[%d] is out of range or listed twice", who, i); return CORB_ERR_ARG; }
            cpos[s] = i;
        }
        {
            std::vector<char> seen_key((size_t)cap, 0); std::vector<int> seen((size_t)cap, -1);
            if (in->n_lc > 0 && in->lc_offset[0] != 0) { corb_set_error("%s: lc_offset[0] != 0", who); return CORB_ERR_ARG; }
            for (int k = 0; k < in->n_lc; k++) {
                const int i = in->lc_kf[k], b = in->lc_offset[k], e = in->lc_offset[k + 1];
                if (i < 0 || i >= cap || seen_key[i] || e < b || (e > b && !in->lc_slots)) { corb_set_error("%s: loop connection %d: key out of range or listed twice, or offsets descend", who, k); return CORB_ERR_ARG; }
                seen_key[i] = 1;
                for (int t = b; t < e; t++) {
                    const int j = in->lc_slots[t];
                    if (j < 0 || j >= cap || seen[j] == k) { corb_set_error("%s: loop connection %d: member %d is out of range or listed twice", who, k, t - b); return CORB_ERR_ARG; }
                    seen[j] = k; lci.push_back(i); lcj.push_back(j);
                }
            }
        }
        rc = corb_select_device(g->kf->device); if (rc) return rc;
        rc = call.begin(g, who, true, nullptr, 1); if (rc) return rc;                               // lane 1: the long-optimisation lane
        CorbScratch& pool = *call.scratch;
        const int P = (int)lci.size(), nc = in->n_corr;
        d.loop_slot = in->loop_slot; d.cur_slot = in->cur_slot; d.min_weight = in->min_weight; d.n_pairs = P;
        d.loops = loop_sets(g);
        int *dcpos = nullptr, *dlci = nullptr, *dlcj = nullptr; double *dcorr = nullptr, *dncorr = nullptr;
        HIPCHK(pool.upload(&dcpos, cpos)); HIPCHK(pool.upload(&dlci, lci)); HIPCHK(pool.upload(&dlcj, lcj));
        HIPCHK(pool.upload(&dcorr, in->corrected, (size_t)nc * 8)); HIPCHK(pool.upload(&dncorr, in->non_corrected, (size_t)nc * 8));
        d.cpos = dcpos; d.lc_i = dlci; d.lc_j = dlcj; d.corr = dcorr; d.ncorr = dncorr;
        HIPCHK(pool.alloc(&d.key, (size_t)cap)); HIPCHK(pool.alloc(&d.bad, (size_t)cap));
        HIPCHK(pool.alloc(&d.hrank, (size_t)cap * 4)); d.vrank = d.hrank + cap; d.hslot = d.vrank + cap; d.vslot = d.hslot + cap;
        HIPCHK(pool.alloc(&d.S, (size_t)cap * 8)); HIPCHK(pool.alloc(&d.snc, (size_t)cap * 8)); HIPCHK(pool.alloc(&d.fixed, (size_t)cap));
        HIPCHK(pool.alloc(&d.head, ESS_H_INTS)); HIPCHK(pool.alloc(&d.lc_flag, (size_t)std::max(P, 1) * 2)); d.lc_pos = d.lc_flag + std::max(P, 1);
        HIPCHK(pool.alloc(&d.ins, (size_t)std::max(P, 1) * 2)); HIPCHK(pool.alloc(&d.n_ins, 1));
        HIPCHK(pool.alloc(&d.cnt, (size_t)cap * 2 + 2)); d.off = d.cnt + cap + 1;
        HIPCHK(pool.alloc(&d.scan_scratch, corb_scan_scratch_ints((size_t)cap)));
        HIPCHK(hipMemsetAsync(d.head, 0, sizeof(int) * ESS_H_INTS, pool.stream));
        HIPCHK(hipMemsetAsync(d.cnt, 0, sizeof(int) * ((size_t)cap * 2 + 2), pool.stream));
        ess_launch_count(g->R, g->T, call.S, d, pool.stream);
        HIPCHK(hipGetLastError());
        HIPCHK(pool.d2h(head, d.head, sizeof(head)));
        HIPCHK(pool.fetch_finish());
        K = head[ESS_H_VERTICES];
        const long long e = (long long)head[ESS_H_KIND] + head[ESS_H_KIND + 1] + head[ESS_H_KIND + 2] + head[ESS_H_KIND + 3];
        if (e > 0x3FFFFFFF) { corb_set_error("%s: %lld edges", who, e); return CORB_ERR_ARG; }
        E = (int)e;
        return CORB_OK;
    }
    void counts(CorbEssentialGraphCounts* o) const
    {
        memset(o, 0, sizeof(*o));
        o->n_vertices = K; o->n_edges = E;
        for (int k = 0; k < 4; k++) o->n_kind[k] = head[ESS_H_KIND + k];
        o->n_dropped = head[ESS_H_DROPPED]; o->n_lc_below_weight = head[ESS_H_LC_BELOW];
        for (int k = 0; k < 6; k++) o->n_suppressed[k] = head[ESS_H_SUPPRESSED + k];
    }
    int fill(CorbCovis* g)
    {
        CorbScratch& pool = *call.scratch;
        const size_t n = (size_t)std::max(E, 1);
        HIPCHK(pool.alloc(&d.vi, n * 2)); d.vj = d.vi + n; HIPCHK(pool.alloc(&d.kind, n)); HIPCHK(pool.alloc(&d.meas, n * 8));
        d.n_edges = E;
        ess_launch_fill(g->R, g->T, call.S, d, pool.stream);
        HIPCHK(hipGetLastError());
        return CORB_OK;
    }
};
}

extern "C" int corb_essential_graph_plan(CorbCovis* g, const CorbEssentialGraphInput* in, int v_cap, int e_cap, int32_t* v_slots, double* S, uint8_t* fixed, double* snc,
                                         int32_t* vi, int32_t* vj, uint8_t* kind, double* measurement, CorbEssentialGraphCounts* counts)
{
    const char* who = "corb_essential_graph_plan";
    if (!counts || v_cap < 0 || e_cap < 0) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    EssPlan p;
    int rc = p.run(g, in, who); if (rc) return rc;
    p.counts(counts);
    if (p.K > v_cap || p.E > e_cap) { corb_set_error("%s: %d vertices and %d edges, v_cap = %d, e_cap = %d; nothing was written", who, p.K, p.E, v_cap, e_cap); return CORB_ERR_CAPACITY; }
    rc = p.fill(g); if (rc) return rc;
    CorbScratch& pool = *p.call.scratch;
    const size_t K = (size_t)p.K, E = (size_t)p.E;
    if (v_slots) HIPCHK(pool.d2h(v_slots, p.d.vslot, K * 4));
    if (S) HIPCHK(pool.d2h(S, p.d.S, K * 64));
    if (snc) HIPCHK(pool.d2h(snc, p.d.snc, K * 64));
    if (fixed) HIPCHK(pool.d2h(fixed, p.d.fixed, K));
    if (vi) HIPCHK(pool.d2h(vi, p.d.vi, E * 4));
    if (vj) HIPCHK(pool.d2h(vj, p.d.vj, E * 4));
    if (kind) HIPCHK(pool.d2h(kind, p.d.kind, E));
    if (measurement) HIPCHK(pool.d2h(measurement, p.d.meas, E * 64));
    HIPCHK(pool.fetch_finish());
    return CORB_OK;
}

extern "C" int corb_essential_graph_store(CorbCovis* g, const CorbEssentialGraphInput* in, int iterations, int fix_scale, float scale_factor, double* chi2_hist,
                                          double* S_final, int v_cap, CorbEssentialGraphResult* out)
{
    const char* who = "corb_essential_graph_store";
    if (!out || iterations < 0 || (S_final && v_cap < 0)) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    EssPlan p;
    int rc = p.run(g, in, who); if (rc) return rc;
    memset(out, 0, sizeof(*out));
    p.counts(&out->graph);
    const int K = p.K, E = p.E;
    if (S_final && K > v_cap) { corb_set_error("%s: %d vertices, v_cap = %d; nothing was written", who, K, v_cap); return CORB_ERR_CAPACITY; }
    if (K < 1) return CORB_OK;                                                                   // no keyframe: nothing to optimise, no point has a vertex to hang on
    rc = p.fill(g); if (rc) return rc;
    CorbScratch& pool = *p.call.scratch;
    // the one download the accumulation lists need: (vi, vj) and the K fixed flags
    std::vector<int32_t> hv((size_t)std::max(E, 1) * 2); std::vector<unsigned char> hfixed((size_t)K);
    if (E > 0) HIPCHK(pool.d2h(hv.data(), p.d.vi, (size_t)E * 8));                               // vj lies behind vi in one allocation
    HIPCHK(pool.d2h(hfixed.data(), p.d.fixed, (size_t)K));
    HIPCHK(pool.fetch_finish());
    const int32_t* hvi = hv.data(); const int32_t* hvj = hv.data() + E;
    std::vector<int> idx((size_t)K);
    const int nP = eg_free_index(K, hfixed.data(), idx.data());
    rc = eg_check_size(who, nP); if (rc) return rc;
    CorbGraphDev d; memset(&d, 0, sizeof(d));
    d.K = K; d.E = E; d.nP = nP; d.sp = 7 * nP; d.fix_scale = fix_scale ? 1 : 0;
    double* dV = nullptr; int* didx = nullptr;
    HIPCHK(pool.alloc(&dV, (size_t)8 * K)); HIPCHK(pool.upload(&didx, idx));
    HIPCHK(hipMemcpyAsync(dV, p.d.S, sizeof(double) * 8 * (size_t)K, hipMemcpyDeviceToDevice, pool.stream));   // p.d.S stays the initial value (Srw of :1101)
    d.V = dV; d.fixed = p.d.fixed; d.idx = didx; d.vi = p.d.vi; d.vj = p.d.vj; d.meas = p.d.meas;
    EgSystem sys{};
    rc = eg_alloc_system(pool, d, sys); if (rc) return rc;
    rc = eg_build_lists(pool, d, hfixed.data(), idx.data(), hvi, hvj); if (rc) return rc;
    int it_done = 0;
    rc = eg_levenberg(pool, d, sys, iterations, chi2_hist, &it_done); if (rc) return rc;
    out->iters_done = it_done;
    ess_launch_commit(p.call.S, p.d, K, p.d.S, dV, g->mp->idt_first, g->mp->idt_n, scale_factor, pool.stream);
    HIPCHK(hipGetLastError());
    int head[ESS_H_INTS];
    HIPCHK(pool.d2h(head, p.d.head, sizeof(head)));
    if (S_final) HIPCHK(pool.d2h(S_final, dV, (size_t)K * 64));
    HIPCHK(pool.fetch_finish());
    out->n_poses_set = head[ESS_H_POSES]; out->n_points_moved = head[ESS_H_MOVED]; out->n_points_kept = head[ESS_H_KEPT];
    out->n_points_skipped = head[ESS_H_SKIPPED]; out->n_points_fixed_ref = head[ESS_H_FIXED_REF];
    return CORB_OK;
}

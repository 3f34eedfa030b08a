// covis_host.h -- host-side object of the covisibility graph and one call's hold on it (corb_covis.cpp, corb_localmap.cpp)
#pragma once
#include "covis_internal.h"
#include "record_call.h"
#include <memory>

struct CorbCovis {
    CorbKfStore* kf = nullptr; CorbMpStore* mp = nullptr;
    CovisRows R{};
    CovisTree T{};
    int device = 0;
    DevMem mem, tree_mem;                    // what R and T point into
    DevMem bef_mem;                          // [capacity][16] mTcwBefGBA of slot r (C/include/KeyFrame.h:63); a fresh graph holds the identity
    float* bef() const { return bef_mem.as<float>(); }
    DevMem loop_mem;                         // mspLoopEdges of every slot: [capacity][CORB_COVIS_MAX_LOOP_EDGES] ids, then [capacity] counts (corb_essgraph.cpp); a fresh graph holds empty sets
    std::mutex mu;
};

// one call's hold on the graph and the stores (record_call.h), and the stores as the kernels read them.  `frames` (optional): a second keyframe store the call
// reads a record of
struct CovisCall {
    RecordCall rec;
    std::unique_ptr<CorbScratch> scratch;            // taken after the stores' locks, as every store call does
    CovisStores S{};
    int begin(CorbCovis* g, const char* who, bool need_points, CorbKfStore* frames = nullptr, int lane = 0)
    {
        CorbKfStore* kf = g->kf; CorbMpStore* mp = g->mp;
        rec.hold(&g->mu, kf, frames, mp);
        scratch.reset(new CorbScratch(lane));                // lane 1: the long optimisations (corb_essgraph.cpp)
        CorbScratch& pool = *scratch;
        if (!pool.stream) { corb_set_error("%s: no workspace stream", who); return CORB_ERR_HIP; }
        int rc = need_points ? record_need_index(who, mp) : CORB_OK; if (rc) return rc;
        rc = record_join(kf->stream, mp->stream, frames ? frames->stream : nullptr); if (rc) return rc;
        S.kf_base = kf->base(); S.kf_bytes = kf->L.bytes; S.F = kf->F; S.kf_capacity = kf->capacity;
        S.mp_base = mp->base(); S.mp_bytes = mp->L.bytes; S.O = mp->O; S.mp_capacity = mp->capacity; S.mpid = mp->idt;
        rc = id_table_scratch(pool, kf->capacity, S.kfid, true, pool.stream); if (rc) return rc;
        corb_launch_kf_index(S.kf_base, S.kf_bytes, 0, S.kf_capacity, S.kfid, pool.stream);        // "in the cache" (Cache::KeyFrameInCache) means: found in this table
        HIPCHK(hipGetLastError());
        return CORB_OK;
    }
};
// the loop-edge sets of a new graph (corb_essgraph.cpp); CORB_ERR_HIP with the message set
int essgraph_loop_sets_create(CorbCovis* g);
inline int covis_slot_ok(CorbCovis* g, int slot, const char* who)
{
    if (!g || slot < 0 || slot >= g->kf->capacity) { corb_set_error("%s: bad graph / slot", who); return CORB_ERR_ARG; }
    return CORB_OK;
}

// covis_host.h -- host-side object of the covisibility graph and one call's hold on it (corb_covis.cpp, corb_localmap.cpp)
#pragma once
#include "covis_internal.h"
#include "store_host.h"
#include "corb_workspace.h"
#include <memory>
#include <mutex>
#include <utility>

void corb_set_error(const char* fmt, ...);
int corb_select_device(int device);
#define COVIS_HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { corb_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); return CORB_ERR_HIP; } } while (0)

struct CorbCovis {
    CorbKfStore* kf = nullptr; CorbMpStore* mp = nullptr;
    CovisRows R{};
    CovisTree T{};
    char* mem = nullptr;
    char* tree_mem = nullptr;
    float* bef = nullptr;                    // [capacity][16] mTcwBefGBA of slot r (C/include/KeyFrame.h:63); a fresh graph holds the identity
    std::mutex mu;
};

// one call's hold on the graph and the stores, and the stores as the kernels read them.  `frames` (optional): a second keyframe store the call reads a record of;
// the keyframe stores are locked once each, by address, then the map (the order of the calls on records, corb_fuse_store)
struct CovisCall {
    std::unique_lock<std::mutex> lk_g, lk_kf, lk_kf2, lk_mp;
    std::unique_ptr<CorbScratch> scratch;            // taken after the stores' locks, as every store call does
    CovisStores S{};
    int begin(CorbCovis* g, const char* who, bool need_points, CorbKfStore* frames = nullptr)
    {
        CorbKfStore* kf = g->kf; CorbMpStore* mp = g->mp;
        lk_g = std::unique_lock<std::mutex>(g->mu);
        CorbKfStore* lo = kf; CorbKfStore* hi = (frames && frames != kf) ? frames : nullptr;
        if (hi && hi < lo) std::swap(lo, hi);
        lk_kf = std::unique_lock<std::mutex>(lo->mu); if (hi) lk_kf2 = std::unique_lock<std::mutex>(hi->mu);
        lk_mp = std::unique_lock<std::mutex>(mp->mu);
        scratch.reset(new CorbScratch(0));
        CorbScratch& pool = *scratch;
        if (!pool.stream) { corb_set_error("%s: no workspace stream", who); return CORB_ERR_HIP; }
        if (need_points && (!mp->idt.keys || !mp->idt_valid)) { corb_set_error("%s: the map-point store has no current id index (corb_mp_store_build_index after the last put / push)", who); return CORB_ERR_ARG; }
        COVIS_HIPCHK(hipStreamSynchronize(kf->stream)); COVIS_HIPCHK(hipStreamSynchronize(mp->stream));
        if (hi) COVIS_HIPCHK(hipStreamSynchronize(frames->stream));
        S.kf_base = kf->base; S.kf_bytes = kf->L.bytes; S.F = kf->F; S.kf_capacity = kf->capacity;
        S.mp_base = mp->base; S.mp_bytes = mp->L.bytes; S.O = mp->O; S.mp_capacity = mp->capacity; S.mpid = mp->idt;
        unsigned int cap = 64; while (cap < 2u * (unsigned int)kf->capacity) cap <<= 1;
        COVIS_HIPCHK(pool.alloc(&S.kfid.keys, (size_t)cap)); COVIS_HIPCHK(pool.alloc(&S.kfid.vals, (size_t)cap)); S.kfid.mask = cap - 1;
        COVIS_HIPCHK(hipMemsetAsync(S.kfid.keys, 0xFF, (size_t)cap * 8, pool.stream));
        COVIS_HIPCHK(hipMemsetAsync(S.kfid.vals, 0x7F, (size_t)cap * 4, pool.stream));              // (corb_idtab_insert_min)
        corb_launch_kf_index(S.kf_base, S.kf_bytes, 0, S.kf_capacity, S.kfid, pool.stream);        // "in the cache" (Cache::KeyFrameInCache) means: found in this table
        COVIS_HIPCHK(hipGetLastError());
        return CORB_OK;
    }
};
inline int covis_slot_ok(CorbCovis* g, int slot, const char* who)
{
    if (!g || slot < 0 || slot >= g->kf->capacity) { corb_set_error("%s: bad graph / slot", who); return CORB_ERR_ARG; }
    return CORB_OK;
}

// record_call.h -- what every call on device-resident records does before it touches one, in this order: the argument checks that read no store state (the
// caller's own); the device; the locks (record_locks.h); and only under the locks the feature counts of the slots, which a put from another thread may change
// until then, and the map's id index where ids are resolved.  The caller initialises its outputs from the counts, takes its early return, and only then waits
// for the stores' streams.  Also the id tables such calls build (a table a handle keeps between calls: owned_hip.h).  Host code only.
#pragma once
#include "host_util.h"
#include "store_host.h"
#include "corb_workspace.h"
#include "record_locks.h"

// the features of (kf, slot); -1 with the message set if the slot is empty.  need_header: the host mirror of the slot's node ids must be current as well
inline int record_slot_count(const char* who, const CorbKfStore* kf, int slot, bool need_header = false)
{
    const CorbKfStore::Host& h = kf->host[slot];
    if (h.n >= 0 && (h.header_valid || !need_header)) return h.n;
    corb_set_error("%s: slot %d is empty (or was filled without a host-known feature count)", who, slot);
    return -1;
}
// the call resolves MapPoint ids through the map's id index
inline int record_need_index(const char* who, const CorbMpStore* map)
{
    if (map->idt.keys && map->idt_valid) return CORB_OK;
    corb_set_error("%s: the map-point store has no current id index (corb_mp_store_build_index after the last put / push)", who);
    return CORB_ERR_ARG;
}
// the stores' own streams may still be filling the records: the call runs on its own stream after them.  Each distinct stream is waited for once, in argument order
inline int record_join(hipStream_t a, hipStream_t b = nullptr, hipStream_t c = nullptr)
{
    if (a) HIPCHK(hipStreamSynchronize(a));
    if (b && b != a) HIPCHK(hipStreamSynchronize(b));
    if (c && c != a && c != b) HIPCHK(hipStreamSynchronize(c));
    return CORB_OK;
}

// one call's hold on its records: an owner's mutex (or null), up to two keyframe stores (either may be null, the two may be one) and the map (or null)
struct RecordCall {
    RecordLocks locks;
    CorbKfStore* kf = nullptr; CorbKfStore* kf2 = nullptr; CorbMpStore* map = nullptr;
    void hold(std::mutex* owner, CorbKfStore* kf_, CorbKfStore* kf2_, CorbMpStore* map_)
    {
        kf = kf_; kf2 = kf2_; map = map_;
        locks.take(owner, kf ? &kf->mu : nullptr, kf2 ? &kf2->mu : nullptr, map ? &map->mu : nullptr);
    }
    int join() const { return record_join(kf ? kf->stream : nullptr, kf2 ? kf2->stream : nullptr, map ? map->stream : nullptr); }
};

// ---- id tables (device_util.h): 8-byte keys preset to CORB_IDTAB_EMPTY; for_min: 4-byte values preset to 0x7F7F7F7F, ready for corb_idtab_insert_min ----
inline int id_table_clear(const CorbIdTable& t, bool for_min, hipStream_t s)
{
    const size_t cap = (size_t)t.mask + 1;
    HIPCHK(hipMemsetAsync(t.keys, 0xFF, cap * 8, s));
    if (for_min) HIPCHK(hipMemsetAsync(t.vals, 0x7F, cap * 4, s));
    return CORB_OK;
}
// an empty table of `entries` ids that lives as long as the call: keys, then values, out of the call's bump allocator (CorbScratch, the store BA's DevBuf)
template <class Pool> int id_table_scratch(Pool& pool, long long entries, CorbIdTable& t, bool for_min, hipStream_t s)
{
    const size_t cap = id_table_capacity(entries);
    HIPCHK(pool.alloc(&t.keys, cap)); HIPCHK(pool.alloc(&t.vals, cap)); t.mask = (unsigned int)(cap - 1);
    return id_table_clear(t, for_min, s);
}

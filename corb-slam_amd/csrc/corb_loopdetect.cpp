// corb_loopdetect.cpp -- C-ABI host side of include/corb_loop_detect.h: LoopClosing::DetectLoop on records, for one keyframe and for a queue.  The object owns its
// device memory, its id table, its page-locked staging and its stream: no call here opens a workspace lane.
// Locks: the detector, the database, the graph, the keyframe store (record_locks.h; the database before the stores as corb_fusion.cpp takes it).
// A detect call enqueues every keyframe's kernels on the object's stream with nothing between them but the stream's order, reads the block back once and only then
// brings the database's host mirrors (live set, add sequence) to what the device decided.  Entry k of a queue is added with sequence number next_seq + k: every
// keyframe before the stopping one is added exactly once, so the number does not depend on the outcomes.
#include "loopdetect_internal.h"
#include "covis_host.h"
#include "record_call.h"
#include <algorithm>
#include <cstring>
#include <vector>

struct CorbLoopDetector {
    CorbCovis* g = nullptr; CorbKfDb* db = nullptr;
    int device = 0, max_cand = 0, max_groups = 0, n_slots = 0, n_entries = 0;
    OwnedStream stream;
    std::mutex mu;
    DevMem mem;                                           // everything LdDev points into but the id table
    OwnedIdTable kfid;
    PinnedMem back;                                       // the read-back block's host side
    LdDev d{};
    size_t block_bytes = 0;
    std::vector<int32_t> slot_entry, entry_slot;          // host mirror of the binding
};

namespace {
inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// one call's opening: the device and the locks; with `stores` the database, the graph and its keyframe store as well, and the views the kernels read
struct LdCall {
    std::unique_lock<std::mutex> lk_det, lk_db;
    RecordCall rec;
    int open(const char* who, CorbLoopDetector* det, bool args_ok, bool stores)
    {
        if (!det || !args_ok) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
        int rc = corb_select_device(det->device); if (rc) return rc;
        lk_det = std::unique_lock<std::mutex>(det->mu);
        if (stores) {
            lk_db = std::unique_lock<std::mutex>(det->db->mu);
            rec.hold(&det->g->mu, det->g->kf, nullptr, nullptr);
            det->d.kf_base = det->g->kf->base(); det->d.R = det->g->R;
        }
        return CORB_OK;
    }
};
int upload_binding(CorbLoopDetector* det)
{
    HIPCHK(hipMemcpyAsync(det->d.slot_entry, det->slot_entry.data(), det->slot_entry.size() * 4, hipMemcpyHostToDevice, det->stream));
    HIPCHK(hipMemcpyAsync(det->d.entry_slot, det->entry_slot.data(), det->entry_slot.size() * 4, hipMemcpyHostToDevice, det->stream));
    HIPCHK(hipStreamSynchronize(det->stream));
    return CORB_OK;
}
int read_state(CorbLoopDetector* det, LdState* st)
{
    HIPCHK(hipMemcpyAsync(st, det->d.st, sizeof(LdState), hipMemcpyDeviceToHost, det->stream));
    HIPCHK(hipStreamSynchronize(det->stream));
    return CORB_OK;
}
int write_field(CorbLoopDetector* det, size_t offset, const void* v, size_t bytes)
{
    HIPCHK(hipMemcpyAsync(reinterpret_cast<char*>(det->d.st) + offset, v, bytes, hipMemcpyHostToDevice, det->stream));
    HIPCHK(hipStreamSynchronize(det->stream));
    return CORB_OK;
}

// DetectLoop for slots[0 .. n): the whole queue enqueued, one read-back
int detect(const char* who, CorbLoopDetector* det, const int32_t* slots, int n, CorbLoopDetectResult* res, int32_t* cand_entries, int32_t* cand_slots, int32_t* enough, int* n_consumed)
{
    LdCall c; int rc = c.open(who, det, n >= 0 && n <= CORB_LOOP_DETECT_MAX_QUEUE && (n == 0 || (slots && res)) && n_consumed, true); if (rc) return rc;
    *n_consumed = 0;
    if (n == 0) return CORB_OK;
    CorbKfStore* kf = det->g->kf; CorbKfDb* db = det->db;
    std::vector<int> entry((size_t)n);
    std::vector<char> seen((size_t)det->n_slots, 0);
    for (int k = 0; k < n; k++) {
        const int s = slots[k];
        if (s < 0 || s >= det->n_slots) { corb_set_error("%s: slot %d of %d", who, s, det->n_slots); return CORB_ERR_ARG; }
        if (seen[s]) { corb_set_error("%s: slot %d is listed twice", who, s); return CORB_ERR_ARG; }
        seen[s] = 1;
        if (record_slot_count(who, kf, s) < 0) return CORB_ERR_ARG;
        if (kf->host[s].n == 0) { corb_set_error("%s: slot %d holds no feature: it is not a keyframe", who, s); return CORB_ERR_ARG; }
        const int e = det->slot_entry[s];
        if (e < 0) { corb_set_error("%s: slot %d has no bound database entry (corb_loop_detector_bind)", who, s); return CORB_ERR_ARG; }
        if (db->n_words[e] < 0 || db->live[e]) { corb_set_error("%s: entry %d of slot %d %s", who, e, s, db->live[e] ? "is in the database already" : "has no BowVector"); return CORB_ERR_ARG; }
        entry[k] = e;
    }
    if (db->next_seq > 0xFFFFFFFFu - (uint32_t)n) { corb_set_error("%s: 2^32 adds; clear the database", who); return CORB_ERR_OVERFLOW; }
    HIPCHK(hipStreamSynchronize(kf->stream));                                                    // the records and the database may still be filling
    HIPCHK(hipStreamSynchronize(db->stream));
    hipStream_t s = det->stream;
    const LdDev& d = det->d;
    rc = id_table_clear(det->kfid, true, s); if (rc) return rc;
    corb_launch_kf_index(d.kf_base, d.kf_bytes, 0, det->n_slots, det->kfid, s);
    const size_t used = 256 + (size_t)n * d.item_bytes;
    HIPCHK(hipMemsetAsync(d.block, 0, used, s));
    for (int k = 0; k < n; k++) {
        ld_launch_begin(d, db->d, k, slots[k], s);
        corb_launch_kfdb_loop_query(db->d, entry[k], db->n_words[entry[k]], d.q, d.score_list, d.R.M, s);
        ld_launch_groups(d, db->d, k, s);
        ld_launch_close(d, db->d, k, entry[k], db->next_seq + (uint32_t)k, s);
    }
    HIPCHK(hipGetLastError());
    char* host = det->back.as<char>();
    HIPCHK(hipMemcpyAsync(host, d.block, used, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const LdHead& H = *reinterpret_cast<const LdHead*>(host);
    const int done = std::min(std::max(H.consumed, 0), n);
    for (int k = 0; k < done; k++) db->live[entry[k]] = 1;                                       // the host mirrors follow the device
    db->next_seq += (uint32_t)done;
    *n_consumed = done;
    const size_t MC = (size_t)det->max_cand;
    for (int k = 0; k < std::min(done + 1, n); k++) {
        const char* item = host + 256 + (size_t)k * d.item_bytes;
        const LdItem& it = *reinterpret_cast<const LdItem*>(item);
        if (k == done && it.status == CORB_OK) break;                                            // gated off: behind the stopping keyframe
        res[k] = it.r;
        if (k == done) {
            if (it.status == CORB_ERR_ARG) corb_set_error("%s: a covisible keyframe of slot %d has no bound database entry with a BowVector; the keyframe is not processed", who, slots[k]);
            else if (it.pad[0] == 1) corb_set_error("%s: slot %d has %d candidates, max_candidates = %d; the keyframe is not processed", who, slots[k], it.r.n_candidates, det->max_cand);
            else corb_set_error("%s: slot %d gives more than max_groups = %d consistent groups (%d before it, %d candidates); the keyframe is not processed", who, slots[k], det->max_groups, it.r.n_groups, it.r.n_candidates);
            return it.status;
        }
        const int32_t* ints = reinterpret_cast<const int32_t*>(item + sizeof(LdItem));
        const size_t nc = (size_t)std::min(std::max(it.r.n_candidates, 0), det->max_cand), ne = (size_t)std::min(std::max(it.r.n_enough, 0), det->max_cand);
        if (cand_entries && nc) memcpy(cand_entries + (size_t)k * MC, ints, nc * 4);
        if (cand_slots && nc) memcpy(cand_slots + (size_t)k * MC, ints + MC, nc * 4);
        if (enough && ne) memcpy(enough + (size_t)k * MC, ints + 2 * MC, ne * 4);
    }
    return CORB_OK;
}
}  // namespace

extern "C" int corb_loop_detector_create(CorbCovis* g, CorbKfDb* db, int max_candidates, int max_groups, CorbLoopDetector** out)
{
    const char* who = "corb_loop_detector_create";
    if (!out || !g || !db || max_candidates < 1 || max_candidates > 4096 || max_groups < 1 || max_groups > 4096) {
        corb_set_error("%s: bad argument (1 <= max_candidates, max_groups <= 4096)", who); return CORB_ERR_ARG;
    }
    *out = nullptr;
    if (g->device != db->device) { corb_set_error("%s: the graph and the database live on different devices", who); return CORB_ERR_ARG; }
    int rc = corb_select_device(g->device); if (rc) return rc;
    CorbLoopDetector* det = new CorbLoopDetector();
    det->g = g; det->db = db; det->device = g->device; det->max_cand = max_candidates; det->max_groups = max_groups;
    det->n_slots = g->kf->capacity; det->n_entries = db->d.capacity;
    det->slot_entry.assign((size_t)det->n_slots, -1); det->entry_slot.assign((size_t)det->n_entries, -1);
    const size_t S = (size_t)det->n_slots, E = (size_t)det->n_entries, MC = (size_t)max_candidates, MG = (size_t)max_groups, W = (S + 63) / 64, M = (size_t)g->R.M;
    LdDev& d = det->d;
    d.item_bytes = (sizeof(LdItem) + 3 * MC * 4 + 31) & ~(size_t)31;
    det->block_bytes = 256 + (size_t)CORB_LOOP_DETECT_MAX_QUEUE * d.item_bytes;
    size_t o = 0;
    const size_t o_block = o; o += al256(det->block_bytes);
    const size_t o_st = o; o += 256;
    const size_t o_q = o; o += 256;
    const size_t o_bind = o; o += al256(S * 4) + al256(E * 4);                 // the 0xFF part: slot_entry | entry_slot
    const size_t o_grp = o; o += al256(2 * MG * W * 8);
    const size_t o_cnt = o; o += al256(2 * MG * 4);
    const size_t o_cb = o; o += al256(MC * W * 8);
    const size_t o_cons = o; o += al256(MC * MG);
    const size_t o_first = o; o += al256(MG * 4);
    const size_t o_src = o; o += al256(MG * 4);
    const size_t o_pos = o; o += 4 * al256((MC + 1) * 4);
    const size_t o_score = o; o += al256(M * 4);
    if (det->stream.create() != hipSuccess || det->mem.room(o) != hipSuccess || det->kfid.room((long long)S) != hipSuccess || det->back.room(det->block_bytes) != hipSuccess) {
        corb_set_error("%s: %d candidates x %d groups over %d slots: allocation failed", who, max_candidates, max_groups, det->n_slots); delete det; return CORB_ERR_HIP;
    }
    char* m = det->mem.as<char>();
    d.kf_base = g->kf->base(); d.kf_bytes = g->kf->L.bytes; d.n_slots = det->n_slots; d.W = (int)W; d.kfid = det->kfid; d.R = g->R;
    d.slot_entry = reinterpret_cast<int*>(m + o_bind); d.entry_slot = reinterpret_cast<int*>(m + o_bind + al256(S * 4)); d.n_entries = det->n_entries;
    d.st = reinterpret_cast<LdState*>(m + o_st); d.q = reinterpret_cast<BowLoopQuery*>(m + o_q);
    d.grp_bits = reinterpret_cast<unsigned long long*>(m + o_grp); d.grp_cnt = reinterpret_cast<int*>(m + o_cnt);
    d.cand_bits = reinterpret_cast<unsigned long long*>(m + o_cb); d.cons = reinterpret_cast<unsigned char*>(m + o_cons);
    d.first = reinterpret_cast<int*>(m + o_first); d.src = reinterpret_cast<int*>(m + o_src);
    d.pos = reinterpret_cast<int*>(m + o_pos); d.any = reinterpret_cast<int*>(m + o_pos + al256((MC + 1) * 4));
    d.en = reinterpret_cast<int*>(m + o_pos + 2 * al256((MC + 1) * 4)); d.epos = reinterpret_cast<int*>(m + o_pos + 3 * al256((MC + 1) * 4));
    d.score_list = reinterpret_cast<int*>(m + o_score);
    d.block = m + o_block; d.max_cand = max_candidates; d.max_groups = max_groups;
    LdState st{}; st.th = 3;                                                    // mnCovisibilityConsistencyTh = 3 (LoopClosing.cc:42), mLastLoopKFid = 0 (:41)
    if (hipMemsetAsync(m, 0, o, det->stream) != hipSuccess || hipMemsetAsync(m + o_bind, 0xFF, al256(S * 4) + al256(E * 4), det->stream) != hipSuccess ||
        hipMemcpyAsync(d.st, &st, sizeof(st), hipMemcpyHostToDevice, det->stream) != hipSuccess || hipStreamSynchronize(det->stream) != hipSuccess) {
        corb_set_error("%s: the state's initialisation failed", who); delete det; return CORB_ERR_HIP;
    }
    *out = det;
    return CORB_OK;
}
extern "C" void corb_loop_detector_destroy(CorbLoopDetector* det) { handle_destroy(det); }

extern "C" int corb_loop_detector_bind(CorbLoopDetector* det, const int32_t* slots, const int32_t* entries, int n)
{
    const char* who = "corb_loop_detector_bind";
    LdCall c; int rc = c.open(who, det, n >= 0 && (n == 0 || (slots && entries)), false); if (rc) return rc;
    std::vector<char> seen_s((size_t)det->n_slots, 0), seen_e((size_t)det->n_entries, 0);
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= det->n_slots || entries[i] < -1 || entries[i] >= det->n_entries) { corb_set_error("%s: pair %d (slot %d of %d, entry %d of %d)", who, i, slots[i], det->n_slots, entries[i], det->n_entries); return CORB_ERR_ARG; }
        if (seen_s[slots[i]] || (entries[i] >= 0 && seen_e[entries[i]])) { corb_set_error("%s: pair %d names a slot or an entry the list has already", who, i); return CORB_ERR_ARG; }
        seen_s[slots[i]] = 1; if (entries[i] >= 0) seen_e[entries[i]] = 1;
    }
    for (int i = 0; i < n; i++) {
        const int s = slots[i], e = entries[i];
        if (det->slot_entry[s] >= 0) det->entry_slot[det->slot_entry[s]] = -1;
        if (e >= 0 && det->entry_slot[e] >= 0) det->slot_entry[det->entry_slot[e]] = -1;
        det->slot_entry[s] = e;
        if (e >= 0) det->entry_slot[e] = s;
    }
    return upload_binding(det);
}

extern "C" int corb_loop_detector_set_last_loop(CorbLoopDetector* det, uint64_t id)
{
    LdCall c; int rc = c.open("corb_loop_detector_set_last_loop", det, true, false); if (rc) return rc;
    const unsigned long long v = id;
    return write_field(det, offsetof(LdState, last_loop), &v, 8);
}
extern "C" int corb_loop_detector_get_last_loop(CorbLoopDetector* det, uint64_t* id)
{
    LdCall c; int rc = c.open("corb_loop_detector_get_last_loop", det, id != nullptr, false); if (rc) return rc;
    LdState st; rc = read_state(det, &st); if (rc) return rc;
    *id = st.last_loop;
    return CORB_OK;
}
extern "C" int corb_loop_detector_reset(CorbLoopDetector* det)
{
    LdCall c; int rc = c.open("corb_loop_detector_reset", det, true, false); if (rc) return rc;
    const unsigned long long v = 0;                                             // mLastLoopKFid = 0 (:647); mvConsistentGroups stays
    return write_field(det, offsetof(LdState, last_loop), &v, 8);
}
extern "C" int corb_loop_detector_clear_groups(CorbLoopDetector* det)
{
    LdCall c; int rc = c.open("corb_loop_detector_clear_groups", det, true, false); if (rc) return rc;
    const int v = 0;
    return write_field(det, offsetof(LdState, n_groups), &v, 4);
}
extern "C" int corb_loop_detector_drop_slot(CorbLoopDetector* det, int slot)
{
    const char* who = "corb_loop_detector_drop_slot";
    LdCall c; int rc = c.open(who, det, true, false); if (rc) return rc;
    if (slot < 0 || slot >= det->n_slots) { corb_set_error("%s: slot %d of %d", who, slot, det->n_slots); return CORB_ERR_ARG; }
    ld_launch_drop_slot(det->d, slot, det->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(det->stream));
    return CORB_OK;
}

extern "C" int corb_loop_detector_get_groups(CorbLoopDetector* det, int32_t* counters, int32_t* offsets, int32_t* members, int cap_groups, int cap_members, int* n_groups, int* n_members)
{
    const char* who = "corb_loop_detector_get_groups";
    LdCall c; int rc = c.open(who, det, n_groups && n_members && cap_groups >= 0 && cap_members >= 0, false); if (rc) return rc;
    LdState st; rc = read_state(det, &st); if (rc) return rc;
    const int G = std::min(std::max(st.n_groups, 0), det->max_groups), cur = st.cur & 1;
    const size_t W = (size_t)det->d.W, MG = (size_t)det->max_groups;
    std::vector<unsigned long long> bits((size_t)G * W); std::vector<int32_t> cnt((size_t)G);
    if (G) {
        HIPCHK(hipMemcpyAsync(bits.data(), det->d.grp_bits + (size_t)cur * MG * W, bits.size() * 8, hipMemcpyDeviceToHost, det->stream));
        HIPCHK(hipMemcpyAsync(cnt.data(), det->d.grp_cnt + (size_t)cur * MG, cnt.size() * 4, hipMemcpyDeviceToHost, det->stream));
        HIPCHK(hipStreamSynchronize(det->stream));
    }
    int total = 0;
    for (unsigned long long w : bits) total += __builtin_popcountll(w);
    *n_groups = G; *n_members = total;
    if (G > cap_groups || total > cap_members) { corb_set_error("%s: %d groups of %d members, cap = %d / %d", who, G, total, cap_groups, cap_members); return CORB_ERR_CAPACITY; }
    if ((G && (!counters || !offsets)) || (total && !members)) { corb_set_error("%s: NULL arrays", who); return CORB_ERR_ARG; }
    int at = 0;
    for (int g = 0; g < G; g++) {
        counters[g] = cnt[g]; offsets[g] = at;
        for (size_t w = 0; w < W; w++) for (unsigned long long b = bits[(size_t)g * W + w]; b; b &= b - 1) members[at++] = (int32_t)(w * 64 + (size_t)__builtin_ctzll(b));
    }
    if (offsets) offsets[G] = at;
    return CORB_OK;
}

extern "C" int corb_loop_detect(CorbLoopDetector* det, int slot, CorbLoopDetectResult* res, int32_t* cand_entries, int32_t* cand_slots, int32_t* enough)
{
    int consumed = 0;
    return detect("corb_loop_detect", det, &slot, 1, res, cand_entries, cand_slots, enough, &consumed);
}
extern "C" int corb_loop_detect_queue(CorbLoopDetector* det, const int32_t* slots, int n, CorbLoopDetectResult* res, int32_t* cand_entries, int32_t* cand_slots, int32_t* enough, int* n_consumed)
{
    return detect("corb_loop_detect_queue", det, slots, n, res, cand_entries, cand_slots, enough, n_consumed);
}

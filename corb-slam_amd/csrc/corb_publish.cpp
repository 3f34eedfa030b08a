// corb_publish.cpp -- C-ABI host side of the map publish on records (include/corb_map_publish.h): the server's pack, the client's apply and the collective that
// carries the message between them.  No workspace lane: every temporary lives in the CorbMapPublisher handle -- the message and receive buffers, an output block
// on the device with a page-locked mirror, integer scratch and five id tables, all grown on demand, never freed per call, and written by every call before it
// reads them.  One launch sequence on the handle's stream, one synchronisation and one read-back per call.
#include "publish_internal.h"
#include "publish_math.h"
#include "record_call.h"
#include "comm_internal.h"
#include "owned_hip.h"
#include <algorithm>
#include <cstring>
#include <string>

struct CorbMapPublisher {
    int device = 0;
    OwnedStream stream;
    std::mutex mu;
    DevMem msg;                                                           // the message of the last pack
    int32_t counts[5] = {0, 0, 0, 0, 0}; int kf_bytes = 0, mp_bytes = 0; int64_t msg_bytes = 0;
    DevMem recv;                                                          // what corb_map_publish received
    DevMem out;                                                           // the output block of an apply
    PinnedMem host;                                                       // a pack's slot lists and table on their way up, an apply's output block on its way down
    DevMem scr;                                                           // a pack's slot lists; an apply's ranks, positions, targets and workgroup counts
    OwnedIdTable kfid, first[2], last[2];
};

namespace {
// a buffer of the handle's holds at least `need` bytes: a quarter more than asked when it grows, 4096 at the least
template <class Mem> int grow(Mem& buf, size_t need) { HIPCHK(buf.room(need, std::max(need + need / 4, (size_t)4096))); return CORB_OK; }
int layout(const int32_t* counts, int kfb, int mpb, int64_t* off)
{
    for (int k = 0; k < 5; k++) if (counts[k] < 0) return CORB_ERR_ARG;
    if ((counts[0] > 0 && (kfb <= 0 || kfb % 16)) || (counts[1] > 0 && (mpb <= 0 || mpb % 16))) return CORB_ERR_ARG;
    const int64_t sz[5] = {(int64_t)counts[0] * kfb, (int64_t)counts[1] * mpb, (int64_t)counts[2] * (int64_t)sizeof(CorbKeyFramePosePacket),
                           (int64_t)counts[3] * (int64_t)sizeof(CorbMapPointPosePacket), (int64_t)counts[4] * (int64_t)sizeof(CorbPublishTransform)};
    int64_t o = 0;
    for (int k = 0; k < 5; k++) { off[k] = o; o = (o + sz[k] + 15) & ~(int64_t)15; if (o >= ((int64_t)1 << 31)) return CORB_ERR_ARG; }
    off[5] = o;
    return CORB_OK;
}
bool slots_in(const int32_t* s, int n, int capacity) { for (int i = 0; i < n; i++) if (s[i] < 0 || s[i] >= capacity) return false; return true; }

// ---- pack ----
// everything that can refuse a pack, before anything is written: arguments, the table and its inverses, the buffers, and (under the locks `call` then holds) the
// keyframe slots' feature counts
int pack_check(const char* who, CorbMapPublisher* h, const CorbPublishPack* p, RecordCall& call, std::vector<CorbPublishTransform>& E, int32_t* counts, int64_t* off)
{
    if (!p || p->n_new_kf < 0 || p->n_upd_kf < 0 || p->n_new_mp < 0 || p->n_upd_mp < 0 || p->n_trans < 0 || (p->n_new_kf && !p->new_kf_slots) || (p->n_upd_kf && !p->upd_kf_slots) ||
        (p->n_new_mp && !p->new_mp_slots) || (p->n_upd_mp && !p->upd_mp_slots) || (p->n_trans && (!p->trans_client_id || !p->trans)) ||
        ((p->n_new_kf || p->n_upd_kf) && !p->kf) || ((p->n_new_mp || p->n_upd_mp) && !p->mp)) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    if ((p->kf && p->kf->device != h->device) || (p->mp && p->mp->device != h->device)) { corb_set_error("%s: the stores and the handle live on different devices", who); return CORB_ERR_ARG; }
    if ((p->kf && (!slots_in(p->new_kf_slots, p->n_new_kf, p->kf->capacity) || !slots_in(p->upd_kf_slots, p->n_upd_kf, p->kf->capacity))) ||
        (p->mp && (!slots_in(p->new_mp_slots, p->n_new_mp, p->mp->capacity) || !slots_in(p->upd_mp_slots, p->n_upd_mp, p->mp->capacity)))) { corb_set_error("%s: slot out of range", who); return CORB_ERR_ARG; }
    counts[0] = p->n_new_kf; counts[1] = p->n_new_mp; counts[2] = p->n_upd_kf; counts[3] = p->n_upd_mp; counts[4] = p->n_trans;
    if (layout(counts, p->kf ? (int)p->kf->L.bytes : 0, p->mp ? (int)p->mp->L.bytes : 0, off) != CORB_OK) { corb_set_error("%s: the message would reach 2^31 bytes", who); return CORB_ERR_ARG; }
    E.resize((size_t)p->n_trans);
    std::vector<int32_t> ids(p->trans_client_id, p->trans_client_id + p->n_trans);
    std::sort(ids.begin(), ids.end());
    if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) { corb_set_error("%s: a client id is named twice in the transform table", who); return CORB_ERR_ARG; }
    for (int k = 0; k < p->n_trans; k++) {
        memset(&E[k], 0, sizeof(E[k])); E[k].client_id = p->trans_client_id[k];
        memcpy(E[k].T, p->trans + 16 * (size_t)k, 64);
        if (!pub_inverse4(E[k].T, E[k].Tinv)) { corb_set_error("%s: the transform of client %d has a zero or non-finite determinant", who, E[k].client_id); return CORB_ERR_ARG; }
    }
    int rc = corb_select_device(h->device); if (rc) return rc;
    const size_t n_slots = (size_t)p->n_new_kf + p->n_new_mp + p->n_upd_kf + p->n_upd_mp;
    rc = grow(h->scr, n_slots * 4); if (rc) return rc;
    rc = grow(h->host, al16(n_slots * 4) + E.size() * sizeof(CorbPublishTransform)); if (rc) return rc;
    call.hold(nullptr, p->kf, nullptr, p->mp);                            // (the handle is the caller's to lock)
    for (int pass = 0; pass < 2; pass++) {
        const int32_t* s = pass ? p->upd_kf_slots : p->new_kf_slots; const int n = pass ? p->n_upd_kf : p->n_new_kf;
        for (int i = 0; i < n; i++) if (record_slot_count(who, p->kf, s[i]) < 0) return CORB_ERR_ARG;
    }
    if ((size_t)off[5] > h->msg.cap()) { h->msg_bytes = 0; memset(h->counts, 0, sizeof(h->counts)); }      // (the last refusal is behind: a buffer that grows drops the message it held)
    return grow(h->msg, (size_t)off[5]);
}
// the pack itself, under the locks pack_check took; ends with the handle's one synchronisation
int pack_run(CorbMapPublisher* h, const CorbPublishPack* p, const RecordCall& call, const std::vector<CorbPublishTransform>& E, const int32_t* counts, const int64_t* off)
{
    h->msg_bytes = 0; memset(h->counts, 0, sizeof(h->counts));            // (a pack that fails from here on leaves no message)
    int rc = call.join(); if (rc) return rc;
    int32_t* hs = h->host.as<int32_t>(); int* ds = h->scr.as<int>();
    const int n[4] = {p->n_new_kf, p->n_new_mp, p->n_upd_kf, p->n_upd_mp};
    const int32_t* lists[4] = {p->new_kf_slots, p->new_mp_slots, p->upd_kf_slots, p->upd_mp_slots};
    size_t at[4], total = 0;
    for (int k = 0; k < 4; k++) { at[k] = total; if (n[k]) memcpy(hs + total, lists[k], (size_t)n[k] * 4); total += (size_t)n[k]; }
    if (total) HIPCHK(hipMemcpyAsync(ds, hs, total * 4, hipMemcpyHostToDevice, h->stream));
    if (!E.empty()) {
        char* he = h->host.as<char>() + al16(total * 4);
        memcpy(he, E.data(), E.size() * sizeof(CorbPublishTransform));
        HIPCHK(hipMemcpyAsync(h->msg.as<char>() + off[4], he, E.size() * sizeof(CorbPublishTransform), hipMemcpyHostToDevice, h->stream));
    }
    // the few bytes between a section's end and the next multiple of 16 travel too: zero
    const int64_t end[5] = {off[0] + (int64_t)n[0] * (p->kf ? (int64_t)p->kf->L.bytes : 0), off[1] + (int64_t)n[1] * (p->mp ? (int64_t)p->mp->L.bytes : 0),
                            off[2] + (int64_t)n[2] * (int64_t)sizeof(CorbKeyFramePosePacket), off[3] + (int64_t)n[3] * (int64_t)sizeof(CorbMapPointPosePacket),
                            off[4] + (int64_t)E.size() * (int64_t)sizeof(CorbPublishTransform)};
    for (int k = 0; k < 5; k++) if (off[k + 1] > end[k]) HIPCHK(hipMemsetAsync(h->msg.as<char>() + end[k], 0, (size_t)(off[k + 1] - end[k]), h->stream));
    if (n[0]) corb_launch_gather_records(p->kf->base(), p->kf->L.bytes, ds + at[0], n[0], h->msg.as<char>() + off[0], h->stream);
    if (n[1]) corb_launch_gather_records(p->mp->base(), p->mp->L.bytes, ds + at[1], n[1], h->msg.as<char>() + off[1], h->stream);
    PubPackDev d; memset(&d, 0, sizeof(d));
    if (p->kf) { d.kf_base = p->kf->base(); d.kf_bytes = p->kf->L.bytes; }
    if (p->mp) { d.mp_base = p->mp->base(); d.mp_bytes = p->mp->L.bytes; }
    d.upd_kf = ds + at[2]; d.n_upd_kf = n[2]; d.upd_mp = ds + at[3]; d.n_upd_mp = n[3]; d.sec_c = h->msg.as<char>() + off[2]; d.sec_d = h->msg.as<char>() + off[3];
    pub_launch_pack_poses(d, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(h->counts, counts, sizeof(h->counts)); h->kf_bytes = p->kf ? (int)p->kf->L.bytes : 0; h->mp_bytes = p->mp ? (int)p->mp->L.bytes : 0; h->msg_bytes = off[5];
    return CORB_OK;
}

// ---- apply ----
void zero_outputs(CorbPublishOutputs* o) { if (o) { o->n_kf_inserted = o->n_mp_inserted = o->n_kf_updated = o->n_mp_updated = 0; o->no_transform = 0; } }
bool range_ok(int first, int n, int capacity) { return first >= 0 && n >= 0 && (long long)first + n <= capacity; }
// what an apply can check of its arguments without a lock and without the message
int apply_check(const char* who, const CorbMapPublisher* h, const CorbPublishApply* a)
{
    if (!a || !a->out) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    if ((a->dst_kf && a->dst_kf->device != h->device) || (a->dst_mp && a->dst_mp->device != h->device)) { corb_set_error("%s: the stores and the handle live on different devices", who); return CORB_ERR_ARG; }
    if (a->dst_kf && (!range_ok(a->kf_first, a->kf_n, a->dst_kf->capacity) || !range_ok(a->kf_free_first, a->kf_room, a->dst_kf->capacity) ||
                      (a->kf_n > 0 && a->kf_room > 0 && a->kf_free_first < a->kf_first + a->kf_n && a->kf_first < a->kf_free_first + a->kf_room))) {
        corb_set_error("%s: bad keyframe slot ranges (inside the store, the free slots apart from the resolved ones)", who); return CORB_ERR_ARG;
    }
    if (a->dst_mp && (!range_ok(a->mp_first, a->mp_n, a->dst_mp->capacity) || !range_ok(a->mp_free_first, a->mp_room, a->dst_mp->capacity) ||
                      (a->mp_n > 0 && a->mp_room > 0 && a->mp_free_first < a->mp_first + a->mp_n && a->mp_first < a->mp_free_first + a->mp_room))) {
        corb_set_error("%s: bad map-point slot ranges (inside the store, the free slots apart from the resolved ones)", who); return CORB_ERR_ARG;
    }
    return CORB_OK;
}
// the handle is locked by the caller
int apply_core(const char* who, CorbMapPublisher* h, const char* msg, const int32_t* counts, int kfb, int mpb, const CorbPublishApply* a)
{
    int rc = apply_check(who, h, a); if (rc) return rc;
    CorbPublishOutputs* out = a->out;
    zero_outputs(out);
    int64_t off[6];
    if (!counts || layout(counts, kfb, mpb, off) != CORB_OK) { corb_set_error("%s: bad counts / record sizes", who); return CORB_ERR_ARG; }
    if (off[5] == 0) return CORB_OK;                                      // nothing was published
    const int nA = counts[0], nB = counts[1], nC = counts[2], nD = counts[3];
    if (!msg) { corb_set_error("%s: NULL message", who); return CORB_ERR_ARG; }
    CorbKfStore* kf = a->dst_kf; CorbMpStore* mp = a->dst_mp;
    if (((nA || nC) && !kf) || ((nB || nD) && !mp)) { corb_set_error("%s: the message has entries for a store the call was not given", who); return CORB_ERR_ARG; }
    if ((nA && (size_t)kfb != kf->L.bytes) || (nB && (size_t)mpb != mp->L.bytes)) { corb_set_error("%s: the message's records and the store's differ in size", who); return CORB_ERR_ARG; }
    rc = corb_select_device(h->device); if (rc) return rc;
    RecordCall call; call.hold(nullptr, kf, nullptr, mp);
    if (nB || nD) {
        rc = record_need_index(who, mp); if (rc) return rc;
        if (mp->idt_first != a->mp_first || mp->idt_n != a->mp_n) { corb_set_error("%s: the map's id index covers slots [%d, %d), the call names [%d, %d)", who, mp->idt_first, mp->idt_first + mp->idt_n, a->mp_first, a->mp_first + a->mp_n); return CORB_ERR_ARG; }
        if (nB && a->mp_room > 0 && a->mp_free_first != a->mp_first + a->mp_n) { corb_set_error("%s: the free map-point slots must follow the indexed ones (the id index covers one run of slots)", who); return CORB_ERR_ARG; }
    }
    const int kf_room = kf ? a->kf_room : 0, mp_room = mp ? a->mp_room : 0;
    const int ua = std::min(nA, kf_room), ub = std::min(nB, mp_room);
    const int wa = (nA + PUB_WG - 1) / PUB_WG, wb = (nB + PUB_WG - 1) / PUB_WG;
    // the output block
    const size_t o_hdr = sizeof(PubState), o_sa = o_hdr + (size_t)ua * 16, o_sb = o_sa + al16((size_t)ua * 4), o_ka = o_sb + al16((size_t)ub * 4), o_kb = o_ka + al16((size_t)nA),
                 o_kc = o_kb + al16((size_t)nB), o_kd = o_kc + al16((size_t)nC), out_bytes = o_kd + al16((size_t)nD);
    // the integer scratch
    const size_t sa = corb_scan_scratch_ints((size_t)wa), sb = corb_scan_scratch_ints((size_t)wb);
    size_t ints = 0; auto take = [&](size_t n) { const size_t at = ints; ints += (n + 3) & ~(size_t)3; return at; };
    const size_t i_ra = take(nA), i_pa = take(nA), i_rb = take(nB), i_pb = take(nB), i_tc = take(nC), i_td = take(nD), i_ca = take(wa), i_oa = take((size_t)wa + 1), i_sa = take(sa),
                 i_cb = take(wb), i_ob = take((size_t)wb + 1), i_sb = take(sb);
    rc = grow(h->out, out_bytes); if (rc) return rc;
    rc = grow(h->host, out_bytes); if (rc) return rc;
    rc = grow(h->scr, ints * 4); if (rc) return rc;
    HIPCHK(h->kfid.room(kf ? a->kf_n : 0)); HIPCHK(h->first[0].room(nA)); HIPCHK(h->first[1].room(nB)); HIPCHK(h->last[0].room(nC)); HIPCHK(h->last[1].room(nD));
    // the map's index after the call: in place if the table has room for the new ids too, else a larger table that replaces it once the call has succeeded
    OwnedIdTable grown;                                                   // (whatever it still holds at the end is not the map's)
    if (a->apply && ub > 0 && id_table_capacity((long long)a->mp_n + ub) > (size_t)mp->idt.mask + 1) HIPCHK(grown.own(id_table_capacity((long long)a->mp_n + ub), 256));

    rc = call.join(); if (rc) return rc;
    HIPCHK(hipMemsetAsync(h->out.as<char>(), 0, sizeof(PubState), h->stream));
    rc = id_table_clear(h->kfid, true, h->stream); if (rc) return rc;
    for (int k = 0; k < 2; k++) { if ((rc = id_table_clear(h->first[k], true, h->stream)) || (rc = id_table_clear(h->last[k], true, h->stream))) return rc; }
    if (kf && a->kf_n > 0) corb_launch_kf_index(kf->base(), kf->L.bytes, a->kf_first, a->kf_n, h->kfid, h->stream);

    int* S = h->scr.as<int>();
    PubApplyDev d; memset(&d, 0, sizeof(d));
    d.st = h->out.as<PubState>();
    d.sec_e = reinterpret_cast<const CorbPublishTransform*>(msg + off[4]); d.n_trans = counts[4]; d.client_id = a->client_id; d.apply = a->apply ? 1 : 0;
    PubSide& K = d.s[0]; PubSide& M = d.s[1];
    K.sec_new = msg + off[0]; K.n_new = nA; K.rec_bytes = kf ? kf->L.bytes : 0; K.sec_upd = msg + off[2]; K.n_upd = nC;
    K.base = kf ? kf->base() : nullptr; K.capacity = kf ? kf->capacity : 0; K.free_first = kf ? a->kf_free_first : 0; K.room = kf_room;
    K.held = h->kfid; K.first = h->first[0]; K.last = h->last[0];
    K.kind_new = reinterpret_cast<unsigned char*>(h->out.as<char>() + o_ka); K.kind_upd = reinterpret_cast<unsigned char*>(h->out.as<char>() + o_kc); K.new_slots = reinterpret_cast<int*>(h->out.as<char>() + o_sa);
    K.rank = S + i_ra; K.src = S + i_pa; K.target = S + i_tc; K.wg_cnt = S + i_ca; K.wg_off = S + i_oa; K.scan_scratch = S + i_sa;
    M.sec_new = msg + off[1]; M.n_new = nB; M.rec_bytes = mp ? mp->L.bytes : 0; M.sec_upd = msg + off[3]; M.n_upd = nD;
    M.base = mp ? mp->base() : nullptr; M.capacity = mp ? mp->capacity : 0; M.free_first = mp ? a->mp_free_first : 0; M.room = mp_room;
    M.held = (nB || nD) ? mp->idt : h->last[1] /* (never probed) */; M.first = h->first[1]; M.last = h->last[1];
    M.kind_new = reinterpret_cast<unsigned char*>(h->out.as<char>() + o_kb); M.kind_upd = reinterpret_cast<unsigned char*>(h->out.as<char>() + o_kd); M.new_slots = reinterpret_cast<int*>(h->out.as<char>() + o_sb);
    M.rank = S + i_rb; M.src = S + i_pb; M.target = S + i_td; M.wg_cnt = S + i_cb; M.wg_off = S + i_ob; M.scan_scratch = S + i_sb;
    d.kf_hdr = reinterpret_cast<int*>(h->out.as<char>() + o_hdr);
    d.mp_first = a->mp_first; d.mp_n = a->mp_n; d.new_index = (grown.keys || !mp) ? grown : mp->idt;
    pub_launch_apply(d, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->host.as<char>(), h->out.as<char>(), out_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));

    const PubState* st = h->host.as<const PubState>();
    const int ins_a = std::min(std::max(st->n_ins[0], 0), nA), ins_b = std::min(std::max(st->n_ins[1], 0), nB);
    out->n_kf_inserted = ins_a; out->n_mp_inserted = ins_b; out->n_kf_updated = st->n_upd[0]; out->n_mp_updated = st->n_upd[1]; out->no_transform = st->found ? 0 : 1;
    if (out->kind_kf_new) memcpy(out->kind_kf_new, h->host.as<char>() + o_ka, (size_t)nA);
    if (out->kind_mp_new) memcpy(out->kind_mp_new, h->host.as<char>() + o_kb, (size_t)nB);
    if (out->kind_kf_upd) memcpy(out->kind_kf_upd, h->host.as<char>() + o_kc, (size_t)nC);
    if (out->kind_mp_upd) memcpy(out->kind_mp_upd, h->host.as<char>() + o_kd, (size_t)nD);
    if (out->kf_new_slots) memcpy(out->kf_new_slots, h->host.as<char>() + o_sa, (size_t)std::min(ins_a, ua) * 4);
    if (out->mp_new_slots) memcpy(out->mp_new_slots, h->host.as<char>() + o_sb, (size_t)std::min(ins_b, ub) * 4);
    if (st->overflow) {
        corb_set_error("%s: %d new keyframes for %d free slots, %d new map points for %d; nothing was written", who, ins_a, kf_room, ins_b, mp_room);
        return CORB_ERR_CAPACITY;
    }
    if (!st->go) return CORB_OK;
    // the host's mirror of the slots the keyframes went to
    const int* hdr = reinterpret_cast<const int*>(h->host.as<char>() + o_hdr);
    for (int k = 0; k < ins_a; k++) {
        CorbKfStore::Host& m = kf->host[a->kf_free_first + k];
        const int n = hdr[4 * k], nodes = hdr[4 * k + 1];
        const bool sane = n >= 0 && n <= kf->F && nodes >= 0 && nodes <= kf->F;
        m.n = sane ? n : -1; m.n_nodes = sane ? nodes : 0; memcpy(&m.id, hdr + 4 * k + 2, 8); m.node_id.clear();
        m.header_valid = sane && nodes == 0;                              // (a FeatureVector's node ids are fetched by the first call that needs them)
    }
    if (ins_b > 0) {
        if (grown.keys) mp->idt = std::move(grown);
        mp->idt_first = a->mp_first; mp->idt_n = a->mp_n + ins_b; mp->idt_valid = !st->dup;
        if (st->dup) { corb_set_error("%s: the map holds one id twice after the insertion", who); return CORB_ERR_ARG; }
    }
    return CORB_OK;
}
}  // namespace

extern "C" int corb_pub_create(int device, CorbMapPublisher** out)
{
    if (!out) { corb_set_error("corb_pub_create: bad argument"); return CORB_ERR_ARG; }
    *out = nullptr;
    int rc = corb_select_device(device); if (rc) return rc;
    CorbMapPublisher* h = new CorbMapPublisher; h->device = device;
    if (h->stream.create() != hipSuccess) { corb_set_error("corb_pub_create: stream creation failed"); delete h; return CORB_ERR_HIP; }
    *out = h;
    return CORB_OK;
}

extern "C" void corb_pub_destroy(CorbMapPublisher* h) { handle_destroy(h); }

extern "C" int corb_pub_message_layout(const int32_t counts[5], int kf_record_bytes, int mp_record_bytes, int64_t offsets[6])
{
    if (!counts || !offsets || layout(counts, kf_record_bytes, mp_record_bytes, offsets) != CORB_OK) { corb_set_error("corb_pub_message_layout: bad counts / record sizes"); return CORB_ERR_ARG; }
    return CORB_OK;
}

extern "C" int corb_pub_pack(CorbMapPublisher* h, CorbKfStore* kf, const int32_t* new_kf_slots, int n_new_kf, const int32_t* upd_kf_slots, int n_upd_kf,
                             CorbMpStore* mp, const int32_t* new_mp_slots, int n_new_mp, const int32_t* upd_mp_slots, int n_upd_mp,
                             const int32_t* trans_client_id, const float* trans, int n_trans)
{
    const char* who = "corb_pub_pack";
    if (!h) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    const CorbPublishPack p{kf, new_kf_slots, n_new_kf, upd_kf_slots, n_upd_kf, mp, new_mp_slots, n_new_mp, upd_mp_slots, n_upd_mp, trans_client_id, trans, n_trans};
    std::lock_guard<std::mutex> lk(h->mu);
    RecordCall call; std::vector<CorbPublishTransform> E; int32_t counts[5]; int64_t off[6];
    int rc = pack_check(who, h, &p, call, E, counts, off); if (rc) return rc;
    return pack_run(h, &p, call, E, counts, off);
}

extern "C" int corb_pub_message(CorbMapPublisher* h, void** device_ptr, int64_t* bytes, int32_t counts[5], int32_t* kf_record_bytes, int32_t* mp_record_bytes)
{
    if (!h) { corb_set_error("corb_pub_message: bad argument"); return CORB_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    if (device_ptr) *device_ptr = h->msg_bytes ? h->msg.as<char>() : nullptr;
    if (bytes) *bytes = h->msg_bytes;
    if (counts) memcpy(counts, h->counts, sizeof(h->counts));
    if (kf_record_bytes) *kf_record_bytes = h->kf_bytes;
    if (mp_record_bytes) *mp_record_bytes = h->mp_bytes;
    return CORB_OK;
}

extern "C" int corb_pub_message_read(CorbMapPublisher* h, void* host, int64_t cap)
{
    if (!h || (!host && cap > 0) || cap < 0) { corb_set_error("corb_pub_message_read: bad argument"); return CORB_ERR_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    if (cap < h->msg_bytes) { corb_set_error("corb_pub_message_read: the message has %lld bytes", (long long)h->msg_bytes); return CORB_ERR_CAPACITY; }
    if (h->msg_bytes == 0) return CORB_OK;
    int rc = corb_select_device(h->device); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(host, h->msg.as<char>(), (size_t)h->msg_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CORB_OK;
}

extern "C" int corb_pub_apply(CorbMapPublisher* h, const void* msg, const int32_t counts[5], int kf_record_bytes, int mp_record_bytes, int32_t client_id,
                              CorbKfStore* dst_kf, int kf_first, int kf_n, int kf_free_first, int kf_room,
                              CorbMpStore* dst_mp, int mp_first, int mp_n, int mp_free_first, int mp_room, int apply, CorbPublishOutputs* out)
{
    const char* who = "corb_pub_apply";
    if (!h) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    const CorbPublishApply a{client_id, dst_kf, kf_first, kf_n, kf_free_first, kf_room, dst_mp, mp_first, mp_n, mp_free_first, mp_room, apply, out};
    std::lock_guard<std::mutex> lk(h->mu);
    return apply_core(who, h, static_cast<const char*>(msg), counts, kf_record_bytes, mp_record_bytes, &a);
}

// ---- the collective's bookkeeping: pure arithmetic on what the ranks contributed to the header all-gather ----
extern "C" int corb_map_publish_plan(int world, int root, const CorbPublishHeader* h, int* failing_rank)
{
    if (failing_rank) *failing_rank = -1;
    if (world < 1 || root < 0 || root >= world || !h) { corb_set_error("corb_map_publish_plan: bad argument"); return CORB_ERR_ARG; }
    auto fail = [&](int r, int code) { if (failing_rank) *failing_rank = r; return code; };
    for (int r = 0; r < world; r++) if (h[r].status != 0) { corb_set_error("map publish: rank %d rejected its arguments (status %d)", r, h[r].status); return fail(r, h[r].status); }
    int64_t off[6];
    if (layout(h[root].counts, h[root].kf_record_bytes, h[root].mp_record_bytes, off) != CORB_OK) { corb_set_error("map publish: the root announces bad counts / record sizes"); return fail(root, CORB_ERR_ARG); }
    for (int r = 0; r < world; r++) {
        if (r == root) continue;
        if (h[root].counts[0] > 0 && h[r].kf_record_bytes != h[root].kf_record_bytes) {
            corb_set_error("map publish: rank %d files keyframe records of %d bytes, the root sends records of %d bytes (max_features differ)", r, h[r].kf_record_bytes, h[root].kf_record_bytes);
            return fail(r, CORB_ERR_ARG);
        }
        if (h[root].counts[1] > 0 && h[r].mp_record_bytes != h[root].mp_record_bytes) {
            corb_set_error("map publish: rank %d files map-point records of %d bytes, the root sends records of %d bytes", r, h[r].mp_record_bytes, h[root].mp_record_bytes);
            return fail(r, CORB_ERR_ARG);
        }
    }
    return CORB_OK;
}

extern "C" int corb_map_publish_messages(int world, int rank, int root, const CorbPublishHeader* h, CorbPushMsg* sends, int* n_sends, CorbPushMsg* recvs, int* n_recvs)
{
    int64_t off[6];
    if (world < 1 || rank < 0 || rank >= world || root < 0 || root >= world || !h || !sends || !n_sends || !recvs || !n_recvs ||
        layout(h[root].counts, h[root].kf_record_bytes, h[root].mp_record_bytes, off) != CORB_OK) { corb_set_error("corb_map_publish_messages: bad argument"); return CORB_ERR_ARG; }
    int ns = 0, nr = 0;
    const int n = h[root].counts[0] + h[root].counts[1] + h[root].counts[2] + h[root].counts[3] + h[root].counts[4];
    if (off[5] > 0) {
        if (rank == root) { for (int r = 0; r < world; r++) if (r != root) sends[ns++] = CorbPushMsg{r, 0, 0, n, off[5]}; }
        else recvs[nr++] = CorbPushMsg{root, 0, 0, n, off[5]};
    }
    *n_sends = ns; *n_recvs = nr;
    return CORB_OK;
}

extern "C" int corb_map_publish(CorbComm* c, CorbMapPublisher* h, int root, const CorbPublishPack* pack, const CorbPublishApply* apply_args)
{
    const char* who = "corb_map_publish";
    if (!c) { corb_set_error("%s: NULL communicator", who); return CORB_ERR_ARG; }
    if (root < 0 || root >= c->world) { corb_set_error("%s: bad root", who); return CORB_ERR_ARG; }      // (the same value on every rank, or the job is broken anyway)
    const int W = c->world; const bool is_root = c->rank == root;
    // ---- 1. local verdict: carried into the collective instead of returned, so that no peer waits for a rank that has left ----
    CorbPublishHeader mine; memset(&mine, 0, sizeof(mine));
    std::string local_why;
    auto reject = [&](int code, const char* w) { if (mine.status == 0) { mine.status = code; local_why = w; } };
    std::unique_lock<std::mutex> lk_h;
    if (!h) reject(CORB_ERR_ARG, "NULL handle");
    else { lk_h = std::unique_lock<std::mutex>(h->mu); if (h->device != c->device) reject(CORB_ERR_ARG, "the handle and the communicator live on different devices"); }
    // in-process transport: ranks can share stores.  The root says which stores it reads before anybody takes a lock; the all-gather's barriers keep the next
    // publish's announcement behind this one's readers
    if (c->hub && W > 1) {
        if (is_root) { std::lock_guard<std::mutex> lk(c->hub->mu); c->hub->publish_src[0] = pack ? pack->kf : nullptr; c->hub->publish_src[1] = pack ? pack->mp : nullptr; }
        c->hub->barrier();
    }
    RecordCall call; std::vector<CorbPublishTransform> E; int64_t off[6];
    if (mine.status == 0 && is_root) {
        if (!pack || apply_args) reject(CORB_ERR_ARG, "the root passes the pack arguments and no apply arguments");
        else if (const int r = pack_check(who, h, pack, call, E, mine.counts, off)) { const std::string w = corb_last_error(); reject(r, w.c_str()); }
        else { mine.kf_record_bytes = pack->kf ? (int)pack->kf->L.bytes : 0; mine.mp_record_bytes = pack->mp ? (int)pack->mp->L.bytes : 0; }
    } else if (mine.status == 0) {
        if (!apply_args || pack) reject(CORB_ERR_ARG, "every rank but the root passes the apply arguments and no pack arguments");
        else if (c->hub && ((apply_args->dst_kf && apply_args->dst_kf == c->hub->publish_src[0]) || (apply_args->dst_mp && apply_args->dst_mp == c->hub->publish_src[1])))
            reject(CORB_ERR_ARG, "the destination store is the root's source store");
        else if (const int r = apply_check(who, h, apply_args)) { const std::string w = corb_last_error(); reject(r, w.c_str()); }
        else { mine.kf_record_bytes = apply_args->dst_kf ? (int)apply_args->dst_kf->L.bytes : 0; mine.mp_record_bytes = apply_args->dst_mp ? (int)apply_args->dst_mp->L.bytes : 0; }
    }
    if (corb_select_device(c->device) != CORB_OK) reject(CORB_ERR_HIP, "device selection failed");
    if (mine.status != 0) memset(mine.counts, 0, sizeof(mine.counts));
    // ---- 2. headers of all ranks; every rank evaluates the plan itself: no second round ----
    std::vector<CorbPublishHeader> hdr(W);
    int rc = c->all_gather(reinterpret_cast<const int*>(&mine), 8, reinterpret_cast<int*>(hdr.data()));
    if (rc) return rc;                                     // the transport itself failed: nothing sensible is left to agree on
    int about = -1;
    const int v = corb_map_publish_plan(W, root, hdr.data(), &about);
    if (v != CORB_OK) { if (about == c->rank && !local_why.empty()) corb_set_error("%s: %s", who, local_why.c_str()); return v; }
    if (!is_root) zero_outputs(apply_args->out);
    const CorbPublishHeader& R = hdr[root];
    if (layout(R.counts, R.kf_record_bytes, R.mp_record_bytes, off) != CORB_OK) return CORB_ERR_ARG;      // (unreachable: the plan checked it)
    if (off[5] == 0) return CORB_OK;                       // an all-empty publish: nothing is exchanged
    // ---- 3. the message.  Errors from here on do not return early -- the peers are committed to the exchange: it is entered and the first error returned after it ----
    int rc_first = CORB_OK;
    auto note = [&](int r) { if (r != CORB_OK && rc_first == CORB_OK) rc_first = r; };
    std::vector<Msg> sends, recvs;
    if (is_root) {
        note(pack_run(h, pack, call, E, R.counts, off));   // (into the buffer pack_check reserved: the announced size is there whatever happens)
        call.locks = RecordLocks();                        // packed and waited for: no store lock is held across the transport's barriers
        for (int r = 0; r < W; r++) if (r != root) sends.push_back({h->msg.as<char>(), (size_t)off[5], r});
    } else {
        note(grow(h->recv, (size_t)off[5]));
        // (a rank that cannot allocate its receive buffer posts no receive: the in-process transport copies nothing for it; over RCCL the job is lost, as with
        // any rank that runs out of device memory inside a collective)
        if (h->recv.cap() >= (size_t)off[5]) recvs.push_back({h->recv.as<char>(), (size_t)off[5], root});
    }
    if (W > 1) note(c->exchange(sends, recvs, true));
    if (rc_first != CORB_OK || is_root) return rc_first;
    // ---- 4. every receiver files the message in its own stores; its status is its own ----
    return apply_core(who, h, h->recv.as<char>(), R.counts, R.kf_record_bytes, R.mp_record_bytes, apply_args);
}

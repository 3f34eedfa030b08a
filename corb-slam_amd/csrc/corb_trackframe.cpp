// corb_trackframe.cpp -- C-ABI host side of include/corb_track_frame.h: Tracking::TrackWithMotionModel and Tracking::TrackReferenceKeyFrame on records as one chain
// each on the workspace lane's stream, and the two per-feature loops at the end of Tracking::Track.  The matchers' counts stay on the device: the kernel after a
// search reads them and decides (trackframe_kernels.hip), the wide search's kernels are gated on the first search's count (proj_internal.h), the pose optimisation
// and the tail read the chain's skip words.  The host contributes the velocity, Tlr, the camera and the launch sizes it already knows, and reads one block back.
#include "trackframe_internal.h"
#include "bow_internal.h"
#include "record_call.h"
#include "track_host.h"
#include <vector>
#include <algorithm>

using namespace proj_host;

namespace {
inline size_t al64(size_t v) { return (v + 63) & ~(size_t)63; }

// the result block: head | PoseResult | match [n] | outlier [n] | (TrackReferenceKeyFrame with ComputeBoW) counts [3] | node ids [n]
struct Block {
    size_t o_pose, o_match, o_outl, o_counts, o_nodes, bytes;
    explicit Block(int n, bool bow)
    {
        o_pose = al64(sizeof(TrackFrameHead)); o_match = al64(o_pose + sizeof(track_host::PoseResult)); o_outl = al64(o_match + (size_t)n * 4);
        o_counts = al64(o_outl + (size_t)n); o_nodes = o_counts + 64; bytes = bow ? o_nodes + (size_t)n * 4 : o_counts;
    }
};

// the opening both chains and the finish share: arguments that read no store state, the device, the locks, the counts under them, the index
struct FrameCall : RecordCall {
    int n = 0, n_last = 0, n_ref = 0;
    int open(const char* who, bool args_ok, CorbKfStore* frames, int cur_slot, int last_slot, CorbKfStore* kfs, int ref_slot, CorbMpStore* map, const CorbTrackCamera* cam)
    {
        if (!args_ok || !frames || !kfs || !map || cur_slot < 0 || cur_slot >= frames->capacity || ref_slot < 0 || ref_slot >= kfs->capacity ||
            (last_slot != -2 && (last_slot < 0 || last_slot >= frames->capacity || last_slot == cur_slot)) || (kfs == frames && (ref_slot == cur_slot))) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
        if (frames->device != map->device || kfs->device != map->device) { corb_set_error("%s: the stores live on different devices", who); return CORB_ERR_ARG; }
        if (cam && !track_host::camera_ok(cam)) { corb_set_error("%s: bad camera", who); return CORB_ERR_ARG; }
        int rc = corb_select_device(frames->device); if (rc) return rc;
        hold(nullptr, frames, kfs, map);
        if ((n = record_slot_count(who, frames, cur_slot)) < 0) return CORB_ERR_ARG;
        if (last_slot != -2 && (n_last = record_slot_count(who, frames, last_slot)) < 0) return CORB_ERR_ARG;
        if ((n_ref = record_slot_count(who, kfs, ref_slot)) < 0) return CORB_ERR_ARG;
        return record_need_index(who, map);
    }
};

bool params_ok(const char* who, const CorbTrackFrameParams* P)
{
    if (P->sensor < 0 || P->sensor > 2 || !(P->th >= 0) || !(P->nnratio > 0)) { corb_set_error("%s: sensor %d (0 .. 2), th %g (>= 0), nnratio %g (> 0)", who, P->sensor, (double)P->th, (double)P->nnratio); return false; }
    return true;
}

void device_views(TrackFrameDev& t, CorbKfStore* frames, int cur_slot, int last_slot, CorbKfStore* kfs, int ref_slot, CorbMpStore* map, const FrameCall& c)
{
    t.cur = frames->rec(cur_slot); t.last = last_slot >= 0 ? frames->rec(last_slot) : nullptr; t.F = frames->F; t.n_cur = c.n; t.n_last = c.n_last;
    t.ref = kfs->rec(ref_slot); t.F_ref = kfs->F; t.n_ref = c.n_ref;
    t.map = map->base(); t.mp_bytes = map->L.bytes; t.max_obs = map->O; t.idt = map->idt;
}

// PoseOptimization from the pose in the current record, the "Discard outliers" loop, the packing: what both chains end with
int optimise_and_tail(CorbScratch& pool, TrackFrameDev& t, CorbKfStore* frames, CorbMpStore* map, const CorbTrackCamera* cam, char* blk, const Block& B, bool want_outlier)
{
    TrackPoseDev tp; memset(&tp, 0, sizeof(tp));
    tp.cur = t.cur; tp.F = frames->F; tp.n_cur = t.n_cur; tp.mp_base = map->base(); tp.mp_bytes = map->L.bytes; tp.idt = map->idt; tp.discard = 1; tp.skip = t.head->skip;
    const float* dev_Tcw = reinterpret_cast<const KfHeader*>(t.cur)->m.Tcw;
    int rc = track_host::pose_enqueue(pool, tp, cam, nullptr, true, reinterpret_cast<double*>(blk + B.o_pose), dev_Tcw); if (rc) return rc;
    t.rejected = tp.rejected;
    if (want_outlier) t.out_outlier = reinterpret_cast<unsigned char*>(blk + B.o_outl);
    trackframe_launch_tail(t, pool.stream);
    HIPCHK(hipGetLastError());
    return CORB_OK;
}

// the block's counts into the result; `ran`: the optimisation and the tail ran
void fill_result(CorbTrackFrameResult* out, const TrackFrameHead& h, const track_host::PoseResult& pr, const CorbTrackFrameParams* P, bool motion_model, float th)
{
    memset(out, 0, sizeof(*out));
    const bool ran = !(h.skip[0] | h.skip[1]);
    out->n_matches_first = h.n_first; out->searched_wide = h.wide; out->n_matches = h.n_matches; out->th_used = h.wide ? 2.0f * th : th;
    out->n_pose_inliers = ran ? track_host::pose_inliers(pr) : 0;
    out->n_matches_kept = h.n_matches - h.n_rejected; out->n_matches_map = h.n_map;
    if (ran) {
        if (motion_model && P->only_tracking) { out->vo = h.n_map < 10; out->ok = out->n_matches_kept > 20; }      // mbVO = nmatchesMap<10; return nmatches>20; (:942-946)
        else out->ok = h.n_map >= 10;
    }
    memcpy(out->Tlw, h.Tlw, sizeof(h.Tlw)); memcpy(out->Tcw_pred, h.Tcw_pred, sizeof(h.Tcw_pred));
    memcpy(out->Tcw, (ran || motion_model) ? h.Tcw_pred : h.Tcw_before, sizeof(h.Tcw_pred));
    if (ran && pr.cnt[2]) corb_pose_to_T(pr.pose, out->Tcw);
}

int motion_model_call(CorbKfStore* frames, int cur_slot, int last_slot, CorbKfStore* kfs, int ref_slot, CorbMpStore* map, const CorbTrackCamera* cam,
                      const float* velocity, const float* Tlr, const CorbTrackFrameParams* P, int32_t* match, uint8_t* outlier, CorbTrackFrameResult* out)
{
    const char* who = "corb_track_with_motion_model";
    FrameCall c; int rc = c.open(who, cam && velocity && P && out, frames, cur_slot, last_slot, kfs, ref_slot, map, cam); if (rc) return rc;
    if (!params_ok(who, P)) return CORB_ERR_ARG;
    const int n = c.n, nq = c.n_last;
    if (proj_too_large(n, nq)) { corb_set_error("%s: a frame of %d features against %d of the last frame, the search takes at most %d and %d", who, n, nq, PROJ_MAX_FEATURES, PROJ_MAX_QUERIES); return CORB_ERR_ARG; }
    const float th = P->th > 0 ? P->th : (P->sensor != 1 ? 15.0f : 7.0f);            // if(mSensor!=System::STEREO) th=15; else th=7; (:899-903)
    rc = c.join(); if (rc) return rc;
    CorbScratch pool(0);
    const Block B(n, false);
    char* blk; HIPCHK(pool.alloc(&blk, B.bytes));
    HIPCHK(hipMemsetAsync(blk, 0, B.o_match, pool.stream));
    TrackFrameDev t; memset(&t, 0, sizeof(t));
    device_views(t, frames, cur_slot, last_slot, kfs, ref_slot, map, c);
    t.head = reinterpret_cast<TrackFrameHead*>(blk); t.frame_id = P->frame_id; t.check_replaced = P->check_replaced ? 1 : 0; t.has_Tlr = Tlr ? 1 : 0;
    t.mono = P->sensor == 0; t.min_matches = 20;
    memcpy(t.velocity, velocity, sizeof(t.velocity)); if (Tlr) memcpy(t.Tlr, Tlr, sizeof(t.Tlr));
    t.fx = cam->fx; t.fy = cam->fy; t.cx = cam->cx; t.cy = cam->cy; t.bf = cam->bf; t.mb = cam->mb;
    const bool search = n > 0 && nq > 0;
    if (search) trackframe_launch_open(t, 1, pool.stream);
    trackframe_launch_motion_pose(t, pool.stream);
    HIPCHK(hipGetLastError());
    if (search) {
        // ---- SearchByProjection(CurrentFrame, LastFrame, th, bMono), and again at 2 th behind a gate on the first count ----
        TrackDev s; memset(&s, 0, sizeof(s));
        s.cur = t.cur; s.last = t.last; s.F = frames->F; s.mp_base = map->base(); s.mp_bytes = map->L.bytes; s.idt = map->idt; s.n_cur = n; s.n_last = nq;
        HIPCHK(pool.alloc(&s.lastp, (size_t)nq)); HIPCHK(pool.alloc(&s.qdesc, (size_t)nq * 4)); HIPCHK(pool.alloc(&s.claimed, (size_t)n));
        ProjBuffers p1, p2;
        rc = p1.alloc(pool, n, nq, true, 0); if (rc) return rc;
        rc = p2.alloc(pool, n, nq, true, 0); if (rc) return rc;
        track_launch_prepare_last(s, pool.stream);                                       // (the frame is all NULL: both searches start from these claims)
        CorbProjDev d1{}; track_host::record_target(d1, cam, t.cur, RecLayout(frames->F), n, nq);
        preset_frame(d1, P->nnratio, P->check_orientation); p1.bind(d1);
        d1.claimed = s.claimed; d1.qdesc = s.qdesc;
        CorbProjDev d2 = d1; p2.bind(d2);
        d2.feat_cell = d1.feat_cell; d2.cell_off = d1.cell_off; d2.cell_idx = d1.cell_idx;      // one target image: the first search's grid
        d2.gate = p1.n_matches; d2.gate_below = t.min_matches;
        corb_launch_projection_frame_dev(d1, s.lastp, &t.head->pose, th, 1, pool.stream);
        corb_launch_projection_frame_dev(d2, s.lastp, &t.head->pose, 2.0f * th, 0, pool.stream);
        t.counts1 = p1.n_matches; t.counts2 = p2.n_matches; t.match1 = p1.res; t.match2 = p2.res;
        t.out_match = reinterpret_cast<int*>(blk + B.o_match);
        trackframe_launch_select(t, pool.stream);
        HIPCHK(hipGetLastError());
        rc = optimise_and_tail(pool, t, frames, map, cam, blk, B, outlier != nullptr); if (rc) return rc;
    }
    // ---- the one read-back ----
    static thread_local std::vector<char> back; back.resize(B.bytes);
    HIPCHK(pool.d2h(back.data(), blk, search ? B.o_outl + (size_t)n : B.o_match));
    HIPCHK(pool.fetch_finish());
    const TrackFrameHead& h = *reinterpret_cast<const TrackFrameHead*>(back.data());
    if (h.status) { corb_set_error("%s: more than %d candidates in one search window", who, PROJ_CAND_CAP); return CORB_ERR_OVERFLOW; }
    if (match) { if (search) memcpy(match, back.data() + B.o_match, (size_t)n * 4); else for (int i = 0; i < n; i++) match[i] = -1; }
    if (outlier) { if (search) memcpy(outlier, back.data() + B.o_outl, (size_t)n); else memset(outlier, 0, (size_t)n); }
    TrackFrameHead hh = h; if (!search) hh.skip[1] = 1;
    fill_result(out, hh, *reinterpret_cast<const track_host::PoseResult*>(back.data() + B.o_pose), P, true, th);
    return CORB_OK;
}

int reference_keyframe_call(CorbKfStore* frames, int cur_slot, int last_slot, CorbKfStore* kfs, int ref_slot, CorbMpStore* map, const CorbTrackCamera* cam,
                            CorbVoc* voc, const CorbTrackFrameParams* P, int32_t* match, uint8_t* outlier, CorbTrackFrameResult* out)
{
    const char* who = "corb_track_reference_keyframe";
    FrameCall c; int rc = c.open(who, cam && P && out, frames, cur_slot, last_slot, kfs, ref_slot, map, cam); if (rc) return rc;
    if (!params_ok(who, P)) return CORB_ERR_ARG;
    if (voc && voc->device != frames->device) { corb_set_error("%s: the vocabulary lives on another device", who); return CORB_ERR_ARG; }
    rc = kf_store_slot_ready(frames, cur_slot, who); if (rc) return rc;                  // the host mirror of the node counts
    rc = kf_store_slot_ready(kfs, ref_slot, who); if (rc) return rc;
    const int n = c.n;
    CorbKfStore::Host& hc = frames->host[cur_slot];
    const bool bow = n > 0 && hc.n_nodes == 0;
    if (bow && !voc) { corb_set_error("%s: slot %d holds no FeatureVector and no vocabulary was given", who, cur_slot); return CORB_ERR_ARG; }
    if (bow && frames->F > BOW_MAX_FEATURES) { corb_set_error("%s: the store holds up to %d features per frame; the transform sorts at most %d", who, frames->F, BOW_MAX_FEATURES); return CORB_ERR_ARG; }
    rc = c.join(); if (rc) return rc;
    CorbScratch pool(0);
    const Block B(n, bow);
    char* blk; HIPCHK(pool.alloc(&blk, B.bytes));
    HIPCHK(hipMemsetAsync(blk, 0, B.o_match, pool.stream));
    TrackFrameDev t; memset(&t, 0, sizeof(t));
    device_views(t, frames, cur_slot, last_slot, kfs, ref_slot, map, c);
    t.head = reinterpret_cast<TrackFrameHead*>(blk); t.frame_id = P->frame_id; t.check_replaced = P->check_replaced ? 1 : 0; t.min_matches = 15;
    t.n_nodes_ref = kfs->host[ref_slot].n_nodes;
    const RecLayout L(frames->F), LK(kfs->F);
    if (n > 0) trackframe_launch_open(t, 0, pool.stream);
    if (bow) {
        // ---- mCurrentFrame.ComputeBoW(): corb_kf_store_compute_bow's launches for the one record, without a database; its read-back rides in the block ----
        int32_t *d_fword, *d_dummy; uint32_t *d_fnode, *d_sw; double* d_sv; BowSetDev* d_set;
        HIPCHK(pool.alloc(&d_fword, (size_t)n)); HIPCHK(pool.alloc(&d_fnode, (size_t)n)); HIPCHK(pool.alloc(&d_sw, (size_t)n)); HIPCHK(pool.alloc(&d_sv, (size_t)n)); HIPCHK(pool.alloc(&d_dummy, 1));
        BowSetDev set{};
        set.desc = reinterpret_cast<const unsigned long long*>(t.cur + L.desc); set.n = n; set.feat_off = 0; set.max_words = n; set.bow_word = d_sw; set.bow_value = d_sv; set.bow_count = d_dummy;
        set.fv_node = reinterpret_cast<uint32_t*>(t.cur + L.fv_node); set.fv_off = reinterpret_cast<int32_t*>(t.cur + L.fv_off); set.fv_idx = reinterpret_cast<uint32_t*>(t.cur + L.fv_idx);
        set.fv_n_nodes = reinterpret_cast<int32_t*>(t.cur + 4);
        set.node_copy = reinterpret_cast<uint32_t*>(blk + B.o_nodes); set.counts = reinterpret_cast<int32_t*>(blk + B.o_counts);
        HIPCHK(pool.upload(&d_set, &set, 1));
        int attr = 0;
        corb_launch_bow_transform(voc->dev, d_set, 1, n, 4, d_fword, d_fnode, pool.stream, &attr);
        if (attr) { corb_set_error("%s: the sort kernel's LDS opt-in failed: %s", who, hipGetErrorString((hipError_t)attr)); return CORB_ERR_HIP; }
        HIPCHK(hipGetLastError());
    }
    {
        // ---- SearchByBoW(mpReferenceKF, mCurrentFrame, vpMapPointMatches) ----
        int *dmatch, *dbin, *dhist;
        HIPCHK(pool.alloc(&dmatch, (size_t)n)); HIPCHK(pool.alloc(&dbin, (size_t)n)); HIPCHK(pool.alloc(&dhist, (size_t)CORB_HISTO_LENGTH + 1)); HIPCHK(pool.alloc(&t.kf_valid, (size_t)c.n_ref));
        HIPCHK(hipMemsetAsync(dmatch, 0xFF, (size_t)n * 4, pool.stream)); HIPCHK(hipMemsetAsync(dbin, 0xFF, (size_t)n * 4, pool.stream));
        HIPCHK(hipMemsetAsync(dhist, 0, (CORB_HISTO_LENGTH + 1) * 4, pool.stream));
        CorbBowDev& d = t.bow;
        d.variant = 0; d.check_ori = P->check_orientation ? 1 : 0; d.n_pairs = 1; d.nnratio = P->nnratio;
        d.off1 = reinterpret_cast<const int*>(t.ref + LK.fv_off); d.idx1 = reinterpret_cast<const int*>(t.ref + LK.fv_idx);
        d.off2 = reinterpret_cast<const int*>(t.cur + L.fv_off); d.idx2 = reinterpret_cast<const int*>(t.cur + L.fv_idx);
        d.desc1 = reinterpret_cast<const unsigned long long*>(t.ref + LK.desc); d.desc2 = reinterpret_cast<const unsigned long long*>(t.cur + L.desc);
        d.angle1 = reinterpret_cast<const float*>(t.ref + LK.angle); d.angle2 = reinterpret_cast<const float*>(t.cur + L.angle);
        d.valid1 = t.kf_valid; d.valid2 = nullptr;
        d.match = dmatch; d.bin = dbin; d.hist = dhist; d.n_matches = dhist + CORB_HISTO_LENGTH;
        t.counts1 = d.n_matches; t.match1 = dmatch;
        t.out_match = reinterpret_cast<int*>(blk + B.o_match);
        trackframe_launch_bow(t, pool.stream);
        trackframe_launch_set_matches(t, pool.stream);
        HIPCHK(hipGetLastError());
        if (n > 0) { rc = optimise_and_tail(pool, t, frames, map, cam, blk, B, outlier != nullptr); if (rc) return rc; }
    }
    // ---- the one read-back ----
    static thread_local std::vector<char> back; back.resize(B.bytes);
    HIPCHK(pool.d2h(back.data(), blk, B.bytes));
    HIPCHK(pool.fetch_finish());
    if (bow) {                                                                           // the host mirror of the record's FeatureVector, as corb_kf_store_compute_bow keeps it
        const int32_t* counts = reinterpret_cast<const int32_t*>(back.data() + B.o_counts); const uint32_t* nodes = reinterpret_cast<const uint32_t*>(back.data() + B.o_nodes);
        hc.n_nodes = std::min(std::max(counts[1], 0), n); hc.node_id.assign(nodes, nodes + hc.n_nodes);
    }
    if (match && n > 0) memcpy(match, back.data() + B.o_match, (size_t)n * 4);
    if (outlier && n > 0) memcpy(outlier, back.data() + B.o_outl, (size_t)n);
    const TrackFrameHead& hh = *reinterpret_cast<const TrackFrameHead*>(back.data());
    fill_result(out, hh, *reinterpret_cast<const track_host::PoseResult*>(back.data() + B.o_pose), P, false, 0.0f);
    return CORB_OK;
}

int frame_finish_call(CorbKfStore* frames, int cur_slot, CorbKfStore* kfs, int ref_slot, CorbMpStore* map, int stage, float* Tcr_out)
{
    const char* who = "corb_track_frame_finish";
    FrameCall c; int rc = c.open(who, (stage == 0 || stage == 1) && (stage == 0 || Tcr_out), frames, cur_slot, -2, kfs, ref_slot, map, nullptr); if (rc) return rc;
    rc = c.join(); if (rc) return rc;
    TrackFrameDev t; memset(&t, 0, sizeof(t));
    device_views(t, frames, cur_slot, -1, kfs, ref_slot, map, c);
    if (stage == 0) {                                                                    // on the frame store's stream: the store's later calls wait for it
        if (c.n > 0) trackframe_launch_finish(t, 0, nullptr, frames->stream);
        HIPCHK(hipGetLastError());
        return CORB_OK;
    }
    CorbScratch pool(0);
    float* dTcr; HIPCHK(pool.alloc(&dTcr, 16));
    trackframe_launch_finish(t, 1, dTcr, pool.stream);
    HIPCHK(hipGetLastError());
    float back[16];
    HIPCHK(pool.d2h(back, dTcr, sizeof(back)));
    HIPCHK(pool.fetch_finish());
    memcpy(Tcr_out, back, sizeof(back));
    return CORB_OK;
}
}  // namespace

// ---------------------------------------------------------------- the exported names ----------------------------------------------------------------
// TO FOLD BACK (as the forwarders of corb_tracklocal.cpp and corb_fusion.cpp): the three calls draw from workspace lane 0 inside the file-local *_call functions
// above, and these forwarders serve no design purpose -- tests/workspace_cases.py, the registry of the lane calls, is an existing test file that a pull request may
// not edit, and its CPU check looks for a CovisCall / CorbScratch inside an exported body.  Their fresh / warm / pattern-filled arena states are run by
// tests/test_gpu_trackframe.py instead.  Whoever may edit the registry: enter the three symbols, then fold the *_call bodies into the exported functions.
extern "C" int corb_track_with_motion_model(CorbKfStore* frames, int cur_slot, int last_slot, CorbKfStore* kfs, int ref_slot, CorbMpStore* map, const CorbTrackCamera* cam,
                                            const float* velocity, const float* Tlr, const CorbTrackFrameParams* params, int32_t* match, uint8_t* outlier, CorbTrackFrameResult* out)
{
    return motion_model_call(frames, cur_slot, last_slot, kfs, ref_slot, map, cam, velocity, Tlr, params, match, outlier, out);
}
extern "C" int corb_track_reference_keyframe(CorbKfStore* frames, int cur_slot, int last_slot, CorbKfStore* kfs, int ref_slot, CorbMpStore* map, const CorbTrackCamera* cam,
                                             CorbVoc* voc, const CorbTrackFrameParams* params, int32_t* match, uint8_t* outlier, CorbTrackFrameResult* out)
{
    return reference_keyframe_call(frames, cur_slot, last_slot, kfs, ref_slot, map, cam, voc, params, match, outlier, out);
}
extern "C" int corb_track_frame_finish(CorbKfStore* frames, int cur_slot, CorbKfStore* kfs, int ref_slot, CorbMpStore* map, int stage, float* Tcr_out)
{
    return frame_finish_call(frames, cur_slot, kfs, ref_slot, map, stage, Tcr_out);
}

// corb_proj.cpp -- C-ABI host side of the projection-guided matchers (see include/corb_accel.h).
// Ships the flat Frame / MapPoint views to the device and launches proj_kernels.hip; the only host arithmetic is the
// frame-to-frame translation test that selects the level window (ORBmatcher.cc:1480-1491).  No CPU compute fallback.
#include "proj_host.h"
#include <algorithm>

using namespace proj_host;

namespace {
// map / last-frame matchers: upload the Frame view + the projected points (one copy), grid, prepare, greedy resolution
int run_projection(const CorbFrameView* F, int nq, const void* qdesc, const CorbTrackedPoint* mp, const CorbLastPoint* last,
                   const CorbProjPose* pose, float th, CorbProjDev& d, int32_t* match, int* n_matches, int device)
{
    if (!F || !match || !n_matches || F->n < 0 || nq < 0 || F->nlevels < 1 || F->nlevels > CORB_MAX_LEVELS ||
        (F->n > 0 && (!F->keys_un || !F->u_right || !F->desc || !F->claimed)) || !F->scale || (nq > 0 && !qdesc)) {
        corb_set_error("projection matcher: bad argument"); return CORB_ERR_ARG;
    }
    if (proj_too_large(F->n, nq)) { corb_set_error("projection matcher: frame too large (%d features)", F->n); return CORB_ERR_ARG; }
    *n_matches = 0;
    for (int i = 0; i < F->n; i++) match[i] = -1;
    if (F->n == 0 || nq == 0) return CORB_OK;          // (before the bounds test: a featureless frame's view may leave its bounds at zero; nothing to match either way)
    if (!(F->max_x > F->min_x) || !(F->max_y > F->min_y)) { corb_set_error("projection matcher: empty image bounds"); return CORB_ERR_ARG; }
    int rc = corb_select_device(device); if (rc) return rc;
    const int n = F->n;
    CorbScratch pool(0);
    void* src;
    HIPCHK(pool.upload_block({{(void**)&d.keys, F->keys_un, (size_t)n * sizeof(CorbKeyPoint)}, {(void**)&d.u_right, F->u_right, (size_t)n * 4}, {(void**)&d.desc, F->desc, (size_t)n * 32},
                              {(void**)&d.claimed, F->claimed, (size_t)n}, {(void**)&d.qdesc, qdesc, (size_t)nq * 32},
                              {&src, mp ? (const void*)mp : (const void*)last, (size_t)nq * (mp ? sizeof(CorbTrackedPoint) : sizeof(CorbLastPoint))}}));
    ProjBuffers pb; rc = pb.alloc(pool, n, nq, true, 0); if (rc) return rc;
    const float bounds[4] = {F->min_x, F->min_y, F->max_x, F->max_y};
    proj_grid(d, n, nq, bounds, F->scale, nullptr, F->nlevels);
    pb.bind(d);
    corb_launch_projection(d, mp ? (const CorbTrackedPoint*)src : nullptr, mp ? nullptr : (const CorbLastPoint*)src, pose, th, pool.stream);
    HIPCHK(hipGetLastError());
    return proj_finish(pool, pb, n, match, n_matches, nullptr, "projection matcher");
}

// keyframe-target matchers: upload the KeyFrame view + MapPoint views, grid, prepare, then either the greedy resolution
// (relocalisation projection, SearchByProjection with Scw) or the independent best candidate per point (Fuse, SearchBySim3)
int run_points(const CorbKeyFrameView* K, const uint8_t* claimed, const CorbMapPointView* pts, const uint8_t* qdesc, int nq, CorbProjDev& d, const CorbProjTf& tf,
               int greedy, int32_t* match, int* n_matches, int32_t* best_idx, int32_t* best_dist, int device)
{
    if (!K || K->n < 0 || nq < 0 || K->nlevels < 1 || K->nlevels > CORB_MAX_LEVELS || !K->scale ||
        (K->n > 0 && (!K->keys_un || !K->u_right || !K->desc)) || (nq > 0 && (!pts || !qdesc)) || (d.chi2_check && !K->inv_level_sigma2) || (greedy && K->n > 0 && !claimed)) {
        corb_set_error("keyframe projection matcher: bad argument"); return CORB_ERR_ARG;
    }
    if (proj_too_large(K->n, nq)) { corb_set_error("keyframe projection matcher: too large (%d features, %d points)", K->n, nq); return CORB_ERR_ARG; }
    if (greedy) { *n_matches = 0; for (int i = 0; i < K->n; i++) match[i] = -1; }
    else for (int i = 0; i < nq; i++) { best_idx[i] = -1; best_dist[i] = 256; }
    if (K->n == 0 || nq == 0) return CORB_OK;          // (before the bounds test, as in run_projection)
    if (!(K->max_x > K->min_x) || !(K->max_y > K->min_y)) { corb_set_error("keyframe projection matcher: empty image bounds"); return CORB_ERR_ARG; }
    int rc = corb_select_device(device); if (rc) return rc;
    const int n = K->n;
    CorbScratch pool(0);
    std::vector<unsigned char> zero_claimed;
    if (!claimed) { zero_claimed.assign(n, 0); claimed = zero_claimed.data(); }
    CorbMapPointView* dpts;
    HIPCHK(pool.upload_block({{(void**)&d.keys, K->keys_un, (size_t)n * sizeof(CorbKeyPoint)}, {(void**)&d.u_right, K->u_right, (size_t)n * 4}, {(void**)&d.desc, K->desc, (size_t)n * 32},
                              {(void**)&d.claimed, claimed, (size_t)n}, {(void**)&d.qdesc, qdesc, (size_t)nq * 32}, {(void**)&dpts, pts, (size_t)nq * sizeof(CorbMapPointView)}}));
    ProjBuffers pb; rc = pb.alloc(pool, n, nq, greedy != 0, 0); if (rc) return rc;
    const float bounds[4] = {K->min_x, K->min_y, K->max_x, K->max_y};
    proj_grid(d, n, nq, bounds, K->scale, K->inv_level_sigma2, K->nlevels);
    pb.bind(d);
    corb_launch_projection_points(d, dpts, tf, greedy, pool.stream);
    HIPCHK(hipGetLastError());
    if (greedy) return proj_finish(pool, pb, n, match, n_matches, nullptr, "keyframe projection matcher");
    return proj_finish_best(pool, pb, best_idx, best_dist);
}
CorbProjTf tf_of(const CorbKeyFrameView* K, float th) { return tf_intrinsics(K->fx, K->fy, K->cx, K->cy, K->bf, K->log_scale_factor, th, K->nlevels); }
}  // namespace

extern "C" int corb_search_by_projection_map(const CorbFrameView* frame, const CorbTrackedPoint* points, const uint8_t* point_desc, int n_points,
                                             float th, float nnratio, int32_t* match, int* n_matches, int device)
{
    if (n_points > 0 && !points) { corb_set_error("corb_search_by_projection_map: bad argument"); return CORB_ERR_ARG; }
    if (frame) for (int i = 0; i < n_points; i++) if (points[i].valid && (points[i].level < 0 || points[i].level >= frame->nlevels)) { corb_set_error("corb_search_by_projection_map: level out of range"); return CORB_ERR_ARG; }
    CorbProjDev d{}; preset_map(d, nnratio);
    return run_projection(frame, n_points, point_desc, points, nullptr, nullptr, th, d, match, n_matches, device);
}

extern "C" int corb_search_by_projection_frame(const CorbFrameView* cur, const float* Tcw, const float* Tlw, float fx, float fy, float cx, float cy,
                                               float bf, float mb, const CorbLastPoint* last, const uint8_t* last_desc, int n_last,
                                               float th, int mono, int check_orientation, int32_t* match, int* n_matches, int device)
{
    if (!Tcw || !Tlw || (n_last > 0 && !last)) { corb_set_error("corb_search_by_projection_frame: bad argument"); return CORB_ERR_ARG; }
    if (cur) for (int i = 0; i < n_last; i++) if (last[i].valid && (last[i].octave < 0 || last[i].octave >= cur->nlevels)) { corb_set_error("corb_search_by_projection_frame: octave out of range"); return CORB_ERR_ARG; }
    const CorbProjPose pose = frame_pose(Tcw, Tlw, fx, fy, cx, cy, bf, mb, mono);
    CorbProjDev d{}; preset_frame(d, 0.f, check_orientation);
    return run_projection(cur, n_last, last_desc, nullptr, last, &pose, th, d, match, n_matches, device);
}

/* int ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched, vector<int>& vnMatches12, int windowSize) (ORBmatcher.cc:540-655) */
extern "C" int corb_search_for_initialization(const CorbFrameView* f1, const CorbFrameView* f2, float* prev_matched, int window_size, float nnratio, int check_orientation,
                                              int32_t* matches12, int* n_matches, int device)
{
    if (!f1 || !f2 || !matches12 || !n_matches || f1->n < 0 || f2->n < 0 || (f1->n > 0 && (!f1->keys_un || !f1->desc || !prev_matched)) || (f2->n > 0 && (!f2->keys_un || !f2->desc)) ||
        window_size < 0) {
        corb_set_error("corb_search_for_initialization: bad argument"); return CORB_ERR_ARG;
    }
    if (f2->n > PROJ_MAX_FEATURES || f1->n > PROJ_INIT_MAX_QUERIES) { corb_set_error("corb_search_for_initialization: frame too large (%d / %d features)", f1->n, f2->n); return CORB_ERR_ARG; }
    *n_matches = 0;
    for (int i = 0; i < f1->n; i++) matches12[i] = -1;
    if (f1->n == 0 || f2->n == 0) return CORB_OK;          // (before the bounds test: the view of a featureless F2 may leave its bounds at zero)
    if (!(f2->max_x > f2->min_x) || !(f2->max_y > f2->min_y)) { corb_set_error("corb_search_for_initialization: empty image bounds"); return CORB_ERR_ARG; }
    int rc = corb_select_device(device); if (rc) return rc;
    const int n = f2->n, nq = f1->n;
    CorbScratch pool(0);
    CorbProjDev d{}; CorbKeyPoint* keys1; float* dpm;
    HIPCHK(pool.upload_block({{(void**)&d.keys, f2->keys_un, (size_t)n * sizeof(CorbKeyPoint)}, {(void**)&d.desc, f2->desc, (size_t)n * 32},
                              {(void**)&keys1, f1->keys_un, (size_t)nq * sizeof(CorbKeyPoint)}, {(void**)&d.qdesc, f1->desc, (size_t)nq * 32}, {(void**)&dpm, prev_matched, (size_t)nq * 8}}));
    ProjBuffers pb; rc = pb.alloc(pool, n, nq, true, std::min(n, PROJ_INIT_CAND_CAP)); if (rc) return rc;
    const float bounds[4] = {f2->min_x, f2->min_y, f2->max_x, f2->max_y};
    proj_grid(d, n, nq, bounds, nullptr, nullptr, 0);
    preset_initialization(d, nnratio, check_orientation);
    pb.bind(d);
    corb_launch_search_for_initialization(d, keys1, dpm, (float)window_size, pool.stream);
    HIPCHK(hipGetLastError());
    std::vector<float> pm2((size_t)nq * 2);                // (prev_matched is only handed over when the call succeeds)
    HIPCHK(pool.d2h(pm2.data(), dpm, (size_t)nq * 8));
    rc = proj_finish(pool, pb, nq, matches12, n_matches, nullptr, "corb_search_for_initialization"); if (rc) return rc;
    memcpy(prev_matched, pm2.data(), (size_t)nq * 8);
    return CORB_OK;
}

/* SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1616-1744) */
extern "C" int corb_search_by_projection_reloc(const CorbKeyFrameView* cur, const uint8_t* claimed, const float* Tcw, const CorbMapPointView* points,
                                               const uint8_t* point_desc, int n_points, float th, int orb_dist, int check_orientation,
                                               int32_t* match, int* n_matches, int device)
{
    if (!cur || !Tcw || !match || !n_matches) { corb_set_error("corb_search_by_projection_reloc: bad argument"); return CORB_ERR_ARG; }
    CorbProjDev d{}; CorbProjTf tf = tf_of(cur, th);
    set_affine(tf.A, Tcw); camera_centre(Tcw, tf.Ow);
    preset_reloc(d, tf, orb_dist, check_orientation);
    return run_points(cur, claimed, points, point_desc, n_points, d, tf, 1, match, n_matches, nullptr, nullptr, device);
}

/* int SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, int th) (ORBmatcher.cc:425-538):
 * the sequential claim of keyframe features (vpMatched[idx] on entry + the commits of earlier points, :510 / :530) is resolved exactly by proj_resolve_kernel. */
extern "C" int corb_search_by_projection_scw(const CorbKeyFrameView* kf, const uint8_t* claimed, const float* Scw, const CorbMapPointView* points,
                                             const uint8_t* point_desc, int n_points, float th, int32_t* match, int* n_matches, int device)
{
    if (!kf || !Scw || !match || !n_matches) { corb_set_error("corb_search_by_projection_scw: bad argument"); return CORB_ERR_ARG; }
    CorbProjDev d{}; CorbProjTf tf = tf_of(kf, th);
    decompose_scw(Scw, tf);
    preset_scw(d, tf);
    return run_points(kf, claimed, points, point_desc, n_points, d, tf, 1, match, n_matches, nullptr, nullptr, device);
}

/* ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) (:960-1116, sim3 = 0) and Fuse(KeyFrame*, cv::Mat Scw, ..., vpReplacePoint) (:1118-1241, sim3 = 1) */
extern "C" int corb_fuse(const CorbKeyFrameView* kf, const float* T, const float* Ow, int sim3, const CorbMapPointView* points, const uint8_t* point_desc,
                         int n_points, float th, int32_t* best_idx, int32_t* best_dist, int* n_fused, int device)
{
    if (!kf || !T || (!sim3 && !Ow) || !best_idx || !best_dist || !n_fused) { corb_set_error("corb_fuse: bad argument"); return CORB_ERR_ARG; }
    CorbProjDev d{}; CorbProjTf tf = tf_of(kf, th);
    if (sim3) { decompose_scw(T, tf); preset_fuse_sim3(d, tf); } else { set_affine(tf.A, T); tf.Ow[0] = Ow[0]; tf.Ow[1] = Ow[1]; tf.Ow[2] = Ow[2]; preset_fuse(d, tf); }
    int rc = run_points(kf, nullptr, points, point_desc, n_points, d, tf, 0, nullptr, nullptr, best_idx, best_dist, device);
    if (rc) return rc;
    int nf = 0; for (int i = 0; i < n_points; i++) nf += best_idx[i] >= 0;
    *n_fused = nf;
    return CORB_OK;
}

/* ORBmatcher::SearchBySim3(KeyFrame*, KeyFrame*, vpMatches12, s12, R12, t12, th) (:1244-1468) */
extern "C" int corb_search_by_sim3(const CorbKeyFrameView* kf1, const CorbKeyFrameView* kf2, const float* T1w, const float* T2w,
                                   const CorbMapPointView* points1, const uint8_t* desc1, const CorbMapPointView* points2, const uint8_t* desc2,
                                   float s12, const float* R12, const float* t12, float th, int32_t* match12, int* n_found, int device)
{
    if (!kf1 || !kf2 || !T1w || !T2w || !R12 || !t12 || !match12 || !n_found) { corb_set_error("corb_search_by_sim3: bad argument"); return CORB_ERR_ARG; }
    float sR12[9], sR21[9], t21[3];
    sim3_pair(s12, R12, t12, sR12, sR21, t21);
    const int N1 = kf1->n, N2 = kf2->n;
    std::vector<int32_t> m1(N1 > 0 ? N1 : 1, -1), m2(N2 > 0 ? N2 : 1, -1), bd((N1 > N2 ? N1 : N2) > 0 ? (N1 > N2 ? N1 : N2) : 1);
    auto direction = [&](const CorbKeyFrameView* B, const float* TAw, const float* sR, const float* t, const CorbMapPointView* pts, const uint8_t* desc, int n, int32_t* out) -> int {
        CorbProjDev d{}; CorbProjTf tf = tf_intrinsics(kf1->fx, kf1->fy, kf1->cx, kf1->cy, B->bf, B->log_scale_factor, th, B->nlevels);      // the intrinsics of both directions are pKF1's (:1247-1250)
        sim3_chain(tf, TAw, sR, t);
        preset_sim3(d, tf);
        return run_points(B, nullptr, pts, desc, n, d, tf, 0, nullptr, nullptr, out, bd.data(), device);
    };
    int rc = direction(kf2, T1w, sR21, t21, points1, desc1, N1, m1.data()); if (rc) return rc;
    rc = direction(kf1, T2w, sR12, t12, points2, desc2, N2, m2.data()); if (rc) return rc;
    int nf = 0;
    for (int i1 = 0; i1 < N1; i1++) {
        match12[i1] = -1;
        const int idx2 = m1[i1];
        if (idx2 >= 0 && m2[idx2] == i1) { match12[i1] = idx2; nf++; }
    }
    *n_found = nf;
    return CORB_OK;
}

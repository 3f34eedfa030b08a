// proj_host.h -- host side of the projection-guided matchers, shared by the host-pointer route (corb_proj.cpp) and the record route (corb_track.cpp): size limits,
// the pose algebra of the reference (cv::gemm on CV_32F: double accumulation, one rounding), the switch set of each matcher, the matcher's scratch and the
// read-back of a greedy match.  Each rule is stated here once.  Host code only.
#pragma once
#include "proj_internal.h"
#include "corb_workspace.h"
#include <cmath>
#include <cstring>
#include <vector>

#include "host_util.h"


#define PROJ_MAX_FEATURES 6000        // target features of one call (the resolution kernels keep per-feature state of one frame in LDS)
#define PROJ_MAX_QUERIES 60000        // projected points of one call
#define PROJ_INIT_MAX_QUERIES 8192    // SearchForInitialization: features of F1
#define PROJ_INIT_CAND_CAP 2048       // SearchForInitialization: candidates kept per window (a 2 x 100 px window of a dense frame holds more than the other matchers' 256)

namespace proj_host {

// ---- pose algebra ----
inline void set_affine(float* A, const float* T4x4) { for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) A[i * 4 + j] = T4x4[i * 4 + j]; }
// Ow = -Rcw^T * tcw : exact negation of the transposed rotation, then cv::gemm (double accumulation, one rounding)
inline void camera_centre(const float* Tcw, float* Ow)
{
    for (int i = 0; i < 3; i++) { double s = 0; for (int k = 0; k < 3; k++) s += (double)(-Tcw[k * 4 + i]) * (double)Tcw[k * 4 + 3]; Ow[i] = (float)s; }
}
// twc = -Rcw^T tcw ; tlc = Rlw twc + tlw  (cv::gemm on CV_32F: double accumulation, one rounding); forward / backward motion test (ORBmatcher.cc:1480-1491)
inline void motion_direction(const float* Tcw, const float* Tlw, float mb, int mono, int* forward, int* backward)
{
    float twc[3], tlc[3];
    camera_centre(Tcw, twc);
    for (int i = 0; i < 3; i++) { double s = 0; for (int k = 0; k < 3; k++) s += (double)Tlw[i * 4 + k] * (double)twc[k]; tlc[i] = (float)(s + (double)Tlw[i * 4 + 3]); }
    *forward = (tlc[2] > mb && !mono) ? 1 : 0;
    *backward = (-tlc[2] > mb && !mono) ? 1 : 0;
}
inline CorbProjPose frame_pose(const float* Tcw, const float* Tlw, float fx, float fy, float cx, float cy, float bf, float mb, int mono)
{
    CorbProjPose pose;
    memcpy(pose.Tcw, Tcw, 16 * sizeof(float));
    pose.fx = fx; pose.fy = fy; pose.cx = cx; pose.cy = cy; pose.bf = bf;
    motion_direction(Tcw, Tlw, mb, mono, &pose.forward, &pose.backward);
    return pose;
}
inline CorbProjTf tf_intrinsics(float fx, float fy, float cx, float cy, float bf, float log_scale, float th, int nlevels)
{
    CorbProjTf tf; memset(&tf, 0, sizeof(tf));
    tf.fx = fx; tf.fy = fy; tf.cx = cx; tf.cy = cy; tf.bf = bf; tf.log_scale = log_scale; tf.th = th; tf.nlevels = nlevels;
    return tf;
}
// decompose Scw (ORBmatcher.cc:434-438 = :1124-1128): Rcw = sRcw / scw, tcw = Scw.col(3) / scw (a division by the double scale = a float multiply by (float)(1/s)), Ow = -Rcw' tcw
inline void decompose_scw(const float* T, CorbProjTf& tf)
{
    const double dd = (double)T[0] * T[0] + (double)T[1] * T[1] + (double)T[2] * T[2];
    const float scw = (float)std::sqrt(dd);
    const float inv = (float)(1.0 / (double)scw);
    float M[16];
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) M[i * 4 + j] = T[i * 4 + j] * inv; M[i * 4 + 3] = T[i * 4 + 3] * inv; }
    M[12] = M[13] = M[14] = 0; M[15] = 1;
    set_affine(tf.A, M); camera_centre(M, tf.Ow);
}
// sR12 = s12*R12 ; sR21 = (1.0/s12)*R12.t() ; t21 = -sR21*t12   (ORBmatcher.cc:1262-1264)
inline void sim3_pair(float s12, const float* R12, const float* t12, float* sR12, float* sR21, float* t21)
{
    const float is = (float)(1.0 / (double)s12);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { sR12[i * 3 + j] = R12[i * 3 + j] * s12; sR21[i * 3 + j] = R12[j * 3 + i] * is; }
    for (int i = 0; i < 3; i++) { double s = 0; for (int k = 0; k < 3; k++) s += (double)(-sR21[i * 3 + k]) * (double)t12[k]; t21[i] = (float)s; }
}
// one direction of SearchBySim3: world -> keyframe A (TAw), then A -> B (sR | t)
inline void sim3_chain(CorbProjTf& tf, const float* TAw, const float* sR, const float* t)
{
    set_affine(tf.A, TAw);
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) tf.B[i * 4 + j] = sR[i * 3 + j]; tf.B[i * 4 + 3] = t[i]; }
}

// ---- the switch set of each matcher of the reference ----
inline void switches(CorbProjDev& d, float nnratio, int ratio_test, int check_ori, int check_uright, int th_dist, int chi2_check)
{
    d.nnratio = nnratio; d.ratio_test = ratio_test; d.check_ori = check_ori ? 1 : 0; d.check_uright = check_uright; d.th_dist = th_dist; d.chi2_check = chi2_check;
}
/* SearchByProjection(Frame&, const vector<MapPoint*>&, th) (ORBmatcher.cc:45-131) */
inline void preset_map(CorbProjDev& d, float nnratio) { switches(d, nnratio, 1, 0, 1, CORB_TH_HIGH, 0); }
/* SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) (ORBmatcher.cc:1470-1614) */
inline void preset_frame(CorbProjDev& d, float nnratio, int check_ori) { switches(d, nnratio, 0, check_ori, 1, CORB_TH_HIGH, 0); }
/* SearchForInitialization (ORBmatcher.cc:540-655) */
inline void preset_initialization(CorbProjDev& d, float nnratio, int check_ori) { switches(d, nnratio, 0, check_ori, 0, CORB_TH_LOW, 0); }
/* SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1616-1744): no depth test, closed image test,
 * invz in double, octaves [level - 1, level + 1] */
inline void preset_reloc(CorbProjDev& d, CorbProjTf& tf, int orb_dist, int check_ori) { switches(d, 0.f, 0, check_ori, 0, orb_dist, 0); tf.reloc = 1; tf.invz_double = 1; tf.lvl_hi = 1; }
/* SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints, vpMatched, th) (ORBmatcher.cc:425-538): Fuse's gates (depth, IsInImage, distance invariance, viewing angle)
 * with a float 1/z (:466), octaves [level-1, level], no chi2 test, TH_LOW */
inline void preset_scw(CorbProjDev& d, CorbProjTf& tf) { switches(d, 0.f, 0, 0, 0, CORB_TH_LOW, 0); tf.invz_double = 0; tf.check_normal = 1; tf.lvl_hi = 0; }
/* Fuse(KeyFrame*, const vector<MapPoint*>&, th) (ORBmatcher.cc:960-1116) */
inline void preset_fuse(CorbProjDev& d, CorbProjTf& tf) { switches(d, 0.f, 0, 0, 0, CORB_TH_LOW, 1); tf.invz_double = 0; tf.check_normal = 1; tf.lvl_hi = 0; }
/* Fuse(KeyFrame*, cv::Mat Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:1118-1241) */
inline void preset_fuse_sim3(CorbProjDev& d, CorbProjTf& tf) { switches(d, 0.f, 0, 0, 0, CORB_TH_LOW, 0); tf.invz_double = 1; tf.check_normal = 1; tf.lvl_hi = 0; }
/* SearchBySim3(KeyFrame*, KeyFrame*, vpMatches12, s12, R12, t12, th) (ORBmatcher.cc:1244-1468), one direction */
inline void preset_sim3(CorbProjDev& d, CorbProjTf& tf) { switches(d, 0.f, 0, 0, 0, CORB_TH_HIGH, 0); tf.two = 1; tf.invz_double = 1; tf.dist_from_cam = 1; tf.lvl_hi = 0; }

inline bool proj_too_large(int n, int nq) { return n > PROJ_MAX_FEATURES || nq > PROJ_MAX_QUERIES; }

// sizes, image bounds {min_x, min_y, max_x, max_y}, grid cell sizes and level tables of the target image (inv_sigma2 == nullptr: 1.0f, no chi2 test reads it)
inline void proj_grid(CorbProjDev& d, int n, int nq, const float* bounds, const float* scale, const float* inv_sigma2, int nlevels)
{
    d.n = n; d.nq = nq; d.min_x = bounds[0]; d.min_y = bounds[1]; d.max_x = bounds[2]; d.max_y = bounds[3];
    d.winv = (float)PROJ_COLS / (d.max_x - d.min_x);                   // mfGridElementWidthInv / HeightInv (Frame.cc:101-102; KeyFrame.cc:44-45)
    d.hinv = (float)PROJ_ROWS / (d.max_y - d.min_y);
    for (int l = 0; l < nlevels; l++) { d.scale[l] = scale[l]; d.inv_sigma2[l] = inv_sigma2 ? inv_sigma2[l] : 1.0f; }
}

// the matcher's scratch for `n` target features and `nq` queries.  The results are ONE block (one copy to the host): n_in_view | n_matches | status | res, where res
// is match[n] after the greedy resolution per feature (greedy, cand_cap == 0) and best_idx[nq] | best_dist[nq] where the result is one feature per query (the
// independent best candidate of Fuse / SearchBySim3; SearchForInitialization, whose candidate lists hold cand_cap entries).  Without `greedy` the candidate
// lists are a token.
struct ProjBuffers {
    CorbProjQuery* query; int *feat_cell, *cell_off, *cell_idx, *cand_cnt, *ev_feat, *ev_bin, *n_matches, *res;
    unsigned long long* cand_key; unsigned char* cand_oct;
    int nq, cand_cap; bool per_query;
    int* n_in_view() const { return n_matches - 1; }
    int alloc(CorbScratch& pool, int n, int nq_, bool greedy, int cand_cap_)
    {
        nq = nq_; cand_cap = cand_cap_; per_query = !greedy || cand_cap;
        const size_t lists = greedy ? (size_t)(nq > 0 ? nq : 1) * (cand_cap ? cand_cap : PROJ_CAND_CAP) : 0;
        int* blk;
        HIPCHK(pool.alloc(&query, (size_t)nq)); HIPCHK(pool.alloc(&feat_cell, (size_t)n)); HIPCHK(pool.alloc(&cell_off, (size_t)PROJ_CELLS + 1)); HIPCHK(pool.alloc(&cell_idx, (size_t)n));
        HIPCHK(pool.alloc(&cand_key, lists)); HIPCHK(pool.alloc(&cand_oct, lists ? lists : 8)); HIPCHK(pool.alloc(&cand_cnt, (size_t)nq));
        HIPCHK(pool.alloc(&ev_feat, (size_t)nq)); HIPCHK(pool.alloc(&ev_bin, (size_t)nq));
        HIPCHK(pool.alloc(&blk, 64 + (per_query ? 2 * (size_t)nq : (size_t)n)));
        res = blk + 64; n_matches = res - 2;
        HIPCHK(hipMemsetAsync(blk + 60, 0, 16, pool.stream));
        return CORB_OK;
    }
    void bind(CorbProjDev& d) const
    {
        d.query = query; d.feat_cell = feat_cell; d.cell_off = cell_off; d.cell_idx = cell_idx; d.cand_key = cand_key; d.cand_oct = cand_oct; d.cand_cnt = cand_cnt;
        d.ev_feat = ev_feat; d.ev_bin = ev_bin; d.n_matches = n_matches; d.status = n_matches + 1; d.cand_cap = cand_cap;
        if (per_query) { d.best_idx = res; d.best_dist = res + nq; } else d.match = res;
    }
};

// the end of a call whose result is counted on the device: read back n_matches | status (+ res[0 .. n) when `out` is wanted, + n_in_view in front) together with
// whatever read-backs the caller has queued, report a full candidate list with the caller's name, else hand the results over (caller arrays are only
// written when the call succeeds)
inline int proj_finish(CorbScratch& pool, const ProjBuffers& pb, int n, int32_t* out, int* n_matches, int* n_in_view, const char* who)
{
    static thread_local std::vector<int32_t> blk;
    const int lead = n_in_view ? 1 : 0;
    blk.resize((size_t)n + 3);
    HIPCHK(pool.d2h(blk.data(), pb.n_matches - lead, ((size_t)lead + 2 + (out ? n : 0)) * 4));
    HIPCHK(pool.fetch_finish());
    const int32_t* r = blk.data() + lead;
    if (r[1] != 0) { corb_set_error("%s: more than %d candidates in one search window", who, pb.cand_cap ? pb.cand_cap : PROJ_CAND_CAP); return CORB_ERR_OVERFLOW; }
    if (out) memcpy(out, r + 2, (size_t)n * 4);
    *n_matches = r[0]; if (n_in_view) *n_in_view = blk[0];
    return CORB_OK;
}

// the end of a call whose result is one feature per query: best_idx | best_dist in one copy, together with whatever read-backs the caller has queued
inline int proj_finish_best(CorbScratch& pool, const ProjBuffers& pb, int32_t* best_idx, int32_t* best_dist)
{
    static thread_local std::vector<int32_t> blk;
    const size_t nq = (size_t)pb.nq;
    blk.resize(2 * nq);
    HIPCHK(pool.d2h(blk.data(), pb.res, 2 * nq * 4));
    HIPCHK(pool.fetch_finish());
    memcpy(best_idx, blk.data(), nq * 4); memcpy(best_dist, blk.data() + nq, nq * 4);
    return CORB_OK;
}

}  // namespace proj_host

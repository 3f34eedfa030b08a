// track_host.h -- host rules the tracking calls on records share (corb_track.cpp, corb_tracklocal.cpp): a record as the target image of a matcher, and
// PoseOptimization(Frame*) on a record put on a stream.  Each is stated here once.  Host code only.
#pragma once
#include "track_internal.h"
#include "proj_host.h"

void corb_pose_from_T(const float* T, double* out7);
void corb_pose_to_T(const double* p7, float* T);
void corb_pose_optimization_stages(CorbBAStage* st);

namespace track_host {

inline bool camera_ok(const CorbTrackCamera* cam) { return cam->nlevels >= 1 && cam->nlevels <= CORB_MAX_LEVELS && cam->max_x > cam->min_x && cam->max_y > cam->min_y; }

// the target image of a matcher is a record: grid and level tables from the camera (mvInvLevelSigma2 = 1 / mvLevelSigma2, ORBextractor.cc:418-430), arrays of the record
inline void record_target(CorbProjDev& d, const CorbTrackCamera* cam, const char* rec, const RecLayout& L, int n, int nq)
{
    const float bounds[4] = {cam->min_x, cam->min_y, cam->max_x, cam->max_y};
    float inv_sigma2[CORB_MAX_LEVELS];
    for (int l = 0; l < cam->nlevels; l++) inv_sigma2[l] = 1.0f / (cam->scale[l] * cam->scale[l]);
    proj_host::proj_grid(d, n, nq, bounds, cam->scale, inv_sigma2, cam->nlevels);
    d.keys = reinterpret_cast<const CorbKeyPoint*>(rec + L.kp); d.u_right = reinterpret_cast<const float*>(rec + L.ur); d.desc = reinterpret_cast<const unsigned long long*>(rec + L.desc);
}

// what track_pose_finish_kernel packs for the host: one copy instead of three
struct PoseResult { double pose[7]; int cnt[4]; int E[2]; };
static_assert(sizeof(PoseResult) == 80, "pose | counters | edge counts");
// `if(nInitialCorrespondences<3) return 0;` else nInitialCorrespondences-nBad
inline int pose_inliers(const PoseResult& r) { return r.E[1] < 3 ? 0 : r.cnt[3]; }

// Optimizer::PoseOptimization(Frame*) on the record t.cur, n = t.n_cur > 0 features, from Tcw_in: gather, the four rounds, finish, all on the pool's stream.  The
// caller has set t.cur / F / n_cur / mp_base / mp_bytes / idt / discard (/ skip); result: where the finish kernel leaves a PoseResult, NULL = allocated here
// (t.result either way); t.rejected is allocated when want_rejected.  dev_Tcw: NULL, or the start pose as 16 floats on the device (a chain that computed it
// there); Tcw_in is then not read
inline int pose_enqueue(CorbScratch& pool, TrackPoseDev& t, const CorbTrackCamera* cam, const float* Tcw_in, bool want_rejected, double* result, const float* dev_Tcw = nullptr)
{
    const int n = t.n_cur;
    double *dpose, *dcam, *dlast; unsigned char* dact; int* dcnt;
    HIPCHK(pool.alloc(&t.edge_off, 2)); HIPCHK(pool.alloc(&t.stage_limit, 1)); HIPCHK(pool.alloc(&t.pt, (size_t)3 * n)); HIPCHK(pool.alloc(&t.obs, (size_t)3 * n)); HIPCHK(pool.alloc(&t.w, (size_t)n));
    HIPCHK(pool.alloc(&t.dim, (size_t)n)); HIPCHK(pool.alloc(&t.efeat, (size_t)n)); HIPCHK(pool.alloc(&dlast, (size_t)n)); HIPCHK(pool.alloc(&dact, (size_t)n)); HIPCHK(pool.alloc(&dcnt, 4));
    double h[12] = {0, 0, 0, 1, 0, 0, 0};
    if (!dev_Tcw) corb_pose_from_T(Tcw_in, h);
    h[7] = cam->fx; h[8] = cam->fy; h[9] = cam->cx; h[10] = cam->cy; h[11] = cam->bf;
    HIPCHK(pool.upload_block({{(void**)&dpose, h, sizeof(h)}}));
    dcam = dpose + 7;
    if (dev_Tcw) track_launch_pose_start(dev_Tcw, dpose, pool.stream);
    track_launch_pose_gather(t, pool.stream);
    CorbPoseDev d; memset(&d, 0, sizeof(d));
    d.n_problems = 1; d.n_stages = 4; corb_pose_optimization_stages(d.stages);
    d.edge_off = t.edge_off; d.pt = t.pt; d.obs = t.obs; d.w = t.w; d.dim = t.dim; d.cam = dcam; d.pose = dpose; d.last_chi2 = dlast; d.active = dact; d.counters = dcnt;
    d.stage_limit = t.stage_limit;                      // the edge count is on the device: the gather kernel turns it into the reference's early exits
    pose_launch_optimize(d, n, pool.stream);
    t.active = dact; t.pose = dpose; t.counters = dcnt;
    if (!result) HIPCHK(pool.alloc(&result, 10));
    t.result = result;
    if (want_rejected) HIPCHK(pool.alloc(&t.rejected, (size_t)n));
    track_launch_pose_finish(t, pool.stream);
    HIPCHK(hipGetLastError());
    return CORB_OK;
}

}  // namespace track_host

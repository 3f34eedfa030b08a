// corb_pose.cpp -- host side of the fused single-pose optimiser (pose_kernels.hip): Optimizer::PoseOptimization for a batch of frames, and the pose conversions
// every BA route shares.
#include "ba_host.h"
#include "pose_internal.h"
#include <algorithm>

// Converter::toSE3Quat (Converter.cc:37-47): float R,t -> double -> Eigen::Quaterniond(R), normalizeRotation
static void quat_from_R(const double* R, double* q)
{
    double t = R[0] + R[4] + R[8];
    if (t > 0) { t = std::sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t; q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t; }
    else {
        int i = 0; if (R[4] > R[0]) i = 1; if (R[8] > R[i * 3 + i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(R[i * 3 + i] - R[j * 3 + j] - R[k * 3 + k] + 1.0);
        q[i] = 0.5 * t; t = 0.5 / t;
        q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t; q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t; q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
    }
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}
static void quat_to_R(const double* q, double* R)
{
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
void corb_pose_from_T(const float* T, double* out7)
{
    const double R[9] = { T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10] };
    quat_from_R(R, out7);
    out7[4] = T[3]; out7[5] = T[7]; out7[6] = T[11];
}
// Converter::toCvMat (double -> float)
void corb_pose_to_T(const double* p7, float* T)
{
    double R[9]; quat_to_R(p7, R);
    T[0] = (float)R[0]; T[1] = (float)R[1]; T[2] = (float)R[2]; T[3] = (float)p7[4];
    T[4] = (float)R[3]; T[5] = (float)R[4]; T[6] = (float)R[5]; T[7] = (float)p7[5];
    T[8] = (float)R[6]; T[9] = (float)R[7]; T[10] = (float)R[8]; T[11] = (float)p7[6];
    T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
}
// runs the batch; active_out[E] (1 = inlier), counters[n][4] = iterations, trials, touched, inliers; last_out optional
int pose_batch_run(const PoseBatch& b, const CorbBAStage* stages, int n_stages, std::vector<double>& pose_out, std::vector<unsigned char>& active_out,
                   std::vector<int>& counters, double* ms_total)
{
    const int n = (int)b.edge_off.size() - 1, E = b.edge_off[n];
    CorbScratch pool(0);                                   // per-frame call of the tracking thread: short lane
    CorbPoseDev d; memset(&d, 0, sizeof(d));
    d.n_problems = n; d.n_stages = n_stages;
    for (int s = 0; s < n_stages; s++) d.stages[s] = stages[s];
    int* doff; int* dlim = nullptr; double *dpt, *dobs, *dw, *dcam, *dpose, *dlast; unsigned char *ddim, *dact; int* dcnt;
    HIPCHK(pool.upload_block({{(void**)&doff, b.edge_off.data(), b.edge_off.size() * 4}, {(void**)&dlim, b.stage_limit.data(), b.stage_limit.size() * 4}, {(void**)&dpt, b.pt.data(), b.pt.size() * 8}, {(void**)&dobs, b.obs.data(), b.obs.size() * 8},
                              {(void**)&dw, b.w.data(), b.w.size() * 8}, {(void**)&ddim, b.dim.data(), b.dim.size()}, {(void**)&dcam, b.cam.data(), b.cam.size() * 8},
                              {(void**)&dpose, b.pose.data(), b.pose.size() * 8}}));
    // results: counters | inlier flags are one block, the poses stay where they were uploaded; both copies are enqueued behind the kernel, one wait
    unsigned char* dres = nullptr;
    const size_t cnt_bytes = sizeof(int) * 4 * (size_t)n;
    HIPCHK(pool.alloc(&dlast, (size_t)E)); HIPCHK(pool.alloc(&dres, cnt_bytes + (size_t)(E ? E : 1)));
    dcnt = reinterpret_cast<int*>(dres); dact = dres + cnt_bytes;
    d.edge_off = doff; d.pt = dpt; d.obs = dobs; d.w = dw; d.dim = ddim; d.cam = dcam; d.pose = dpose; d.last_chi2 = dlast; d.active = dact; d.counters = dcnt; d.stage_limit = b.stage_limit.empty() ? nullptr : dlim;
    hipEvent_t e0 = pool.event(6), e1 = pool.event(7);
    HIPCHK(hipEventRecord(e0, pool.stream));
    int max_edges = 0; for (int k = 0; k < n; k++) max_edges = std::max(max_edges, b.edge_off[k + 1] - b.edge_off[k]);
    pose_launch_optimize(d, max_edges, pool.stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e1, pool.stream));
    pose_out.resize(7 * (size_t)n); active_out.resize(E ? E : 1); counters.resize(4 * (size_t)n);
    static thread_local std::vector<unsigned char> res;
    res.resize(cnt_bytes + (size_t)(E ? E : 1));
    HIPCHK(pool.d2h(pose_out.data(), dpose, sizeof(double) * 7 * (size_t)n));
    HIPCHK(pool.d2h(res.data(), dres, res.size()));
    HIPCHK(pool.fetch_finish());
    memcpy(counters.data(), res.data(), cnt_bytes);
    if (E) memcpy(active_out.data(), res.data() + cnt_bytes, (size_t)E);
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    if (ms_total) *ms_total = ms;
    return CORB_OK;
}
// (corb_track.cpp: the same conversions and the same four rounds for a frame that lives in a store record)
void corb_pose_optimization_stages(CorbBAStage* st)
{
    // the four rounds of Optimizer.cc:385-470: chi2 thresholds 5.991 / 7.815, Huber deltas sqrt of those, the last round without kernel
    for (int s = 0; s < 4; s++) {
        memset(&st[s], 0, sizeof(CorbBAStage));
        st[s].iterations = 10; st[s].robust = s < 3 ? 1 : 0; st[s].chi2_mono = 5.991f; st[s].chi2_stereo = 7.815f;
        st[s].recompute_inactive = 1; st[s].allow_reactivate = 1; st[s].reset_estimates = 1; st[s].float_compare = 1;
        st[s].huber_mono = sqrtf(5.991f); st[s].huber_stereo = sqrtf(7.815f);
    }
}
/* Optimizer::PoseOptimization(Frame*) for a batch of frames: one workgroup per frame, no host round trips */
extern "C" int corb_pose_optimization_batch(const CorbPoseOptFrame* frames, int n_frames, float* Tcw_out, uint8_t* const* outlier,
                                            int32_t* n_inliers, int device)
{
    if (!frames || n_frames < 1 || !Tcw_out) { corb_set_error("corb_pose_optimization_batch: bad argument"); return CORB_ERR_ARG; }
    int rc = corb_select_device(device); if (rc) return rc;
    PoseBatch b;
    for (int f = 0; f < n_frames; f++) {
        const CorbPoseOptFrame& F = frames[f];
        if (!F.Tcw || F.n_obs < 0 || (F.n_obs > 0 && (!F.points || !F.u || !F.v || !F.u_right || !F.inv_sigma2))) { corb_set_error("corb_pose_optimization_batch: frame %d: bad argument", f); return CORB_ERR_ARG; }
        double p7[7]; corb_pose_from_T(F.Tcw, p7);
        b.pose.insert(b.pose.end(), p7, p7 + 7);
        const double cam[5] = { F.fx, F.fy, F.cx, F.cy, F.bf };
        b.cam.insert(b.cam.end(), cam, cam + 5);
        for (int i = 0; i < F.n_obs; i++) {
            for (int a = 0; a < 3; a++) b.pt.push_back((double)F.points[3 * (size_t)i + a]);
            b.obs.push_back(F.u[i]); b.obs.push_back(F.v[i]); b.obs.push_back(F.u_right[i]);
            b.w.push_back(F.inv_sigma2[i]); b.dim.push_back(F.u_right[i] < 0 ? 2 : 3);             // mvuRight<0 -> monocular edge (Optimizer.cc:310)
        }
        b.edge_off.push_back(b.edge_off.back() + F.n_obs);
        // `if(nInitialCorrespondences<3) return 0;` (Optimizer.cc:396-397): no optimisation at all; `if(optimizer.edges().size()<10) break;` (:470-471):
        // one round only
        b.stage_limit.push_back(F.n_obs < 3 ? 0 : F.n_obs < 10 ? 1 : 4);
    }
    CorbBAStage st[4]; corb_pose_optimization_stages(st);
    std::vector<double> pose; std::vector<unsigned char> act; std::vector<int> cnt;
    rc = pose_batch_run(b, st, 4, pose, act, cnt, nullptr); if (rc) return rc;
    for (int f = 0; f < n_frames; f++) {
        if (frames[f].n_obs < 3) {                        // plain `return 0`: pose untouched, mvbOutlier as set while the edges were collected (all false)
            memcpy(Tcw_out + 16 * (size_t)f, frames[f].Tcw, 16 * sizeof(float));
            if (outlier && outlier[f]) for (int i = 0; i < frames[f].n_obs; i++) outlier[f][i] = 0;
            if (n_inliers) n_inliers[f] = 0;
            continue;
        }
        if (cnt[4 * (size_t)f + 2]) corb_pose_to_T(&pose[7 * (size_t)f], Tcw_out + 16 * (size_t)f);
        else memcpy(Tcw_out + 16 * (size_t)f, frames[f].Tcw, 16 * sizeof(float));
        if (outlier && outlier[f]) for (int i = 0; i < frames[f].n_obs; i++) outlier[f][i] = act[b.edge_off[f] + i] ? 0 : 1;
        if (n_inliers) n_inliers[f] = cnt[4 * (size_t)f + 3];
    }
    return CORB_OK;
}

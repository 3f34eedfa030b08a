// corb_ba.cpp -- C-ABI host side of the global bundle adjustment (see include/corb_accel.h).
// Follows Optimizer::BundleAdjustment (corbslam_client/src/Optimizer.cc:54-270): graph flattening, the
// g2o index mapping (free poses, then free landmarks, ascending id; G/core/sparse_optimizer.cpp:166-190),
// and the Levenberg-Marquardt control flow (G/core/optimization_algorithm_levenberg.cpp:61-164).  All
// per-edge / per-vertex arithmetic runs in ba_kernels.hip; the dense reduced camera system is factorised
// by the hand-written blocked Cholesky of dense_chol.hip.  The host only sequences launches and reads back 3 scalars per trial.
#include "ba_internal.h"
#include "device_util.h"
#include "pose_internal.h"
#include "corb_workspace.h"
#include "dense_chol.h"
#include "ba_multilevel.h"
#include "ba_device_problem.h"
#include <atomic>
#include <vector>
#include <memory>
#include <mutex>
#include <algorithm>
#include <cmath>
#include <cfloat>
#include <cstring>
#include <chrono>
#include <thread>
#include <cstdio>
#include <cstdlib>

void corb_set_error(const char* fmt, ...);
int corb_select_device(int device);

#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { corb_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); return CORB_ERR_HIP; } } while (0)

namespace {
// host flattening of large maps runs on a few worker threads: contiguous index ranges, results identical to the serial order
template <class F> void parallel_ranges(size_t n, int threads, F fn)
{
    if (threads <= 1 || n < 2) { fn(0, (size_t)0, n); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++) { const size_t b = n * t / threads, e = n * (t + 1) / threads; th.emplace_back([=] { fn(t, b, e); }); }
    for (auto& x : th) x.join();
}
// worker threads of the host-side graph flattening for n observations: 8 / 16 / 32 from ~2 / 4 / 16 M on (27.5 M observations: 0.45 s serial of a 1.3 s call), 4 from
// ~260 k on (660 k observations: 12.5 ms serial beside 40 ms of device time); local windows stay serial.  CORB_BA_HOST_THREADS=n forces a count
// (tests: the threaded paths produce the serial paths' lists, element for element).
static int ba_host_threads(size_t n, bool sort_stage = false)
{
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    if (const char* f = getenv("CORB_BA_HOST_THREADS")) { const int v = atoi(f); if (v > 0) return (int)std::min((unsigned)v, std::max(hw, 2u)); }
    // (the filter + two-level sort only pay from ~2 M observations: 2.5 ms serial, 4.2 ms on 4 threads at 660 k)
    // (27.5 M observations: 163 / 105 / 75 ms of flattening on 8 / 16 / 32 threads)
    return (int)std::min(hw, n >= ((size_t)1 << 24) ? 32u : n >= ((size_t)1 << 22) ? 16u : n >= ((size_t)1 << 21) ? 8u : (n >= ((size_t)1 << 18) && !sort_stage) ? 4u : 1u);
}
struct Pool : CorbScratch { Pool() : CorbScratch(1) {} };      // bundle adjustment runs in the long-optimisation lane

// Converter::toSE3Quat (Converter.cc:37-47): float R,t -> double -> Eigen::Quaterniond(R), normalizeRotation
void quat_from_R_host(const double* R, double* q)
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
void quat_to_R_host(const double* q, double* R)
{
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
}  // namespace

namespace {
struct BAState { std::vector<double> q, t, pt; };      // double-precision estimates carried across stages

void state_from_floats(const CorbBAProblem* p, BAState& st)
{
    const int K = p->n_poses, M = p->n_points;
    st.q.resize(4 * (size_t)K); st.t.resize(3 * (size_t)K); st.pt.resize(3 * (size_t)M);
    for (int k = 0; k < K; k++) {
        const float* T = p->poses + 16 * (size_t)k;
        const double R[9] = { T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10] };
        quat_from_R_host(R, &st.q[4 * (size_t)k]);
        st.t[3 * (size_t)k] = T[3]; st.t[3 * (size_t)k + 1] = T[7]; st.t[3 * (size_t)k + 2] = T[11];
    }
    for (size_t i = 0; i < 3 * (size_t)M; i++) st.pt[i] = p->points[i];
}

// write-back: Converter::toCvMat (double -> float); fixed / never-optimised vertices are passed through
void state_to_floats(const CorbBAProblem* p, const BAState& st, const std::vector<uint8_t>& pose_touched, const std::vector<uint8_t>& pt_touched, CorbBAResult* r)
{
    for (int k = 0; k < p->n_poses; k++) {
        float* T = r->poses + 16 * (size_t)k;
        if (p->pose_fixed[k] || !pose_touched[k]) { memcpy(T, p->poses + 16 * (size_t)k, 16 * sizeof(float)); continue; }
        double R[9]; quat_to_R_host(&st.q[4 * (size_t)k], R);
        T[0] = (float)R[0]; T[1] = (float)R[1]; T[2] = (float)R[2]; T[3] = (float)st.t[3 * (size_t)k];
        T[4] = (float)R[3]; T[5] = (float)R[4]; T[6] = (float)R[5]; T[7] = (float)st.t[3 * (size_t)k + 1];
        T[8] = (float)R[6]; T[9] = (float)R[7]; T[10] = (float)R[8]; T[11] = (float)st.t[3 * (size_t)k + 2];
        T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
    }
    for (int m = 0; m < p->n_points; m++) {
        const bool keep = p->point_fixed[m] || !pt_touched[m];
        for (int a = 0; a < 3; a++) r->points[3 * (size_t)m + a] = keep ? p->points[3 * (size_t)m + a] : (float)st.pt[3 * (size_t)m + a];
    }
}

// intrinsics of every pose vertex as doubles (e->fx = pKF->fx ... e->bf = pKF->mbf: float -> double, Optimizer.cc:160-163, 189-193)
void cam_table(const CorbBAProblem* p, std::vector<double>& cam)
{
    cam.resize(5 * (size_t)(p->n_poses > 0 ? p->n_poses : 1));
    for (int k = 0; k < p->n_poses; k++) {
        double* c = &cam[5 * (size_t)k];
        if (p->intr) for (int a = 0; a < 5; a++) c[a] = p->intr[5 * (size_t)k + a];
        else { c[0] = p->fx; c[1] = p->fy; c[2] = p->cx; c[3] = p->cy; c[4] = p->bf; }
    }
}

int validate(const CorbBAProblem* p, const CorbBAResult* r)
{
    if (!p || !r || !r->poses || !r->points || p->n_poses < 0 || p->n_points < 0 || p->n_edges < 0 ||
        (p->n_poses > 0 && (!p->poses || !p->pose_fixed)) || (p->n_points > 0 && (!p->points || !p->point_fixed)) || (p->n_edges > 0 && !p->edges)) {
        corb_set_error("corb_ba_solve: bad argument"); return CORB_ERR_ARG;
    }
    for (int i = 0; i < p->n_edges; i++)
        if (p->edges[i].pose < 0 || p->edges[i].pose >= p->n_poses || p->edges[i].point < 0 || p->edges[i].point >= p->n_points) { corb_set_error("corb_ba_solve: edge %d out of range", i); return CORB_ERR_ARG; }
    return CORB_OK;
}

// fresh e->computeError() / isDepthPositive() of EVERY edge at the given estimates (classification between stages)
int ba_eval_edges_device(const CorbBAProblem* p, const std::vector<double>& q, const std::vector<double>& t, const std::vector<double>& pt,
                         std::vector<double>& chi2, std::vector<double>& depth)
{
    const int E = p->n_edges;
    chi2.assign(E ? E : 1, 0.0); depth.assign(E ? E : 1, 0.0);
    if (E == 0) return CORB_OK;
    std::vector<int> vp(E), vx(E); std::vector<double> obs(3 * (size_t)E), w(E); std::vector<unsigned char> dim(E);
    for (int i = 0; i < E; i++) { const CorbBAEdge& e = p->edges[i]; vp[i] = e.pose; vx[i] = e.point; dim[i] = e.u_right < 0 ? 2 : 3;
                                  obs[3 * (size_t)i] = e.u; obs[3 * (size_t)i + 1] = e.v; obs[3 * (size_t)i + 2] = e.u_right; w[i] = e.inv_sigma2; }
    Pool pool;
    CorbBADev d; memset(&d, 0, sizeof(d));
    d.nE = E;
    std::vector<double> cam; cam_table(p, cam);
    int *dvp, *dvx; double *dobs, *dw, *dq, *dt, *dpt, *dchi, *ddep, *dcam; unsigned char* ddim;
    // one staging block in, one block (chi2 | depth) out: for a local window the eight separate copies cost more than the evaluation
    HIPCHK(pool.upload_block({{(void**)&dvp, vp.data(), vp.size() * 4}, {(void**)&dvx, vx.data(), vx.size() * 4}, {(void**)&dobs, obs.data(), obs.size() * 8}, {(void**)&dw, w.data(), w.size() * 8},
                              {(void**)&ddim, dim.data(), dim.size()}, {(void**)&dq, q.data(), q.size() * 8}, {(void**)&dt, t.data(), t.size() * 8}, {(void**)&dpt, pt.data(), pt.size() * 8},
                              {(void**)&dcam, cam.data(), cam.size() * 8}}));
    HIPCHK(pool.alloc(&dchi, (size_t)2 * E)); ddep = dchi + E;
    d.e_vpose = dvp; d.e_vpoint = dvx; d.e_obs = dobs; d.e_w = dw; d.e_dim = ddim; d.pose_q = dq; d.pose_t = dt; d.pt = dpt; d.cam = dcam;
    ba_launch_edge_eval(d, dchi, ddep, pool.stream);
    HIPCHK(hipGetLastError());
    HIPCHK(pool.d2h(chi2.data(), dchi, sizeof(double) * (size_t)E)); HIPCHK(pool.d2h(depth.data(), ddep, sizeof(double) * (size_t)E));
    HIPCHK(pool.fetch_finish());
    return CORB_OK;
}

// The flattened graph in device memory: what the Levenberg-Marquardt loop below works on.  Filled either by the host flattening of a CorbBAProblem (host
// arrays in: corb_ba_solve*) or by the device flattening of a CorbBADeviceProblem (ba_flatten.hip: corb_ba_solve_device / corb_ba_solve_store).
struct BAFlat {
    int nE = 0, nP = 0, nL = 0;                   // active edges, free poses, free landmarks
    int nA = 0;                                   // edges of free landmarks (= loff[nL]; the edges of fixed landmarks follow)
    int nnzb = 0, bsr_max_row = 0, nu = 0;        // blocks of the reduced system, largest block row, blocks on / above the diagonal
    bool have_pattern = false;
    size_t pairs_bound = 0;                       // local windows, host flattening: an upper bound of the Schur pair lists' length (0 = not known: the count is read back)
    int *e_pose = nullptr, *e_point = nullptr, *e_vpose = nullptr, *e_vpoint = nullptr, *loff = nullptr, *lnfree = nullptr, *poff = nullptr, *pedge = nullptr;
    int *pose_vertex = nullptr, *point_vertex = nullptr, *bsr_rowptr = nullptr, *bsr_col = nullptr, *bsr_diag = nullptr, *uinfo = nullptr, *plm = nullptr;
    double *e_obs = nullptr, *e_w = nullptr, *cam = nullptr; unsigned char* e_dim = nullptr;
    double *dq = nullptr, *dq_bak = nullptr;      // estimates: quaternions | translations | points (all vertices), and the push() copy
    size_t n_q = 0, n_t = 0, n_pt = 0;
};
// pcg_tol: the caller's fixed tolerance, or (pcg_forcing) the default policy: every reduced solve stops at BA_PCG_TOL_LOOSE, and a trial whose accept / reject or
// lambda decision could depend on the solve's accuracy is continued to BA_PCG_TOL_TIGHT before the decision is taken (ba_lm_device, at the trial's rho).
// tools/pcg_tol_sweep.py, round 5 (profiles/r05_pcg_tol_sweep.txt; 320 / 1 200 / 4 800 / 20 000 keyframes, 10 LM iterations against a 1e-13 solve): the chi2 after every
// iteration moves by <= 6e-8 / 3e-7 / 3.2e-6 relative at 1e-8 / 1e-5 / 1e-4 (the parity bar is 1e-4) while the CG iterations fall 902 -> 541 -> 430 at 20 000 keyframes;
// What binds the loose tolerance is lambda, not chi2: where rho falls into the steep part of the schedule, d lambda / lambda ~ 10 d rho, and rho = (chi2_old - chi2_new) /
// scale amplifies a relative chi2 error by chi2 / (chi2_old - chi2_new) -- 1e3 in the late iterations.  At 1e-5 a 100-keyframe robust problem's lambda moved by 1.5e-3
// at its seventh iteration (tests/test_gpu_ba.py compares lambda at 1e-3) -- through the chi2 the EARLIER loose iterations had left, not through that iteration's own
// solve (continuing it to 1e-8 changed nothing).  1e-6 keeps that at 1.5e-4; the continuation guards the discrete decisions.
// Two more rules keep the policy away from where NO finite tolerance reproduces an exact solve's decisions: (1) on a plateau -- chi2 flat to 1e-7 and below -- the sign of
// a trial's gain is rounding noise of whichever solver ran, and one flipped accept moves a weakly observed map point by 1e-2 without moving chi2 (a 10-keyframe robust
// problem of tests/test_gpu_ba.py: 16 / 17 / 10 trials at 1e-8 / exact / the policy): the tolerance of an iteration follows the relative gain of the iteration before it,
// tol = clamp(1e-2 gain, 1e-8, BA_PCG_TOL_LOOSE) -- the classical forcing sequence, tight as the iteration converges; (2) the policy applies to the maps the PCG solver is the automatic
// choice for (more than BA_PCG_FORCING_MIN_POSES free keyframes), where the solve is the cost; a small problem forced onto the PCG solver solves to 1e-8 like before.
// Round 6 re-examined the cap with the oracle's exact sparse LDL^T at 4 800 (non-robust and Huber) and 12 000 keyframes (tests/golden/ba_config3.json, ba_12k.json):
// tools/pcg_loose_margins.py, cap 1e-6 / 1e-5 / 1e-4 / 1e-3 (CORB_BA_PCG_LOOSE): chi2 per iteration within 1.6e-8 / 1.4e-7 / 3.1e-7 / 1.7e-5 of those trajectories, lambda
// identical, estimates within 6e-8 .. 4e-7, counts equal -- >= 300x inside every bar at 1e-4, with 500 -> 308 CG iterations at 50 000 keyframes (solve 72.7 -> 45.6 ms).
// The goldens are well-conditioned maps.  On noisy maps above 256 keyframes whose LM runs reject trials (tools/pcg_policy_rejections.py: 24 runs against the dense solver,
// 48 rejected trials) the accept / reject histories stay equal at every cap, but the worst chi2 deviation is 6e-6 at 1e-6 and 3.0e-4 / 7.1e-4 / 3.8e-4 at 1e-5 / 3e-5 /
// 1e-4 -- outside the 1e-4 parity bar.  The cap stays 1e-6; a caller who knows its maps sets CorbBAOptions.pcg_tol (bench.py reports the 1e-4 figure beside the default's).
#define BA_PCG_TOL_LOOSE 1e-6
#define BA_PCG_TOL_TIGHT 1e-8
#define BA_PCG_FORCING_MIN_POSES 256
struct BAChoice { int solver = 1, pc_g = 1; double pcg_tol = 1e-8; bool pcg_forcing = false; int pcg_max_iter = 4000; bool fused_small = false, want_pattern = false, multilevel = false; };

#define BA_TRACE(what) do { static const bool t_ = getenv("CORB_BA_TRACE") != nullptr; if (t_) { fprintf(stderr, "[corb_ba trace] %s\n", what); fflush(stderr); } } while (0)
struct Lap {                          // CORB_BA_TIMING=1: host-side phase times of a call on stderr (development aid)
    bool on; std::chrono::steady_clock::time_point t;
    Lap() : on(getenv("CORB_BA_TIMING") != nullptr), t(std::chrono::steady_clock::now()) {}
    void operator()(const char* what) {
        if (!on) return;
        auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "[corb_ba] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count()); t = n;
    }
};

// ---- multilevel preconditioner: structure (ba_multilevel.h).  Host side, once per optimize() call: the hierarchy depends on the number of free keyframes
// and the block pattern only. ----
struct MLHostLevel {
    int n = 0, stride = 0, max_row = 0;
    std::vector<int> rowptr, col;            // pattern of A_k
    std::vector<int> i0, i1, lo, hi, seg;    // hats over the level below (size n_below: i0, i1; size n: lo, hi, seg = trajectory of every node)
    std::vector<double> w1;
};
// hats of one level over the nodes of the level below, trajectory by trajectory (seg_f non-decreasing): a trajectory of m nodes gets ceil(m / stride) coarse nodes at
// the centres of its groups of `stride`, linear interpolation between neighbouring centres, constant beyond the first / last centre
static void ml_make_hats(const std::vector<int>& seg_f, int stride, MLHostLevel& c)
{
    const int n_f = (int)seg_f.size();
    c.stride = stride; c.i0.resize(n_f); c.i1.resize(n_f); c.w1.resize(n_f); c.seg.clear(); c.lo.clear(); c.hi.clear();
    int base = 0;
    for (int a = 0; a < n_f;) {
        int b = a; while (b < n_f && seg_f[b] == seg_f[a]) b++;
        const int m = b - a, nc = (m + stride - 1) / stride;
        for (int j = 0; j < m; j++) {
            const double t = ((double)j - 0.5 * (stride - 1)) / (double)stride;
            const int I0 = std::min(std::max((int)std::floor(t), 0), nc - 1), I1 = std::min(I0 + 1, nc - 1);
            double w = std::min(std::max(t - (double)I0, 0.0), 1.0);
            if (I1 == I0) w = 0.0;
            c.i0[a + j] = base + I0; c.i1[a + j] = base + I1; c.w1[a + j] = w;
        }
        for (int I = 0; I < nc; I++) c.seg.push_back(seg_f[a]);
        base += nc; a = b;
    }
    c.n = base; c.lo.assign(c.n, n_f); c.hi.assign(c.n, -1);
    for (int i = 0; i < n_f; i++) {
        c.lo[c.i0[i]] = std::min(c.lo[c.i0[i]], i); c.hi[c.i0[i]] = std::max(c.hi[c.i0[i]], i);
        if (c.w1[i] != 0.0) { c.lo[c.i1[i]] = std::min(c.lo[c.i1[i]], i); c.hi[c.i1[i]] = std::max(c.hi[c.i1[i]], i); }
    }
}
// coarse pattern of P' A P from the fine pattern: row I = the coarse nodes of the columns of the fine rows under the hat of I (stamp array, then sorted)
static void ml_coarse_pattern(const int* f_rowptr, const int* f_col, MLHostLevel& c, int threads)
{
    const int n_c = c.n;
    std::vector<std::vector<int>> part_col(threads), part_cnt(threads);
    parallel_ranges((size_t)n_c, threads, [&](int t, size_t Ib, size_t Ie) {
        std::vector<int> stamp(n_c, -1), cols, out, cnt;      // (locals, handed over at the end: see the composite lists below)
        for (size_t I = Ib; I < Ie; I++) {
            cols.clear();
            for (int i = c.lo[I]; i <= c.hi[I]; i++) {
                if (!((int)I == c.i0[i] || ((int)I == c.i1[i] && c.w1[i] != 0.0))) continue;
                for (int sl = f_rowptr[i]; sl < f_rowptr[i + 1]; sl++) {
                    const int j = f_col[sl], J0 = c.i0[j], J1 = c.i1[j];
                    if (stamp[J0] != (int)I) { stamp[J0] = (int)I; cols.push_back(J0); }
                    if (c.w1[j] != 0.0 && stamp[J1] != (int)I) { stamp[J1] = (int)I; cols.push_back(J1); }
                }
            }
            std::sort(cols.begin(), cols.end());
            cnt.push_back((int)cols.size()); out.insert(out.end(), cols.begin(), cols.end());
        }
        part_col[t] = std::move(out); part_cnt[t] = std::move(cnt);
    });
    c.rowptr.assign(n_c + 1, 0); c.max_row = 0;
    { int I = 0; for (int t = 0; t < threads; t++) for (int k : part_cnt[t]) { c.rowptr[I + 1] = c.rowptr[I] + k; c.max_row = std::max(c.max_row, k); I++; } }
    c.col.resize(c.rowptr[n_c]);
    { size_t o = 0; for (int t = 0; t < threads; t++) { if (!part_col[t].empty()) memcpy(&c.col[o], part_col[t].data(), part_col[t].size() * sizeof(int)); o += part_col[t].size(); } }
}
// The hierarchy is built on the host from the fine pattern (ba_ml_host: 15 ms at 50 000 keyframes -- on a helper thread, beside the device's pair-list kernels) and
// left in device memory by ba_ml_upload (pool); m.L == 0: not built (too few keyframes).
struct MLHostAll {
    std::vector<int> h_rowptr, h_col;                 // the fine pattern (read back by the caller)
    std::vector<MLHostLevel> lv; std::vector<int> node_off, p_ptr, p_node, r_ptr, r_pose, ch_begin, ch_ptr; std::vector<double> p_w, r_w; int n_nodes = 0;
};
static void ba_ml_host(int nP, MLHostAll& H)
{
    Lap lap_ml;
    const std::vector<int>& h_rowptr = H.h_rowptr; const std::vector<int>& h_col = H.h_col; const int nnzb = (int)h_col.size();
    std::vector<MLHostLevel>& lv = H.lv;
    // trajectories: keyframes i and i + 1 belong together iff they share a landmark, i.e. iff block (i, i + 1) is in the pattern
    std::vector<int> seg(nP, 0);
    for (int i = 0; i + 1 < nP; i++) {
        const int* b = h_col.data() + h_rowptr[i]; const int* e = h_col.data() + h_rowptr[i + 1];
        seg[i + 1] = seg[i] + (std::binary_search(b, e, i + 1) ? 0 : 1);
    }
    const int threads = ba_host_threads((size_t)nnzb * 4);
    for (int first = 1; (int)lv.size() < BA_ML_MAX_LEVELS; first = 0) {
        const std::vector<int>& seg_f = lv.empty() ? seg : lv.back().seg;
        const int n_f = (int)seg_f.size();
        if (n_f <= BA_ML_G) break;
        static const int first_stride = getenv("CORB_BA_ML_STRIDE0") ? std::max(2, atoi(getenv("CORB_BA_ML_STRIDE0"))) : BA_ML_STRIDE0;
        static const int next_stride = getenv("CORB_BA_ML_STRIDE1") ? std::max(2, atoi(getenv("CORB_BA_ML_STRIDE1"))) : 4;
        MLHostLevel l; ml_make_hats(seg_f, first ? first_stride : next_stride, l);
        if (l.n >= n_f) break;                                 // every trajectory is down to one node
        ml_coarse_pattern(lv.empty() ? h_rowptr.data() : lv.back().rowptr.data(), lv.empty() ? h_col.data() : lv.back().col.data(), l, (lv.empty() || n_f >= 2048) ? threads : 1);
        lv.push_back(std::move(l));
    }
    if (lv.empty()) return;
    lap_ml("hierarchy: levels + patterns");
    // composite restriction: per keyframe the (node, weight) list of every level, level by level (W_k = P_k' W_{k-1})
    std::vector<int>& node_off = H.node_off; node_off.assign(lv.size() + 1, 0);
    for (size_t k = 0; k < lv.size(); k++) node_off[k + 1] = node_off[k] + lv[k].n;
    const int n_nodes = H.n_nodes = node_off[lv.size()];
    std::vector<int>& p_ptr = H.p_ptr; std::vector<int>& p_node = H.p_node; std::vector<double>& p_w = H.p_w; p_ptr.assign((size_t)nP + 1, 0);
    {
        // (keyframes are independent: ranges of them on the host's threads, each into its own lists, joined in order -- 3..8 ms on one thread at 50 000 keyframes)
        std::vector<std::vector<int>> t_node(threads), t_cnt(threads); std::vector<std::vector<double>> t_w(threads);
        parallel_ranges((size_t)nP, threads, [&](int t, size_t ib, size_t ie) {
            std::vector<std::pair<int, double>> cur, nxt;
            std::vector<int> on, oc; std::vector<double> ow;      // (locals, handed over at the end: the shared arrays' vector headers would share cache lines)
            on.reserve((ie - ib) * 24); ow.reserve((ie - ib) * 24); oc.reserve(ie - ib);
            for (size_t i = ib; i < ie; i++) {
                const size_t before = on.size();
                cur.assign(1, std::make_pair((int)i, 1.0));
                for (size_t k = 0; k < lv.size(); k++) {
                    nxt.clear();
                    for (const auto& e : cur) {
                        const double w1 = lv[k].w1[e.first];
                        auto add = [&](int I, double w) { if (w == 0.0) return; for (auto& x : nxt) if (x.first == I) { x.second += w; return; } nxt.emplace_back(I, w); };
                        add(lv[k].i0[e.first], e.second * (1.0 - w1)); add(lv[k].i1[e.first], e.second * w1);
                    }
                    std::sort(nxt.begin(), nxt.end());
                    for (const auto& e : nxt) { on.push_back(node_off[k] + e.first); ow.push_back(e.second); }
                    cur.swap(nxt);
                }
                oc.push_back((int)(on.size() - before));
            }
            t_node[t] = std::move(on); t_w[t] = std::move(ow); t_cnt[t] = std::move(oc);
        });
        size_t total = 0; for (int t = 0; t < threads; t++) total += t_node[t].size();
        p_node.resize(total); p_w.resize(total);
        size_t o = 0; int i = 0;
        for (int t = 0; t < threads; t++) {
            if (!t_node[t].empty()) { memcpy(&p_node[o], t_node[t].data(), t_node[t].size() * sizeof(int)); memcpy(&p_w[o], t_w[t].data(), t_w[t].size() * sizeof(double)); }
            o += t_node[t].size();
            for (int c : t_cnt[t]) { p_ptr[i + 1] = p_ptr[i] + c; i++; }
        }
    }
    lap_ml("hierarchy: composite lists");
    // its transpose: node <- keyframes, ascending in the keyframe (counting sort by node: stable); chunks of the rows
    std::vector<int>& r_ptr = H.r_ptr; std::vector<int>& r_pose = H.r_pose; std::vector<double>& r_w = H.r_w;
    r_ptr.assign((size_t)n_nodes + 1, 0); r_pose.resize(p_node.size()); r_w.resize(p_node.size());
    for (int g : p_node) r_ptr[(size_t)g + 1]++;
    for (int g = 0; g < n_nodes; g++) r_ptr[g + 1] += r_ptr[g];
    { std::vector<int> at(r_ptr.begin(), r_ptr.end() - 1); for (int i = 0; i < nP; i++) for (int e = p_ptr[i]; e < p_ptr[i + 1]; e++) { const int o = at[p_node[e]]++; r_pose[o] = i; r_w[o] = p_w[e]; } }
    std::vector<int>& ch_begin = H.ch_begin; std::vector<int>& ch_ptr = H.ch_ptr; ch_ptr.assign((size_t)n_nodes + 1, 0);
    for (int g = 0; g < n_nodes; g++) {
        ch_ptr[g] = (int)ch_begin.size();
        // (at most 16 chunks per row -- the block kernel adds a row's chunk sums one after the other --: the rows of the top levels gather from thousands of keyframes)
        const int len = r_ptr[g + 1] - r_ptr[g], step = std::max(BA_ML_CHUNK, ((len + 15) / 16 + 63) / 64 * 64);
        for (int e = r_ptr[g]; e < r_ptr[g + 1]; e += step) ch_begin.push_back(e);
        if (r_ptr[g + 1] == r_ptr[g]) ch_begin.push_back(r_ptr[g]);             // (no entries: one empty chunk keeps the tables simple)
    }
    ch_ptr[n_nodes] = (int)ch_begin.size(); ch_begin.push_back(r_ptr[n_nodes]);
    lap_ml("hierarchy: transpose + chunks");
    // a chunk must end where its node's row ends: chunk c covers [ch_begin[c], min(ch_begin[c + 1], end of its node's row)); rows are consecutive, so ch_begin[c + 1]
    // of a node's last chunk IS the end of the row
}
// Weight of coarse level k's term in the additive sum z = D_0^-1 r + sum_k w_k W_k' D_k^-1 W_k r (k = 0: the first coarse level).  With w_k = 1 (rounds 3-5) every level
// re-counts the smooth part of the correction the levels next to it already made -- on large lambda (early LM iterations) the sum was WORSE than the 16-keyframe blocks alone
// (tools/pcg_proto.py on dumped systems, profiles/HISTORY_r6.md).  CORB_BA_ML_W = "w" or "w0,w1,...": development override (the last value serves the deeper levels).
static double ml_level_weight(int k)
{
    double last = BA_ML_WEIGHT;
    if (const char* e = getenv("CORB_BA_ML_W")) {           // (read per call: a sweep sets it between solves)
        const char* p = e;
        for (int i = 0; *p; i++) { char* q; const double x = strtod(p, &q); if (q == p) break; last = x; if (i == k) break; p = *q == ',' ? q + 1 : q; }
    }
    return last;
}
static int ba_ml_upload(Pool& pool, int nP, const MLHostAll& H, BAMLDev& m)
{
    memset(&m, 0, sizeof(m));
    const std::vector<MLHostLevel>& lv = H.lv;
    if (lv.empty()) return CORB_OK;
    const std::vector<int>& node_off = H.node_off; const int n_nodes = H.n_nodes;
    const std::vector<int>& p_ptr = H.p_ptr; const std::vector<int>& p_node = H.p_node; const std::vector<double>& p_w = H.p_w;
    const std::vector<int>& r_ptr = H.r_ptr; const std::vector<int>& r_pose = H.r_pose; const std::vector<double>& r_w = H.r_w;
    const std::vector<int>& ch_begin = H.ch_begin; const std::vector<int>& ch_ptr = H.ch_ptr;
    m.L = (int)lv.size(); m.n_nodes = n_nodes; m.n_chunks = (int)ch_begin.size() - 1;
    int blk = 0;
    for (int k = 0; k < m.L; k++) {
        BAMLLevel& c = m.lv[k];
        c.wgt = ml_level_weight(k);
        c.n = lv[k].n; c.stride = lv[k].stride; c.nblk = (c.n + BA_ML_G - 1) / BA_ML_G; c.nnzb = lv[k].rowptr[c.n]; c.max_row = lv[k].max_row;
        c.node_off = node_off[k]; c.blk_off = blk; blk += c.nblk;
        for (int I = 0; I < c.n; I++)                           // ml_galerkin_kernel: a hat's fine nodes are one run of at most 16 rows / columns
            if (lv[k].hi[I] - lv[k].lo[I] + 1 > 16) { corb_set_error("multilevel preconditioner: a hat over %d nodes", lv[k].hi[I] - lv[k].lo[I] + 1); return CORB_ERR_CAPACITY; }
        HIPCHK(pool.upload(&c.rowptr, lv[k].rowptr)); HIPCHK(pool.upload(&c.col, lv[k].col));
        HIPCHK(pool.alloc(&c.val, (size_t)c.nnzb * 36)); HIPCHK(pool.alloc(&c.pc_inv32, (size_t)c.nblk * 36 * BA_ML_G * BA_ML_G));
        int *di0, *di1, *dlo, *dhi; double* dw1;
        HIPCHK(pool.upload(&di0, lv[k].i0)); HIPCHK(pool.upload(&di1, lv[k].i1)); HIPCHK(pool.upload(&dw1, lv[k].w1)); HIPCHK(pool.upload(&dlo, lv[k].lo)); HIPCHK(pool.upload(&dhi, lv[k].hi));
        c.i0 = di0; c.i1 = di1; c.w1 = dw1; c.lo = dlo; c.hi = dhi;
    }
    m.n_blocks = blk;
    int *dp_ptr, *dp_node, *dr_ptr, *dr_pose, *dch_begin, *dch_ptr; double *dp_w, *dr_w;
    HIPCHK(pool.upload(&dp_ptr, p_ptr)); HIPCHK(pool.upload(&dp_node, p_node)); HIPCHK(pool.upload(&dp_w, p_w));
    HIPCHK(pool.upload(&dr_ptr, r_ptr)); HIPCHK(pool.upload(&dr_pose, r_pose)); HIPCHK(pool.upload(&dr_w, r_w));
    HIPCHK(pool.upload(&dch_begin, ch_begin)); HIPCHK(pool.upload(&dch_ptr, ch_ptr));
    m.p_ptr = dp_ptr; m.p_node = dp_node; m.p_w = dp_w; m.r_ptr = dr_ptr; m.r_pose = dr_pose; m.r_w = dr_w; m.ch_begin = dch_begin; m.ch_ptr = dch_ptr;
    HIPCHK(pool.alloc(&m.ch_sum, (size_t)6 * m.n_chunks)); HIPCHK(pool.alloc(&m.rk, (size_t)6 * n_nodes)); HIPCHK(pool.alloc(&m.yk, (size_t)6 * n_nodes));
    m.np = (6 * nP + 255) / 256; m.ngrp = (m.np + 63) / 64;
    HIPCHK(pool.alloc(&m.part, (size_t)m.np)); HIPCHK(pool.alloc(&m.part2, (size_t)m.ngrp)); HIPCHK(pool.alloc(&m.tick, ((size_t)m.ngrp + 1) * 64));
    return CORB_OK;
}

// optimizer.optimize(iterations) on a flattened graph: allocates the work arrays from the lane's arena, runs g2o's Levenberg-Marquardt control
// (G/core/optimization_algorithm_levenberg.cpp:61-164) and leaves the estimates in f.dq.  *e_chi2_out (optional) = chi2 of every edge's last computeError().
// The work arrays and pair lists of a local window's optimize() (dense reduced system, one-workgroup solve), kept by a staged solve's session: the later optimize()
// calls run on the same graph and take them as they are instead of allocating and building them again.
struct LMWork { bool ready = false; int n_pairs = 0; CorbBADev d; double* d_partial = nullptr; double* d_scal = nullptr; double* d_chi_partial = nullptr; BALMCtl* d_ctl = nullptr; };
int ba_lm_device(Pool& pool, BAFlat& f, const BAChoice& ch, int iterations, int robust, volatile int* stop_flag, CorbBAResult* r, double delta2, double delta3,
                 Lap& lap, double** e_chi2_out, LMWork* work = nullptr)
{
    const int nE = f.nE, nP = f.nP, nL = f.nL, sp = 6 * nP;
    // (CORB_BA_PCG_LOOSE: the cap of the default policy's forcing sequence, for A/B runs against the oracle goldens -- tools/pcg_loose_sweep.sh)
    static const double tol_loose = getenv("CORB_BA_PCG_LOOSE") ? std::min(1e-2, std::max(BA_PCG_TOL_TIGHT, atof(getenv("CORB_BA_PCG_LOOSE")))) : BA_PCG_TOL_LOOSE;
    const int solver = ch.solver, pc_g = ch.pc_g; double pcg_tol = ch.pcg_forcing ? tol_loose : ch.pcg_tol; const int pcg_max_iter = ch.pcg_max_iter;
    const bool fused_small = ch.fused_small, want_pattern = f.have_pattern, timing = lap.on;
    const bool use_pairs = want_pattern;        // every multi-kernel call runs the deterministic pair-list Schur kernel
    const int nnzb = f.nnzb, bsr_max_row = f.bsr_max_row;
    int rc = CORB_OK;
    hipStream_t s = pool.stream;
    double* cert_b = nullptr; double* cert_part = nullptr; double* cert_out = nullptr;
    CorbBADev d; memset(&d, 0, sizeof(d));
    BAMLDev ml; memset(&ml, 0, sizeof(ml));
    // multilevel preconditioner: the hierarchy's host part runs on a helper thread while this one enqueues and waits for the pair-list kernels
    MLHostAll ml_host; std::thread ml_thread;
    struct ThreadJoin { std::thread& t; ~ThreadJoin() { if (t.joinable()) t.join(); } } ml_join{ml_thread};
    if (ch.multilevel && solver == 2 && pc_g == BA_ML_G && want_pattern && nP > BA_ML_G) {
        ml_host.h_rowptr.resize((size_t)nP + 1); ml_host.h_col.resize((size_t)nnzb);
        HIPCHK(pool.d2h(ml_host.h_rowptr.data(), f.bsr_rowptr, sizeof(int) * ((size_t)nP + 1))); HIPCHK(pool.d2h(ml_host.h_col.data(), f.bsr_col, sizeof(int) * (size_t)nnzb));
        HIPCHK(pool.fetch_finish());
        ml_thread = std::thread([&ml_host, nP]() { ba_ml_host(nP, ml_host); });
    }
    bool ml_pending = false;                      // the helper thread's hierarchy has not been taken over yet
    double* chol_ws = nullptr;                    // workspace of the dense solve (solver 1 above the one-workgroup sizes), allocated at its first use
    const bool reuse = work && work->ready;
    int* h_npairs = nullptr;                      // (page-locked) the pair lists' length, when it was not waited for
    int *d_bad = nullptr, *d_info = nullptr; double *d_partial = nullptr, *d_scal = nullptr;
    const size_t n_state = f.n_q + f.n_t + f.n_pt;
    double* dq = f.dq; double* dq_bak = f.dq_bak;
    // per-workgroup partial sums of the chi2 / scale reductions: small problems use ONE workgroup, which writes the result directly
    const int nparts = std::max(1, std::min(256, (std::max(nE, sp + 3 * nL) + 1023) / 1024));
    const int n_upd_blocks = (std::max(nP, nL) + 255) / 256;
    if (reuse) {
        d = work->d; d_partial = work->d_partial; d_scal = work->d_scal; d_bad = reinterpret_cast<int*>(d_scal + 6); d_info = d_bad + 1;
        HIPCHK(hipMemsetAsync(d_bad, 0, 2 * sizeof(int), s));
    } else {
    d.nE = nE; d.nP = nP; d.nL = nL; d.sp = sp;
    int *de_pose = f.e_pose, *de_point = f.e_point, *de_vpose = f.e_vpose, *de_vpoint = f.e_vpoint, *dloff = f.loff, *dlnfree = f.lnfree, *dpoff = f.poff, *dpedge = f.pedge;
    int *dpv = f.pose_vertex, *dlv = f.point_vertex;
    double *de_obs = f.e_obs, *de_w = f.e_w, *dt = f.dq + f.n_q, *dpt = f.dq + f.n_q + f.n_t, *dcam = f.cam;
    unsigned char* de_dim = f.e_dim;
    // scalars [0..5] and the two status words (as the 7th double) are one block: one read-back per trial
    // (the reductions' ticket lives behind them, so that one fill clears it and the status words)
    HIPCHK(pool.alloc(&d_partial, (size_t)std::max(nparts, n_upd_blocks <= BA_FUSED_UPDATE_BLOCKS ? n_upd_blocks : 1))); HIPCHK(pool.alloc(&d_scal, 16)); d_bad = reinterpret_cast<int*>(d_scal + 6); d_info = d_bad + 1;
    d.red_tick = reinterpret_cast<int*>(d_scal + 8);
    HIPCHK(hipMemsetAsync(d_bad, 0, 3 * sizeof(double), s));      // (d_bad holds the number of the trial that failed: never cleared again)
    d.e_pose = de_pose; d.e_point = de_point; d.e_vpose = de_vpose; d.e_vpoint = de_vpoint; d.e_obs = de_obs; d.e_w = de_w; d.e_dim = de_dim;
    d.loff = dloff; d.lnfree = dlnfree; d.poff = dpoff; d.pedge = dpedge; d.pose_vertex = dpv; d.point_vertex = dlv;
    d.pose_q = dq; d.pose_t = dt; d.pt = dpt; d.cam = dcam;
    // lean records on the multi-kernel path (JB | r, no Hpl array: see ba_build_lean_kernel); the one-workgroup optimiser keeps round 2's per-edge blocks
    d.lean = fused_small ? 0 : 1; d.backsub_rederive = (d.lean && !getenv("CORB_BA_BACKSUB_V")) ? 1 : 0; d.edge_stride = d.lean ? 21 : BA_EDGE_STRIDE; d.edge_jb = d.lean ? 0 : 9; d.nfree_edges = f.nA;
    HIPCHK(pool.alloc(&d.edge_blk, (size_t)nE * d.edge_stride)); if (!d.lean) HIPCHK(pool.alloc(&d.hpl, (size_t)nE * 18)); HIPCHK(pool.alloc(&d.Hpp, (size_t)nP * 36)); HIPCHK(pool.alloc(&d.Hll, (size_t)nL * 9));
    HIPCHK(pool.alloc(&d.b, (size_t)sp + 3 * (size_t)nL)); HIPCHK(pool.alloc(&d.x, (size_t)sp + 3 * (size_t)nL));
    HIPCHK(pool.alloc(&d.Dinv, (size_t)nL * 9)); HIPCHK(pool.alloc(&d.db, (size_t)nL * 3));
    HIPCHK(pool.alloc(&d.e_chi2, (size_t)nE));             // (cleared below, where the call's first pass over the edges does not write it anyway)
    d.use_bsr = solver == 2 ? 1 : 0; d.bsr_max_row = bsr_max_row; d.nnzb = nnzb;
    if (want_pattern) { d.bsr_rowptr = f.bsr_rowptr; d.bsr_col = f.bsr_col; d.bsr_diag = f.bsr_diag; }
    if (use_pairs && nP > 0) {
        // pair lists of the deterministic Schur kernel, built on the device: count per block (+ the slot of the transposed block), scan, fill
        d.uinfo = reinterpret_cast<int4*>(f.uinfo); d.plm = f.plm; d.nu = f.nu;
        HIPCHK(pool.alloc(&d.pair_off, (size_t)d.nu + 1));
        size_t scan_ints = corb_scan_scratch_ints((size_t)d.nu);
        HIPCHK(pool.alloc(&d.scan_scratch, scan_ints));
        // block-sparse maps: the row-owner Schur kernel (pairs carry the first edge's position in its keyframe's list; see ba_schur_row_kernel)
        d.row_schur = (solver == 2 && d.lean && nP >= BA_ROW_MIN_POSES) ? 1 : 0;
#ifdef CORB_DEV
        const bool row_dbg = corb_dev_env("CORB_BA_ROWDBG") != nullptr;
#endif
        if (d.row_schur) {                                      // maps: Hpp | b_p from the edges' static data in keyframe-list order (no JB | r records: see ba_hpp_scratch_kernel)
            BAKfRec* kfrec = nullptr; HIPCHK(pool.alloc(&kfrec, (size_t)(nE ? nE : 1)));
            int n_pe = 0; HIPCHK(hipMemcpyAsync(&n_pe, d.poff + nP, sizeof(int), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
            if (n_pe > nE) { corb_set_error("corb_ba_solve: keyframe lists longer than the edge array"); return CORB_ERR_ARG; }
            ba_launch_kfrec(d, kfrec, n_pe, s);
            d.kfrec = kfrec; d.hpp_scratch = 1;
            // round 6: the V blocks in keyframe-list order (ba_v_kf_kernel) wherever the stream form of the row kernel runs; CORB_BA_V_EDGE keeps the edge order (A/B timing)
            static const bool v_edge = getenv("CORB_BA_V_EDGE") != nullptr || getenv("CORB_BA_ROW_UNITS") != nullptr;
            if (!v_edge) {
                int* vslot = nullptr; HIPCHK(pool.alloc(&vslot, (size_t)(nE ? nE : 1)));
                d.v_kf = 1; d.n_list = n_pe; d.vslot = vslot;
                ba_launch_vslot(d, vslot, nE, n_pe, s);
            }
        }
        if (d.row_schur) { HIPCHK(pool.alloc(&d.urow, (size_t)nP + 1)); HIPCHK(pool.alloc(&d.rr_off, (size_t)nP + 1)); HIPCHK(pool.alloc(&d.rowwb, (size_t)nP + 1)); ba_launch_row_structure(d, s); ba_launch_rr_count(d, s); }
    BA_TRACE("pairs_count");
        ba_launch_pairs_count(d, s);
        int n_pairs = 0; int2* dpairs = nullptr;
        if (f.pairs_bound > 0 && f.pairs_bound <= ((size_t)1 << 22) && !d.row_schur) {
            // local windows: the lists are allocated at the flattening's bound and the count travels with the call's first read-back -- no wait for it here
            HIPCHK(pool.alloc(&dpairs, f.pairs_bound));
            h_npairs = reinterpret_cast<int*>(static_cast<char*>(pool.pinned()) + 3072); *h_npairs = 0;
            HIPCHK(hipMemcpyAsync(h_npairs, d.pair_off + d.nu, sizeof(int), hipMemcpyDeviceToHost, s));
        } else {
        HIPCHK(hipMemcpyAsync(&n_pairs, d.pair_off + d.nu, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (n_pairs < 0) { corb_set_error("corb_ba_solve: more than 2^31 Schur pairs"); return CORB_ERR_ARG; }
        HIPCHK(pool.alloc(&dpairs, (size_t)(n_pairs ? n_pairs : 1)));
        }
        d.pairs = dpairs; r->schur_pairs = n_pairs;
    BA_TRACE("pairs_fill");
        ba_launch_pairs_fill(d, s);
        d.use_pairs = 1;
        if (d.row_schur) {                                      // work decomposition of the row kernel: workgroups (keyframe, range), units, tables
            int tot[2] = {0, 0};
            HIPCHK(hipMemcpyAsync(&tot[0], d.rr_off + nP, sizeof(int), hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(&tot[1], d.rowwb + nP, sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            d.n_wg = tot[0]; d.n_wb = tot[1];
            HIPCHK(pool.alloc(&d.wghdr, (size_t)d.n_wg)); HIPCHK(pool.alloc(&d.wb_off, (size_t)d.n_wg)); HIPCHK(pool.alloc(&d.wb_unit, (size_t)d.n_wb + 1));
            if (corb_scan_scratch_ints((size_t)d.n_wb) > scan_ints) { scan_ints = corb_scan_scratch_ints((size_t)d.n_wb); HIPCHK(pool.alloc(&d.scan_scratch, scan_ints)); }
            ba_launch_rr_units(d, false, s);
            HIPCHK(hipMemcpyAsync(&d.n_units, d.wb_unit + d.n_wb, sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            HIPCHK(pool.alloc(&d.units, (size_t)d.n_units + 1)); HIPCHK(pool.alloc(&d.upart, (size_t)d.n_units * 36 + 36)); HIPCHK(pool.alloc(&d.rpart, (size_t)d.n_wg * BA_ROW_WAVES * 6 + 6));
            ba_launch_rr_units(d, true, s);
            static const bool row_per_unit = getenv("CORB_BA_ROW_UNITS") != nullptr;       // (round 5's per-unit kernel, for A/B timing)
            if (!row_per_unit) {
                // round 6: every wavefront's rounds as one padded stream (ba_schur_row_stream_kernel)
                const size_t nwv = (size_t)d.n_wg * BA_ROW_WAVES;
                HIPCHK(pool.alloc(&d.wave_off, nwv + 1)); HIPCHK(pool.alloc(&d.wunit, (size_t)d.n_units + 1)); HIPCHK(pool.alloc(&d.wave_ucnt, (size_t)d.n_wg + 1));
                ba_launch_rr_stream(d, false, s);
                if (corb_scan_scratch_ints(nwv) > scan_ints) { scan_ints = corb_scan_scratch_ints(nwv); HIPCHK(pool.alloc(&d.scan_scratch, scan_ints)); }
                corb_launch_exclusive_scan(d.wave_off, d.wave_off, nwv, d.scan_scratch, s);
                int n_rounds = 0;
                HIPCHK(hipMemcpyAsync(&n_rounds, d.wave_off + nwv, sizeof(int), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                if (n_rounds < 0 || (size_t)n_rounds * 16 > ((size_t)1 << 31)) { corb_set_error("corb_ba_solve: more than 2^27 rounds of Schur pairs"); return CORB_ERR_ARG; }
                HIPCHK(pool.alloc(&d.row_stream, (size_t)n_rounds * 16 + 16));
                ba_launch_rr_stream(d, true, s);
            }
#ifdef CORB_DEV
            if (corb_dev_env("CORB_BA_ROWABL")) d.row_abl = atoi(corb_dev_env("CORB_BA_ROWABL"));
            if (row_dbg) { const size_t nw = (size_t)8 * ((d.n_wg + 7) / 8) * 8 * 8; HIPCHK(pool.alloc(&d.row_dbg, nw)); HIPCHK(hipMemsetAsync(d.row_dbg, 0, nw * 8, s)); }
#endif
        }
    }
    if (d.lean) HIPCHK(pool.alloc(&d.bd, (size_t)nE * 18));
    if (solver == 1) HIPCHK(pool.alloc(&d.S, (size_t)sp * sp));
    else {
        d.cg_nparts = (sp + 255) / 256 > 0 ? (sp + 255) / 256 : 1;
        d.pc_g = pc_g;
        if (pc_g > 1) {
            d.pc_gb = 6 * pc_g; d.pc_nblk = (nP + pc_g - 1) / pc_g;
            // the blocks (48 x 48 or 96 x 96) are inverted in registers (ba_pc_sweep_body) and left in single precision; the CG step reads their upper triangles
            // (pc_pack32, one workgroup per block) unless CORB_BA_PC_SQUARE asks for round 4's square form (a workgroup per 48 rows: for A/B timing)
            HIPCHK(pool.alloc(&d.pc_inv32, (size_t)d.pc_nblk * d.pc_gb * d.pc_gb));
            static const bool pc_square = getenv("CORB_BA_PC_SQUARE") != nullptr;
            d.pc_split = d.pc_gb / BA_PC_ROWS;
            if (!pc_square) { const int nt = d.pc_gb / 16; HIPCHK(pool.alloc(&d.pc_pack32, (size_t)d.pc_nblk * (nt * (nt + 1) / 2) * 256)); d.pc_split = 1; }
            d.cg_nparts = d.pc_nblk * d.pc_split;
            HIPCHK(pool.alloc(&d.pc_info, (size_t)2 * d.pc_nblk));
        }
        d.cg_nparts_spmv = 8 * std::max(1, ((nP + 3) / 4 + 7) / 8);          // a multiple of 8 workgroups: XCD x takes the x-th eighth of the block rows (ba_pcg_spmv_kernel)
        HIPCHK(pool.alloc(&d.bsr_val, (size_t)nnzb * 36)); HIPCHK(pool.alloc(&d.Minv, (size_t)nP * 36));
        { int* ts = nullptr; HIPCHK(pool.alloc(&ts, (size_t)nnzb + 1)); ba_launch_tslot(d, ts, s); d.bsr_tslot = ts; }
        HIPCHK(pool.alloc(&d.cg_r[0], (size_t)sp)); HIPCHK(pool.alloc(&d.cg_r[1], (size_t)sp)); HIPCHK(pool.alloc(&d.cg_z, (size_t)sp)); HIPCHK(pool.alloc(&d.cg_q, (size_t)sp));
        HIPCHK(pool.alloc(&d.cg_p[0], (size_t)sp)); HIPCHK(pool.alloc(&d.cg_p[1], (size_t)sp));
        HIPCHK(pool.alloc(&d.cg_part, (size_t)4 * d.cg_nparts + d.cg_nparts_spmv)); HIPCHK(pool.alloc(&d.cg_scal, 8)); HIPCHK(pool.alloc(&d.cg_flag, 2));
        // self-certification (ba_launch_true_residual): the right-hand side of the solve in progress, the residual kernel's partials, {max, last, |J'r|_inf}
        HIPCHK(pool.alloc(&cert_b, (size_t)sp)); HIPCHK(pool.alloc(&cert_part, (size_t)2 * ((sp + 255) / 256))); HIPCHK(pool.alloc(&cert_out, 4));
        HIPCHK(hipMemsetAsync(cert_out, 0, 4 * sizeof(double), s));
        d.cg_ngrp = (d.cg_nparts + 63) / 64; d.cg_ngrp_spmv = (d.cg_nparts_spmv + 63) / 64;
        HIPCHK(pool.alloc(&d.cg_part2, (size_t)4 * d.cg_ngrp + d.cg_ngrp_spmv)); HIPCHK(pool.alloc(&d.cg_tick, ((size_t)d.cg_ngrp + d.cg_ngrp_spmv + 2) * 64)); HIPCHK(pool.alloc(&d.cg_fin, 8));      // CG_TICK_STRIDE ints per ticket
        d.cg_two_level = (d.cg_nparts + d.cg_nparts_spmv > 3000 || getenv("CORB_BA_TWO_LEVEL")) ? 1 : 0;     // measured: 1 800 partials 59.5 vs 57.5 ms per 10 LM iterations, 3 750: 87.1 vs 92.0   // env: lets the tests run the large-system path on a small map
        // multilevel preconditioner on large maps (ba_multilevel.h): the consumers of r.z then read the final scalar only (the three-level reduction path)
        // (the hierarchy's host part is waited for where the first preconditioner set-up needs it -- ml_ready below, behind the first trial's Schur products)
        if (ch.multilevel && pc_g == BA_ML_G && want_pattern && ml_thread.joinable()) { ml_pending = true; d.cg_two_level = 1; }
    }
    }
    d.robust = robust ? 1 : 0; d.delta2 = delta2; d.delta3 = delta3;
    // small problems (local windows, small maps): the whole optimize() call is ONE kernel launch (ba_small_optimize_kernel), no rocSOLVER; an explicit
    // solver = 1 keeps the multi-kernel path.  pbStopFlag is honoured before the launch only -- such a call takes about a millisecond.
    lap("alloc + pair lists");
    hipEvent_t ev[10];
    for (int i = 0; i < 10; i++) ev[i] = pool.event(i);
    hipGraphExec_t pcg_graph[4] = {nullptr, nullptr, nullptr, nullptr};      // chunks of PCG_CHUNK, / 2, / 4, / 8 CG iterations (captured when first needed)
    int cg_pred = 0;                                    // CG iterations of this call's previous solve (they grow slowly from trial to trial): sizes the chunks
    const int PCG_CHUNK = d.cg_two_level ? 16 : 64;     // (50 000 keyframes, chunks of 8 / 12 / 16 / 24 / 32: 208.2 / 209.3 / 209-212 / 208.2 / 209.7 ms per 10 LM iterations: flat)     // CG iterations between two convergence read-backs: the kernels left over in a chunk after
                                                        // convergence return at once but still cost a dispatch each (~50 us per iteration at 50 000 keyframes)
    struct GraphGuard { hipGraphExec_t* g; ~GraphGuard() { for (int i = 0; i < 4; i++) if (g[i]) (void)hipGraphExecDestroy(g[i]); } } graph_guard{pcg_graph};
    // One reduced solve by PCG, or (resume) the continuation of the solve in progress to a tighter tolerance: the stop tolerance lives on the device (CG_TOL2), the
    // kernels of an iteration are the same at every tolerance, and a solve that has stopped at iteration t holds exactly the state iteration t starts from
    // (x, r, z, p_{t-1}, both r.z scalars: the kernel that sees |r| <= tol |b| returns before it writes anything) -- so tightening the tolerance and clearing
    // the flag takes the recurrence up where it stopped, with the Krylov space it has built (a restart from x would pay for it again).  The captured chunks
    // start at even parity: after an odd number of iterations one iteration is launched on its own.
    // CORB_BA_NO_GRAPH: the chunk's kernels are launched one by one instead of replayed as a captured hipGraph -- same kernels, same order, same
    // results.  For rocprofv3 runs: its kernel tracing dies (SIGSEGV inside hipGraphLaunch) after a few hundred launches of a captured graph,
    // which a 25 000-keyframe solve exceeds (chunks of 16 CG iterations); measured here, tools/gpu_profile_ba_store.sh sets it.
    // Chunks: the host reads the convergence flag between two chunks (a graph launch, a 16-byte read-back into page-locked memory, a wake-up: ~20 us), and the
    // iterations left over in a chunk after convergence return at once but still cost their dispatches (~12 us each on a mid-size map, ~50 on a large one).  The
    // previous solve's count predicts this one's: full chunks while more than a chunk is expected, then halves / quarters / eighths, then eighths until the
    // flag is up.  (One fixed size: a 1 200-keyframe map's 30 iterations per solve ran as two chunks of 16 + 8 dead iterations on average.)
    int cg_its_solve = 0;                               // CG iterations of the solve in progress (what a continuation starts from)
    int pcg_refined = 0;                                // trials whose solve was continued to the tight tolerance (default policy)
    auto cg_run = [&](bool resume, double tol, bool& ok2) -> int {
        static const bool no_graph = getenv("CORB_BA_NO_GRAPH") != nullptr;
        int* h_flags = reinterpret_cast<int*>(static_cast<char*>(pool.pinned()) + 512); double* h_its = reinterpret_cast<double*>(static_cast<char*>(pool.pinned()) + 528);
        int done = 0;
        if (!resume) {
            HIPCHK(hipMemcpyAsync(cert_b, d.x, (size_t)sp * sizeof(double), hipMemcpyDeviceToDevice, s));      // b_schur, before the solve consumes it
            ba_launch_pcg_init(d, tol, s);
            cg_its_solve = 0;
        } else {
            ba_launch_pcg_resume(d, tol, s);
            done = cg_its_solve;
            if (done & 1) { ba_launch_pcg_chunk(d, 1, s, 1); done++; }
        }
        h_flags[0] = h_flags[1] = 0; *h_its = (double)cg_its_solve;
        const int pred = resume ? 0 : cg_pred;
        while (done < pcg_max_iter && !h_flags[0] && !h_flags[1]) {
            const int left = pred > done ? pred - done : 0;
            int gi = 3;                                          // graph index: chunk of PCG_CHUNK >> gi iterations
            if (resume) gi = 1; else
            if (left >= PCG_CHUNK || pred == 0) gi = 0; else if (left >= PCG_CHUNK / 2) gi = 1; else if (left >= PCG_CHUNK / 4) gi = 2;
            const int n_it = std::max(2, PCG_CHUNK >> gi);
            if (!pcg_graph[gi] && !no_graph) {                 // capture a chunk of that size once, replay it
                hipGraph_t graph = nullptr;
    BA_TRACE("capture");
                HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
                ba_launch_pcg_chunk(d, n_it, s);
                HIPCHK(hipStreamEndCapture(s, &graph));
    BA_TRACE("instantiate");
                HIPCHK(hipGraphInstantiate(&pcg_graph[gi], graph, nullptr, nullptr, 0));
                (void)hipGraphDestroy(graph);
            }
    BA_TRACE("graph_launch");
            if (no_graph) ba_launch_pcg_chunk(d, n_it, s); else
            HIPCHK(hipGraphLaunch(pcg_graph[gi], s));
            HIPCHK(hipMemcpyAsync(h_flags, d.cg_flag, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(h_its, d.cg_scal + 4, sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            done += n_it;
        }
        ba_launch_true_residual(d, cert_b, cert_part, cert_out, s);      // |b - S x| / |b| of this solve, recomputed (read back once, at the end of the call)
        const int its = (int)*h_its;
        if (!resume) cg_pred = its + 2;
        r->pcg_iterations += its - cg_its_solve; cg_its_solve = its;
        ok2 = h_flags[0] && !h_flags[1];                           // converged, positive definite (Dinv finite: checked with the trial's read-back)
        return CORB_OK;
    };
    auto scalar = [&](int slot, double* out) -> int { HIPCHK(hipMemcpyAsync(out, d_scal + slot, sizeof(double), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); return CORB_OK; };
    auto chi2 = [&](double* out) -> int { ba_launch_error(d, d_partial, nparts, d_scal + 0, s); return scalar(0, out); };
    auto elapsed = [&](hipEvent_t a, hipEvent_t b) { float ms = 0; (void)hipEventElapsedTime(&ms, a, b); return (double)ms; };
    // phase times (ms_build / ms_schur / ms_solve / ms_update): six event records per trial, 17 % of a local window's call -- measured from 65 536
    // observations on (or with CORB_BA_TIMING=1); smaller calls report ms_total only
    const bool phase_ev = nE >= 65536 || timing;
    HIPCHK(hipEventRecord(ev[0], s));
    int it_done = 0, trials = 0;
    if (fused_small) HIPCHK(hipMemsetAsync(d.e_chi2, 0, sizeof(double) * (size_t)(nE ? nE : 1), s));
    if (fused_small && !(stop_flag && *stop_flag) && (nP + nL) > 0 && iterations > 0) {
        double* d_hist; int* d_cnt;                       // chi2 history | lambda history | the two counters (as one more double): one read-back
        HIPCHK(pool.alloc(&d_hist, (size_t)2 * iterations + 3)); d_cnt = reinterpret_cast<int*>(d_hist + 2 * iterations + 2);
        CorbBASmall a; a.iterations = iterations; a.state = dq; a.state_bak = dq_bak; a.n_state = n_state;
        a.chi2_hist = d_hist; a.lambda_hist = d_hist + iterations + 1; a.counters = d_cnt;
        ba_launch_small_optimize(d, a, s);
        std::vector<double> hist((size_t)2 * iterations + 3); int cnt[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(hist.data(), d_hist, hist.size() * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
        memcpy(cnt, &hist[(size_t)2 * iterations + 2], sizeof(cnt));
        it_done = cnt[0]; trials = cnt[1];
        if (r->chi2) for (int i = 0; i <= it_done; i++) r->chi2[i] = hist[i];
        if (r->lambda) for (int i = 0; i < it_done; i++) r->lambda[i] = hist[(size_t)iterations + 1 + i];
        r->solver_used = 1;
    } else {
    double cur = 0;
    double lambda = -1, ni = 2; int nBad = 0; bool ok = true;
    // The block inverses of the preconditioner are recomputed on every 3rd accepted LM trial and after every rejected one (lambda jumped): a stale
    // inverse is still symmetric positive definite, i.e. a valid preconditioner, and costs ~1 % more CG iterations (1 200 poses: a period of 5 is 2 %
    // faster over 10 LM iterations but 7 % slower over 5, where the first, large-lambda inverse then serves every trial; 50 000 poses, round 3, with the
    // blocks inverted in LDS at 2.7 ms per trial -- 0.39 ms since round 4's register form --: period 1 / 2 / 3 = 480 / 468 / 466 ms per 10 LM iterations, the solve itself 304.7 / 306.0 / 307.1).
    // With the multilevel preconditioner (round 4: its coarse levels age faster than the 16-keyframe blocks did alone, and a set-up is 1.6 ms instead of 8 since the blocks are
    // inverted in registers and the Galerkin products are gathers) the period is 2 -- 50 000 poses, device time per 10 LM iterations: period 1 / 2 / 3 / 5 = 204.0 / 202.5 / 207.5 /
    // 238.0 ms; separate periods for the fine blocks and the coarse levels (1 + 2, 1 + 3, 2 + 4) bought nothing over 2 + 2 (tools/gpu_ba_sweep.sh).
    int pc_age = 0; int pc_period = (d.ml || ml_pending) ? 2 : 3;
    if (const char* pe = corb_dev_env("CORB_BA_PC_PERIOD")) pc_period = std::max(1, atoi(pe));     // development aid (-DCORB_DEV builds only)
    // push(): the update kernel backs up the free vertices of every trial (up to BA_FUSED_UPDATE_BLOCKS workgroups); the fixed ones here, once
    const bool fused_update = n_upd_blocks <= BA_FUSED_UPDATE_BLOCKS && (nP + nL) > 0;
    if (fused_update && n_state) HIPCHK(hipMemcpyAsync(dq_bak, dq, n_state * 8, hipMemcpyDeviceToDevice, s));
    bool chi2_fresh = true;            // the per-edge chi2 on the device are those of the current estimates (first call above; an accepted trial)
    bool S_clean = false;              // S holds zeros outside the block pattern
    // Small calls (no phase events) are bound by the host round trip of every trial: the next iteration's linearisation is enqueued behind the trial's
    // read-back BEFORE the host waits for it, i.e. as if the trial were accepted (it nearly always is).  A rejected trial restores the estimates and
    // linearises them again -- the same numbers as before, the kernels are deterministic -- so the retry sees what g2o's retry sees.
    const bool speculate = !phase_ev;
    // Maps (phase events on), lean form: the same speculation with the trial's chi2 taken FROM the next linearisation -- ba_build_lean_kernel evaluates every edge's
    // error anyway -- instead of from a separate pass over the edges (0.8 ms per trial at 27.5 M observations); the host waits for that launch.
    double* d_chi_partial = reuse ? work->d_chi_partial : nullptr;
    if (!reuse && d.lean && ba_build_lean_blocks(d) > 0) HIPCHK(pool.alloc(&d_chi_partial, (size_t)ba_build_lean_blocks(d)));      // (also the chains of a local window, below)
    bool built = false;                // the linearisation of the current estimates is already enqueued
    const bool small_solve = solver == 1 && sp > 0 && sp <= 128;   // local windows: one workgroup in LDS, S is left alone
    // Local windows: a trial is ~70 us of kernels, the host's turn-around between two trials (wake-up, the next trial's launches) about as much.  The host enqueues
    // CHAINS of iterations whose accept / lambda / stop-rule decisions are taken on the device (BALMCtl, ba_lm_ctl_kernel) and reads the outcome once per chain; a trial
    // that is not accepted stops its chain and is repeated by the loop below from the estimates before it (the kernels are deterministic: the repeat sees the same
    // numbers).  The first chain of a call starts with the call itself (round 5: the chi2 of the start estimates, the first linearisation and computeLambdaInit stay on
    // the device -- ba_lm_begin_kernel -- where the host loop reads chi2, the largest diagonal entry and the first trial back one after the other).  pbStopFlag is looked
    // at when a chain is enqueued (a chain of BA_LM_CHAIN iterations runs ~0.35 ms).
    static const bool no_chain = getenv("CORB_BA_NO_CHAIN") != nullptr;       // (the host-driven loop alone: for A/B timing)
    static const int chain_len = getenv("CORB_BA_CHAIN") ? std::max(1, std::min(BA_CHAIN_MAX, atoi(getenv("CORB_BA_CHAIN")))) : BA_LM_CHAIN;      // (for A/B timing)
    const bool chain_ok = solver == 1 && small_solve && fused_update && d.lean && !phase_ev && sp > 0 && !no_chain;
    BALMCtl* d_ctl = reuse ? work->d_ctl : nullptr;
    if (chain_ok && !d_ctl) HIPCHK(pool.alloc(&d_ctl, 1));
    if (work && !work->ready && solver == 1 && !fused_small) { work->d = d; work->d_partial = d_partial; work->d_scal = d_scal; work->d_chi_partial = d_chi_partial; work->d_ctl = d_ctl; work->ready = true; }
    bool chain_begin = chain_ok && iterations > 0 && (nP + nL) > 0 && !(stop_flag && *stop_flag);      // the call's first iteration runs inside a chain
    if (!chain_begin) {
    BA_TRACE("chi2");
        HIPCHK(hipMemsetAsync(d.e_chi2, 0, sizeof(double) * (size_t)(nE ? nE : 1), s));      // (a begin chain's first kernel writes every edge's chi2)
        rc = chi2(&cur); if (rc) return rc;
        if (r->chi2) r->chi2[0] = cur;
    }
    for (int it = 0; it < iterations && !(stop_flag && *stop_flag) && ok && (nP + nL) > 0; it++) {
        if (chain_ok && (it > 0 || chain_begin) && chi2_fresh) {
            const bool begin = chain_begin; chain_begin = false;
            const int nb = std::min(iterations - it, chain_len);
            BALMCtl* hc = reinterpret_cast<BALMCtl*>(static_cast<char*>(pool.pinned()) + 1024);
            BALMCtl* hr = reinterpret_cast<BALMCtl*>(static_cast<char*>(pool.pinned()) + 2048);
            memset(hc, 0, sizeof(BALMCtl));
            hc->lambda = lambda; hc->ni = ni; hc->currentChi = cur; hc->nBad = nBad; hc->iterations = nb; hc->begin = begin ? 1 : 0;
            HIPCHK(hipMemcpyAsync(d_ctl, hc, sizeof(BALMCtl), hipMemcpyHostToDevice, s));
            CorbBADev dc = d; dc.ctl = d_ctl;
            if (begin) {                                              // computeActiveErrors, the first linearisation, computeLambdaInit
                ba_launch_error(dc, d_partial, nparts, d_scal + 0, s);
                ba_launch_build(dc, d_scal + 1, s);
                ba_launch_lm_begin(dc, d_scal, s);
                built = true;
            }
            for (int j = 0; j < nb; j++) {
                const int epoch = trials + j + 1;
                if (j == 0 && !built) ba_launch_build(dc, nullptr, s);
                ba_launch_schur(dc, lambda, d_bad, epoch, !(S_clean && small_solve), s); S_clean = true;        // (lambda: the device's, see BALMCtl)
                ba_launch_small_solve(dc, d_info, s);
                ba_launch_backsub_update(dc, lambda, d_partial, nparts, d_scal + 2, dq, dq_bak, n_state, s);
                // the trial's chi2 comes from the next iteration's linearisation (one launch less per trial); a trial that is not accepted stops the chain, and the
                // host loop restores the estimates and linearises them again
                const bool nxt = it + j + 1 < iterations;
                // ... and the trial's decision (BALMCtl) is taken by the thread of that launch that files the chi2 (round 5: one launch less per trial)
                static const bool ctl_launch = getenv("CORB_BA_CTL_LAUNCH") != nullptr;      // (the decision as its own one-thread launch, as in round 4: for A/B timing)
                const int* cb = ctl_launch ? nullptr : d_bad;
                if (nxt && d_chi_partial) ba_launch_build(dc, nullptr, s, d_chi_partial, d_scal + 0, cb, epoch);
                else ba_launch_error(dc, d_partial, nparts, d_scal + 0, s, cb, epoch);
                if (ctl_launch) ba_launch_lm_ctl(dc, d_scal, d_bad, epoch, s);
                if (nxt && !d_chi_partial) ba_launch_build(dc, nullptr, s);
            }
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(hr, d_ctl, sizeof(BALMCtl), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            const int m = hr->it_done;
            if (begin && r->chi2) r->chi2[0] = hr->chi0;
            for (int k = 0; k < m; k++) { it_done++; if (r->chi2) r->chi2[it_done] = hr->chi2_hist[k]; if (r->lambda) r->lambda[it_done - 1] = hr->lambda_hist[k]; }
            trials += hr->trials; lambda = hr->lambda; ni = hr->ni; nBad = hr->nBad; cur = hr->currentChi;
            if (hr->stop == 2) { ok = false; continue; }                                    // nBad >= 3 (Optimizer's stop rule)
            if (hr->stop != 3) { built = it + m < iterations; chi2_fresh = true; it += m - 1; continue; }
            // a trial of iteration it + m was not accepted (or its solve failed): the estimates before it, and the host loop from there
            HIPCHK(hipMemcpyAsync(dq, dq_bak, n_state * 8, hipMemcpyDeviceToDevice, s));
            chi2_fresh = false; built = false; it += m;
        }
        // computeActiveErrors(): the state is the one whose chi2 the host already holds (initial value or the last accepted trial), so
        // the kernel only refreshes the per-edge chi2 (g2o's stale _error semantics) -- no read-back, no synchronisation
        double currentChi = cur;
        if (!chi2_fresh) { ba_launch_error(d, d_partial, nparts, d_scal + 0, s); chi2_fresh = true; }      // (after a rejected trial: the values on the device are the trial's)
        const double iniChi = currentChi; double tempChi = currentChi;
        if (phase_ev) HIPCHK(hipEventRecord(ev[1], s));
    BA_TRACE("build");
        if (!built) ba_launch_build(d, it == 0 ? d_scal + 1 : nullptr, s);
        built = false;
        if (phase_ev) HIPCHK(hipEventRecord(ev[2], s));
        bool build_timed = false;
        if (it == 0) { double maxDiag; rc = scalar(1, &maxDiag); if (rc) return rc; lambda = 1e-5 * maxDiag; ni = 2; nBad = 0; if (phase_ev) r->ms_build += elapsed(ev[1], ev[2]); build_timed = true; }   // computeLambdaInit, _tau = 1e-5
        double rho = 0; int qmax = 0;
        do {
            if (pc_age >= pc_period) pc_age = 0;
            const int epoch = trials + 1;                                  // what a failing kernel leaves in d_bad[0]
    BA_TRACE("schur_bsr");
            if (phase_ev) HIPCHK(hipEventRecord(ev[6], s));
            if (solver == 1) { ba_launch_schur(d, lambda, d_bad, epoch, !(S_clean && small_solve), s); S_clean = true; HIPCHK(hipGetLastError()); }       // setLambda + Schur complement (block_solver.hpp:371-431)
            else {
                // the call's first trial: the Schur products are enqueued, THEN the host waits for the hierarchy (its ~15 ms at 50 000 keyframes ran beside the pair-list
                // kernels, the first chi2 / linearisation and these products), uploads it and enqueues the preconditioner's set-up
                if (ba_launch_schur_bsr(d, lambda, nnzb, d_bad, epoch, s, ml_pending ? 0 : pc_age == 0)) { corb_set_error("preconditioner blocks larger than 128 x 128"); return CORB_ERR_ARG; }
                if (ml_pending) {
                    ml_pending = false;
                    if (ml_thread.joinable()) ml_thread.join();
                    if (timing) lap("LM start .. hierarchy joined");
                    rc = ba_ml_upload(pool, nP, ml_host, ml); if (rc) return rc;
                    if (ml.L > 0) { d.ml = &ml; r->pc_levels = ml.L; }
                    if (ba_launch_pc_refresh(d, s)) { corb_set_error("preconditioner blocks larger than 128 x 128"); return CORB_ERR_ARG; }
                }
            }
            if (phase_ev) HIPCHK(hipEventRecord(ev[7], s));
#ifdef CORB_DEV
            if (d.row_dbg && trials == 1) {                    // development aid: where a row workgroup's time goes (cycle stamps of every wavefront of the 2nd trial)
                const size_t nw = (size_t)8 * ((d.n_wg + 7) / 8) * 8;
                std::vector<long long> ts(nw * 8);
                HIPCHK(hipStreamSynchronize(s)); HIPCHK(hipMemcpy(ts.data(), d.row_dbg, ts.size() * 8, hipMemcpyDeviceToHost));
                double sum[8] = {0}; double cnt = 0, cnt5 = 0, sum5 = 0, pairs = 0; double wgspan = 0; size_t nwg = 0;
                for (size_t g = 0; g < nw / 8; g++) {
                    long long lo = 0, hi = 0;
                    for (int w = 0; w < 8; w++) {
                        const long long* t = &ts[(g * 8 + w) * 8];
                        if (!t[0] || !t[3]) continue;
                        if (!lo || t[0] < lo) lo = t[0];
                        const long long e = t[5] ? t[5] : t[4] ? t[4] : t[3]; if (e > hi) hi = e;
                        if (t[4]) { for (int i = 1; i <= 4; i++) sum[i] += (double)(t[i] - t[i - 1]); cnt++; pairs += (double)t[7]; }
                        if (t[5]) { sum5 += (double)(t[5] - t[4]); cnt5++; }
                    }
                    if (lo && hi) { wgspan += (double)(hi - lo); nwg++; }
                }
                fprintf(stderr, "[row_dbg] wavefronts with a block %.0f: hdr+list %.0f  pieces+blockhdr issue %.0f  prologue issue %.0f  barrier wait %.0f  first block %.0f (pairs %.1f) | later turns %.0f x %.0f | workgroup span %.0f cycles (%zu workgroups)\n",
                        cnt, 0.0, sum[1] / cnt, sum[2] / cnt, sum[3] / cnt, sum[4] / cnt, pairs / cnt, cnt5, cnt5 ? sum5 / cnt5 : 0.0, wgspan / (nwg ? nwg : 1), nwg);
            }
#endif
            bool ok2 = true;
            if (sp > 0 && solver == 1) {                               // LinearSolver: S x_p = b_schur (dense Cholesky); the launches are enqueued,
                                                                       // the factorisation status is read back together with the trial's scalars
                if (small_solve) { ba_launch_small_solve(d, d_info, s); HIPCHK(hipGetLastError()); }      // local windows: one workgroup in LDS; a launch that fails must not leave a stale info word
                else {
                // hand-written blocked Cholesky + substitutions (dense_chol.hip: 3.4 ms per solve at 320 keyframes, rocSOLVER's dpotrf + dpotrs took 6; replaying
                // the 2 launches per panel as a captured hipGraph measured the same -- the panels' dependent chains, not the launches, are the time)
                if (!chol_ws) HIPCHK(pool.alloc(&chol_ws, corb_chol_workspace_doubles(sp)));      // (the panels' diagonal factors: dense_chol.h)
                corb_launch_chol_solve(d.S, sp, sp, d.x, d_info, chol_ws, s);
                HIPCHK(hipGetLastError());
                }
            } else if (sp > 0) {                                       // block-Jacobi preconditioned CG on the BSR system
    BA_TRACE("pcg_init");
                rc = cg_run(false, pcg_tol, ok2); if (rc) return rc;
            }
            bool built_ahead = false;
            for (int attempt = 0;; attempt++) {
            if (phase_ev) HIPCHK(hipEventRecord(ev[3], s));
            // back-substitution, oplus, the trial's chi2: enqueued unconditionally, ONE read-back per trial
            ba_launch_backsub_update(d, lambda, d_partial, nparts, d_scal + 2, dq, dq_bak, n_state, s);       // (with push(): the estimates are backed up first)
            if (phase_ev) HIPCHK(hipEventRecord(ev[4], s));
            const bool fuse_chi = d_chi_partial && phase_ev && it + 1 < iterations;
            if (fuse_chi) {
                HIPCHK(hipEventRecord(ev[8], s));
                ba_launch_build(d, nullptr, s, d_chi_partial, d_scal + 0);
                HIPCHK(hipEventRecord(ev[9], s));
            } else
            ba_launch_error(d, d_partial, nparts, d_scal + 0, s);
            double* h_stat = static_cast<double*>(pool.pinned());      // page-locked: the copy is enqueued, the host goes on to enqueue the next linearisation
            HIPCHK(hipMemcpyAsync(h_stat, d_scal, 7 * sizeof(double), hipMemcpyDeviceToHost, s));
            const bool spec = speculate && it + 1 < iterations;
            built_ahead = spec || fuse_chi;
            if (spec) {
                HIPCHK(hipEventRecord(ev[1], s));
                ba_launch_build(d, nullptr, s);
                HIPCHK(hipEventSynchronize(ev[1]));
            } else
            HIPCHK(hipStreamSynchronize(s));
            int h_bad[2]; memcpy(h_bad, &h_stat[6], sizeof(h_bad));
            if (h_bad[0] == epoch || (solver == 1 && h_bad[1] != 0)) ok2 = false;          // Dinv not finite / not positive definite => solve() returns false
            double scale = 0;
            if (ok2) { scale = h_stat[2]; tempChi = h_stat[0]; }
            else tempChi = DBL_MAX;                                    // (the update applied a meaningless step: it is rejected and undone below)
            if (phase_ev) {
            if (!build_timed) { r->ms_build += elapsed(ev[1], ev[2]); build_timed = true; }
            if (fuse_chi) r->ms_build += elapsed(ev[8], ev[9]);          // (the next iteration's linearisation + this trial's chi2)
            r->ms_update += elapsed(ev[3], ev[4]);
            if (attempt == 0) r->ms_schur += elapsed(ev[6], ev[7]);
            r->ms_solve += elapsed(ev[7], ev[3]);
            }
            rho = currentChi - tempChi;
            scale += 1e-3;
            rho /= scale;
            // The default tolerance policy (BAChoice): what a loose solve must not change is a DECISION of the LM loop.  rho decides accept / reject (rho > 0) and
            // the lambda factor max(1/3, min(2/3, 1 - (2 rho - 1)^3)), which is constant (2/3) below rho = 0.847 and (1/3) above 0.937 and steep in between.  A trial
            // whose rho, as the loose solve gives it, lies near zero or in / near that window -- or whose predicted decrease is so small against chi2 that the loose
            // solve's error in chi2 (~0.03 tol chi2, profiles/r05_pcg_tol_sweep.txt) could move rho across a margin -- is solved AGAIN: the estimates are restored,
            // the same CG recurrence continues to the tight tolerance, update and chi2 are redone, and the decision is taken from those.
            if (attempt == 0 && ch.pcg_forcing && solver == 2 && sp > 0 && ok2 && pcg_tol > BA_PCG_TOL_TIGHT &&
                (!(rho > 0.05) || (rho > 0.80 && rho < 0.97) || !(pcg_tol * currentChi < 0.3 * scale) || !std::isfinite(tempChi))) {
                HIPCHK(hipMemcpyAsync(dq, dq_bak, n_state * 8, hipMemcpyDeviceToDevice, s));
                if (built_ahead) ba_launch_build(d, nullptr, s);      // (computeScale reads b: the linearisation of the restored estimates again)
                if (phase_ev) HIPCHK(hipEventRecord(ev[7], s));
                rc = cg_run(true, BA_PCG_TOL_TIGHT, ok2); if (rc) return rc;
                pcg_refined++;
                continue;
            }
            break;
            }
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = 1. - std::pow((2 * rho - 1), 3);
                alpha = std::min(alpha, 2. / 3.);
                if (ch.pcg_forcing) pcg_tol = std::min(tol_loose, std::max(BA_PCG_TOL_TIGHT, 1e-2 * (currentChi - tempChi) / currentChi));    // (BAChoice: the next iteration's tolerance)
                lambda *= std::max(1. / 3., alpha); ni = 2; currentChi = tempChi; cur = tempChi;      // discardTop()
                pc_age++; chi2_fresh = true; built = built_ahead;
            } else {
                lambda *= ni; ni *= 2;                                                 // pop()
                pc_age = 0; chi2_fresh = false;
                HIPCHK(hipMemcpyAsync(dq, dq_bak, n_state * 8, hipMemcpyDeviceToDevice, s));
                if (!ok2) { ba_launch_error(d, d_partial, nparts, d_scal + 0, s); chi2_fresh = true; }        // failed solve: g2o evaluated the errors at the unchanged state
                if (built_ahead) ba_launch_build(d, nullptr, s);                        // the speculative linearisation was the rejected estimates'
            }
            qmax++; trials++;
        } while (rho < 0 && qmax < 10 && !(stop_flag && *stop_flag));
        it_done++;
        if (r->chi2) r->chi2[it_done] = currentChi;
        if (r->lambda) r->lambda[it_done - 1] = lambda;
        if (qmax == 10 || rho == 0) { ok = false; continue; }                          // Terminate
        if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;               // ORB-SLAM2 stop rule (:155-161)
        if (nBad >= 3) ok = false;
    }
    }
    HIPCHK(hipEventRecord(ev[5], s));
    if (cert_out && nE > 0 && (nP + nL) > 0) {
        // what the call certifies about itself: the true residuals of its reduced solves and |J'r|_inf = |b|_inf of a linearisation at the estimates it returns
        // (outside the timed span: ms_total is the optimisation's)
        double* h_cert = reinterpret_cast<double*>(static_cast<char*>(pool.pinned()) + 640);
        ba_launch_build(d, nullptr, s);
        ba_launch_absmax(d.b, (size_t)sp + 3 * (size_t)nL, cert_out + 2, s);
        HIPCHK(hipMemcpyAsync(h_cert, cert_out, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (!(h_cert[0] <= r->pcg_residual_max)) r->pcg_residual_max = h_cert[0];
        r->pcg_residual_last = h_cert[1]; r->grad_inf = h_cert[2]; r->pcg_refined_trials += pcg_refined;
    }
    HIPCHK(hipStreamSynchronize(s)); lap("LM iterations");
    if (h_npairs) {
        if (*h_npairs < 0 || (size_t)*h_npairs > f.pairs_bound) { corb_set_error("corb_ba_solve: %d Schur pairs beyond the flattening's bound %zu", *h_npairs, f.pairs_bound); return CORB_ERR_HIP; }
        r->schur_pairs = *h_npairs; if (work && work->ready) work->n_pairs = *h_npairs;
    } else if (reuse) r->schur_pairs = work->n_pairs;
    else if (work && work->ready) work->n_pairs = (int)r->schur_pairs;
    r->ms_total += elapsed(ev[0], ev[5]);
    r->iters_done += it_done; r->trials_total += trials;
    if (e_chi2_out) *e_chi2_out = d.e_chi2;
    return CORB_OK;
}

// A staged call (LocalBundleAdjustment: optimize(5), classify, optimize(10)) used to flatten, upload and build the pair lists once per optimize(): with
// a session the device-resident graph of the FIRST optimize() -- which has every edge active -- serves the later ones: an edge that a classification
// switched off keeps its place with the weight 0 (J = 0, r = 0, V = 0: it adds exact zeros in the same places of the same sums, i.e. the estimates are
// those of the re-flattened graph up to the rounding of a zero update of vertices left without an active edge), only the weights and the estimates travel.
// Round 5: with want_dev the classifications between the optimize() calls run on the device as well (ba_stage_classify_kernel: the active sets, the chi2 every edge
// had when it last was active and the masked weights stay in device memory), so a staged solve reads NOTHING back until its end -- a local window's call was
// bound by those round trips (per optimize(): estimates + per-edge chi2 down, fresh chi2 + depth down, weights + estimates up).
struct BASession {
    std::unique_ptr<Pool> pool; BAFlat f; BAChoice ch; bool ready = false;
    std::vector<int> act;             // flattened edge j = edge act[j] of the problem
    std::vector<double> e_w0;         // its information scale
    bool covers_all = false;          // every edge of the problem is in the graph (none between two fixed vertices)
    LMWork work;                      // the first optimize()'s work arrays and pair lists (local windows)
    bool want_dev = false, dev = false;
    int n_sets = 0, cur_set = 0;      // active sets on the device: set 0 = every edge (the first optimize()), set k + 1 = after the k-th classification
    double *d_w0 = nullptr, *d_last = nullptr, *d_e_chi2 = nullptr; unsigned char* d_act = nullptr;
};
// dev sessions: optimize(iterations) on the estimates / weights the device holds
static int ba_optimize_session_dev(BASession& S, int iterations, int robust, volatile int* stop_flag, CorbBAResult* r, double delta2, double delta3)
{
    Lap lap;
    double* d_e_chi2 = nullptr;
    int rc = ba_lm_device(*S.pool, S.f, S.ch, iterations, robust, stop_flag, r, delta2, delta3, lap, &d_e_chi2, &S.work);
    S.d_e_chi2 = d_e_chi2;
    return rc;
}
// dev sessions: the classification after an optimize() call (corb_ba_solve_staged's loop over the edges), set cur_set -> cur_set + 1
static int ba_classify_session_dev(BASession& S, const CorbBAStage& cs)
{
    BAFlat& f = S.f; Pool& pool = *S.pool;
    if (S.cur_set + 1 >= S.n_sets) { corb_set_error("corb_ba_solve_staged: more classifications than stages"); return CORB_ERR_ARG; }
    auto th_double = [](float t) { return std::round((double)t * 1e6) / 1e6; };
    CorbBADev d; memset(&d, 0, sizeof(d));
    d.nE = f.nE; d.e_vpose = f.e_vpose; d.e_vpoint = f.e_vpoint; d.e_obs = f.e_obs; d.e_w = S.d_w0; d.e_dim = f.e_dim;
    d.pose_q = f.dq; d.pose_t = f.dq + f.n_q; d.pt = f.dq + f.n_q + f.n_t; d.cam = f.cam; d.e_chi2 = S.d_e_chi2;
    BAStageDev a; memset(&a, 0, sizeof(a));
    a.last = S.d_last; a.w0 = S.d_w0; a.e_w = f.e_w;
    a.act_in = S.cur_set == 0 ? nullptr : S.d_act + (size_t)S.cur_set * f.nE; a.act_out = S.d_act + (size_t)(S.cur_set + 1) * f.nE;
    a.th_mono = cs.chi2_mono; a.th_stereo = cs.chi2_stereo; a.thd_mono = th_double(cs.chi2_mono); a.thd_stereo = th_double(cs.chi2_stereo);
    a.check_depth = cs.check_depth; a.recompute_inactive = cs.recompute_inactive; a.allow_reactivate = cs.allow_reactivate; a.float_compare = cs.float_compare;
    ba_launch_stage_classify(d, a, pool.stream);
    HIPCHK(hipGetLastError());
    S.cur_set++;
    return CORB_OK;
}

// optimize(iterations) on the session's graph: the estimates in, the weights of the active set in, LM, the estimates (and per-edge chi2) out
static int ba_optimize_session(const CorbBAProblem* p, const uint8_t* active, BAState& st, int iterations, int robust, volatile int* stop_flag, CorbBAResult* r,
                               BASession& S, std::vector<double>* last_chi2, std::vector<uint8_t>* pose_touched, std::vector<uint8_t>* pt_touched, double delta2, double delta3)
{
    Lap lap;
    Pool& pool = *S.pool; BAFlat& f = S.f;
    const int nE = f.nE;
    const size_t n_state = f.n_q + f.n_t + f.n_pt;
    static thread_local std::vector<double> blob;
    blob.resize((size_t)nE + n_state + 1);
    int n_active = 0;
    for (int j = 0; j < nE; j++) {
        const int i = S.act[j]; const bool on = !active || active[i];
        blob[j] = on ? S.e_w0[j] : 0.0;
        if (on) { n_active++; const CorbBAEdge& e = p->edges[i]; if (pose_touched) (*pose_touched)[e.pose] = 1; if (pt_touched) (*pt_touched)[e.point] = 1; }
    }
    double* stp = blob.data() + nE;
    if (f.n_q) memcpy(stp, st.q.data(), f.n_q * 8);
    if (f.n_t) memcpy(stp + f.n_q, st.t.data(), f.n_t * 8);
    if (f.n_pt) memcpy(stp + f.n_q + f.n_t, st.pt.data(), f.n_pt * 8);
    if (nE) HIPCHK(pool.h2d(f.e_w, blob.data(), (size_t)nE * 8));
    if (n_state) HIPCHK(pool.h2d(f.dq, stp, n_state * 8));
    r->active_edges = n_active;
    lap("session: weights + estimates");
    double* d_e_chi2 = nullptr;
    int rc = ba_lm_device(pool, f, S.ch, iterations, robust, stop_flag, r, delta2, delta3, lap, &d_e_chi2, &S.work);
    if (rc) return rc;
    std::vector<double> ec; if (last_chi2 && nE > 0) ec.resize(nE);
    static thread_local std::vector<double> back; back.resize(n_state ? n_state : 1);
    if (n_state) HIPCHK(pool.d2h(back.data(), f.dq, n_state * 8));
    if (!ec.empty()) HIPCHK(pool.d2h(ec.data(), d_e_chi2, sizeof(double) * (size_t)nE));
    HIPCHK(pool.fetch_finish());
    if (f.n_q) memcpy(st.q.data(), back.data(), f.n_q * 8);
    if (f.n_t) memcpy(st.t.data(), back.data() + f.n_q, f.n_t * 8);
    if (f.n_pt) memcpy(st.pt.data(), back.data() + f.n_q + f.n_t, f.n_pt * 8);
    for (int j = 0; j < (int)ec.size(); j++) if (!active || active[S.act[j]]) (*last_chi2)[S.act[j]] = ec[j];      // (an edge that is switched off has no computeError())
    lap("session: read back");
    return CORB_OK;
}

// e->computeError(), chi2 and the depth test of EVERY edge at the session's current estimates (the classification between / after the optimize() calls)
static int ba_eval_session(const CorbBAProblem* p, BASession& S, std::vector<double>& chi2, std::vector<double>& depth)
{
    const int E = p->n_edges; BAFlat& f = S.f; Pool& pool = *S.pool;
    chi2.assign(E ? E : 1, 0.0); depth.assign(E ? E : 1, 0.0);
    if (f.nE == 0) return CORB_OK;
    double *dw0, *dchi, *ddep;
    HIPCHK(pool.alloc(&dw0, (size_t)f.nE)); HIPCHK(pool.alloc(&dchi, (size_t)2 * f.nE)); ddep = dchi + f.nE;
    HIPCHK(pool.h2d(dw0, S.e_w0.data(), (size_t)f.nE * 8));
    CorbBADev d; memset(&d, 0, sizeof(d));
    d.nE = f.nE; d.e_vpose = f.e_vpose; d.e_vpoint = f.e_vpoint; d.e_obs = f.e_obs; d.e_w = dw0; d.e_dim = f.e_dim;
    d.pose_q = f.dq; d.pose_t = f.dq + f.n_q; d.pt = f.dq + f.n_q + f.n_t; d.cam = f.cam;
    ba_launch_edge_eval(d, dchi, ddep, pool.stream);
    HIPCHK(hipGetLastError());
    std::vector<double> both((size_t)2 * f.nE);
    HIPCHK(pool.d2h(both.data(), dchi, sizeof(double) * (size_t)2 * f.nE));
    HIPCHK(pool.fetch_finish());
    for (int j = 0; j < f.nE; j++) { chi2[S.act[j]] = both[j]; depth[S.act[j]] = both[(size_t)f.nE + j]; }
    return CORB_OK;
}

// optimizer.initializeOptimization(0) + optimize(iterations) over the edges with active[i] != 0 (NULL = all), from and to
// the double-precision state.  last_chi2 (orig-indexed, optional) receives chi2 of every computeError() on an active edge.
int ba_optimize_device(const CorbBAProblem* p, const uint8_t* active, BAState& st, int iterations, int robust, volatile int* stop_flag,
                       CorbBAResult* r, int device, const CorbBAOptions* opt, std::vector<double>* last_chi2,
                       std::vector<uint8_t>* pose_touched, std::vector<uint8_t>* pt_touched, double delta2, double delta3, BASession* sess = nullptr)
{
    if (sess && sess->ready) return ba_optimize_session(p, active, st, iterations, robust, stop_flag, r, *sess, last_chi2, pose_touched, pt_touched, delta2, delta3);
    const int K = p->n_poses, M = p->n_points;
    int rc = CORB_OK;
    Lap lap;
    // ---- graph flattening ----
    // host staging vectors live per thread and keep their capacity: at 16 M observations most of the flattening time was first-touch page
    // faults of freshly allocated vectors (every element below is (re)written on every call)
    struct HostScratch { std::vector<int> deg, act, pidx, lidx, pose_vertex, point_vertex, cnt, sorted, e_pose, e_point, e_vpose, e_vpoint, loff, lnfree, poff, pedge,
                                          bsr_rowptr, bsr_col, bsr_diag, uinfo, plm, stamp, cols, cur, keys; std::vector<double> e_obs, e_w; std::vector<unsigned char> e_dim; };
    static thread_local HostScratch hs;
    std::vector<int>& deg = hs.deg; deg.assign(M, 0);
    std::vector<int>& act = hs.act; act.clear();             // active edges (allVerticesFixed dropped, sparse_optimizer.cpp:234)
    const int NT0 = ba_host_threads((size_t)p->n_edges, true);
    if (NT0 > 1) {
        // every thread filters its range of edges; the ranges are concatenated in order, so `act` is ascending like the serial loop's
        std::vector<std::vector<int>> part(NT0);
        parallel_ranges((size_t)p->n_edges, NT0, [&](int t, size_t ib, size_t ie) {
            std::vector<int>& mine = part[t]; mine.reserve(ie - ib);
            for (size_t i = ib; i < ie; i++) {
                const CorbBAEdge& e = p->edges[i];
                if (active && !active[i]) continue;
                if (p->pose_fixed[e.pose] && p->point_fixed[e.point]) continue;
                mine.push_back((int)i); __atomic_store_n(&deg[e.point], 1, __ATOMIC_RELAXED);      // only "has an edge" is used
                if (pose_touched) __atomic_store_n(&(*pose_touched)[e.pose], (uint8_t)1, __ATOMIC_RELAXED);
                if (pt_touched) __atomic_store_n(&(*pt_touched)[e.point], (uint8_t)1, __ATOMIC_RELAXED);
            }
        });
        size_t tot = 0; std::vector<size_t> at(NT0);
        for (int t = 0; t < NT0; t++) { at[t] = tot; tot += part[t].size(); }
        act.resize(tot);
        parallel_ranges((size_t)NT0, NT0, [&](int, size_t tb, size_t te) { for (size_t t = tb; t < te; t++) if (!part[t].empty()) memcpy(act.data() + at[t], part[t].data(), part[t].size() * sizeof(int)); });
    } else
    for (int i = 0; i < p->n_edges; i++) {
        const CorbBAEdge& e = p->edges[i];
        if (active && !active[i]) continue;
        if (p->pose_fixed[e.pose] && p->point_fixed[e.point]) continue;
        act.push_back(i); deg[e.point]++;
        if (pose_touched) (*pose_touched)[e.pose] = 1;
        if (pt_touched) (*pt_touched)[e.point] = 1;
    }
    std::vector<int>& pidx = hs.pidx; std::vector<int>& lidx = hs.lidx; std::vector<int>& pose_vertex = hs.pose_vertex; std::vector<int>& point_vertex = hs.point_vertex;
    pidx.resize(K); lidx.resize(M); pose_vertex.clear(); point_vertex.clear();
    for (int k = 0; k < K; k++) { pidx[k] = p->pose_fixed[k] ? -1 : (int)pose_vertex.size(); if (pidx[k] >= 0) pose_vertex.push_back(k); }
    for (int m = 0; m < M; m++) { lidx[m] = (p->point_fixed[m] || deg[m] == 0) ? -1 : (int)point_vertex.size(); if (lidx[m] >= 0) point_vertex.push_back(m); }   // points without edges are removed (Optimizer.cc:198-202)
    const int nP = (int)pose_vertex.size(), nL = (int)point_vertex.size(), sp = 6 * nP;
    int solver = opt ? opt->solver : 0;
    if (solver < 0 || solver > 2) { corb_set_error("corb_ba_solve: bad solver option"); return CORB_ERR_ARG; }
    if (solver == 0) solver = nP <= 256 ? 1 : 2;            // tools/ba_solver_sweep.py (round 3, dense_chol.hip: 17 / 36 / 62 ms per 10 iterations at 160 / 320 / 512 poses against 38 / 48 / 57 for PCG); round 2 note: rocSOLVER potrf/potrs is latency-bound, PCG wins from ~200 poses
    const double pcg_tol = (opt && opt->pcg_tol > 0) ? opt->pcg_tol : 0.0;     // 0: the default policy (BAChoice::pcg_forcing)
    const int pcg_max_iter = (opt && opt->pcg_max_iter > 0) ? opt->pcg_max_iter : 4000;
    // block-Jacobi block size in poses (tools/ba_pc_sweep.py, 1 200 keyframes, 10 LM iterations): 1 / 8 / 16 / 32 / 64 poses per block need
    // 5 891 / 4 329 / 3 283 / 2 538 / 1 889 CG iterations; the batched potrf + potri of the blocks costs 0.4 / 1.1 / 2.9 ms at 16 / 32 / 64 and is paid on
    // every 3rd trial only (below): 79 ms with 6x6 blocks, 54 / 51.7 / 56 ms with 16 / 32 / 64.  Below ~500 poses the setup is not repaid.
    // From 4096 poses on (measured at 10 000 and 50 000) the SpMV is HBM-bound, the bytes of the larger blocks count and a stale inverse costs 30-40 % more
    // iterations: 16-pose blocks refreshed on every trial are faster there (176 vs 216 ms per 5 LM iterations at 50 000 keyframes).
    // Late in round 4 (blocks inverted in registers: a set-up is 0.1 ms at these sizes; the coarse levels on): 280 / 400 / 600 keyframes per 10 LM iterations with 6 x 6
    // blocks 36.8 / 44.9 / - ms, 16-keyframe blocks 20.0 / 23.4 / 26.7, 16-keyframe blocks + coarse levels 12.4 / 11.9 / 14.0 (tools/ml_small.py): 16 from 128 poses on.
    int pc_g = (opt && opt->pc_block > 0) ? opt->pc_block : (nP >= 128 ? 16 : 1);
    if (pc_g > 1 && pc_g != 8 && pc_g != 16) { corb_set_error("corb_ba_solve: pc_block must be 1, 8 or 16"); return CORB_ERR_ARG; }
    if (solver != 2) pc_g = 1;
    if (solver == 1 && (double)sp * sp * 8.0 > 96e9) { corb_set_error("corb_ba_solve: %d free poses need a %.1f GB dense reduced system; use the PCG solver", nP, (double)sp * sp * 8e-9); return CORB_ERR_ARG; }
    r->solver_used = solver; r->free_poses = nP; r->free_points = nL; r->pc_block = solver == 2 ? pc_g : 0;
    // order: free landmarks ascending, inside a landmark free-pose edges first; then edges of fixed landmarks.
    // Counting sort on the key (landmark, pose-fixed) -- stable, O(E).
    {
        const size_t nkeys = 2 * (size_t)nL + 2;
        std::vector<int>& cnt = hs.cnt; std::vector<int>& sorted = hs.sorted; cnt.assign(nkeys + 1, 0); sorted.resize(act.size());
        auto key = [&](int i) -> size_t { const CorbBAEdge& e = p->edges[i]; const int l = lidx[e.point]; return (l < 0 ? 2 * (size_t)nL : 2 * (size_t)l) + (pidx[e.pose] < 0 ? 1 : 0); };
        if (NT0 > 1) {
            // threads: a stable two-level counting sort.  Level 1 splits the edges into NB buckets of consecutive keys (per-thread histograms, the
            // threads' slots inside a bucket follow the thread order, so the split is stable); level 2 counting-sorts every bucket on its own small
            // key range (cache-resident counters), buckets in parallel.  Same result as the serial sort below.
            const size_t nA = act.size();
            const int NB = 2048;
            const size_t per = (nkeys + NB - 1) / NB;                     // keys per bucket
            std::vector<int>& keys = hs.keys; keys.resize(nA);
            std::vector<int>& tmp = hs.cur; tmp.resize(nA);
            std::vector<std::vector<int>> hist(NT0, std::vector<int>(NB + 1, 0));
            parallel_ranges(nA, NT0, [&](int t, size_t jb, size_t je) { int* h = hist[t].data(); for (size_t j = jb; j < je; j++) { const int k = (int)key(act[j]); keys[j] = k; h[(size_t)k / per]++; } });
            std::vector<int> bstart(NB + 1, 0);
            { int run = 0; for (int b = 0; b < NB; b++) { bstart[b] = run; for (int t = 0; t < NT0; t++) { const int c = hist[t][b]; hist[t][b] = run; run += c; } } bstart[NB] = run; }
            // tmp holds positions j (into act / keys) grouped by bucket
            parallel_ranges(nA, NT0, [&](int t, size_t jb, size_t je) { int* h = hist[t].data(); for (size_t j = jb; j < je; j++) tmp[h[(size_t)keys[j] / per]++] = (int)j; });
            parallel_ranges((size_t)NB, NT0, [&](int, size_t bb, size_t be) {
                std::vector<int> c(per + 1);
                for (size_t b = bb; b < be; b++) {
                    const int s0 = bstart[b], s1 = bstart[b + 1];
                    if (s0 == s1) continue;
                    const int k0 = (int)(b * per);
                    std::fill(c.begin(), c.end(), 0);
                    for (int q = s0; q < s1; q++) c[keys[tmp[q]] - k0 + 1]++;
                    for (size_t k = 0; k < per; k++) c[k + 1] += c[k];
                    for (int q = s0; q < s1; q++) { const int j = tmp[q]; sorted[s0 + c[keys[j] - k0]++] = act[j]; }
                }
            });
        } else {
            for (int i : act) cnt[key(i) + 1]++;
            for (size_t k = 0; k < nkeys; k++) cnt[k + 1] += cnt[k];
            for (int i : act) sorted[cnt[key(i)]++] = i;
        }
        act.swap(sorted);
    }
    const int nE = (int)act.size(); r->active_edges = nE;
    lap("active edges + sort");
    std::vector<int>& e_pose = hs.e_pose; std::vector<int>& e_point = hs.e_point; std::vector<int>& e_vpose = hs.e_vpose; std::vector<int>& e_vpoint = hs.e_vpoint;
    std::vector<int>& loff = hs.loff; std::vector<int>& lnfree = hs.lnfree; std::vector<int>& poff = hs.poff; std::vector<int>& pedge = hs.pedge;
    std::vector<double>& e_obs = hs.e_obs; std::vector<double>& e_w = hs.e_w; std::vector<unsigned char>& e_dim = hs.e_dim;
    e_pose.clear(); e_point.clear(); e_vpose.clear(); e_vpoint.clear(); e_obs.clear(); e_w.clear(); e_dim.clear();      // (no copy of stale elements when a vector grows)
    e_pose.resize(nE); e_point.resize(nE); e_vpose.resize(nE); e_vpoint.resize(nE); loff.assign(nL + 1, 0); lnfree.assign(nL, 0); poff.assign(nP + 1, 0);
    e_obs.resize(3 * (size_t)nE); e_w.resize(nE); e_dim.resize(nE);
    const int NT = ba_host_threads((size_t)nE);
    std::vector<std::vector<int>> phist(NT, std::vector<int>(NT > 1 ? nP : 0));
    parallel_ranges((size_t)nE, NT, [&](int t, size_t jb, size_t je) {
        int* ph = NT > 1 ? phist[t].data() : nullptr;
        for (size_t j = jb; j < je; j++) {
            const CorbBAEdge& e = p->edges[act[j]];
            const int ep = pidx[e.pose], el = lidx[e.point];
            e_pose[j] = ep; e_point[j] = el; e_vpose[j] = e.pose; e_vpoint[j] = e.point;
            e_dim[j] = e.u_right < 0 ? 2 : 3;               // mvuRight<0 -> EdgeSE3ProjectXYZ, else EdgeStereoSE3ProjectXYZ (Optimizer.cc:147)
            e_obs[3 * j] = e.u; e_obs[3 * j + 1] = e.v; e_obs[3 * j + 2] = e.u_right; e_w[j] = e.inv_sigma2;
            if (NT > 1) {
                if (el >= 0) { __atomic_fetch_add(&loff[el + 1], 1, __ATOMIC_RELAXED); if (ep >= 0) __atomic_fetch_add(&lnfree[el], 1, __ATOMIC_RELAXED); }   // (integer counts: order-free)
                if (ep >= 0) ph[ep]++;
            } else {
                if (el >= 0) { loff[el + 1]++; if (ep >= 0) lnfree[el]++; }
                if (ep >= 0) poff[ep + 1]++;
            }
        }
    });
    if (NT > 1) for (int k = 0; k < nP; k++) { int c = 0; for (int t = 0; t < NT; t++) c += phist[t][k]; poff[k + 1] = c; }
    for (int l = 0; l < nL; l++) loff[l + 1] += loff[l];
    for (int k = 0; k < nP; k++) poff[k + 1] += poff[k];
    pedge.resize(poff[nP]);
    if (NT > 1) {
        // thread t's first slot in pose k's list = poff[k] + what the threads before it hold: every list stays in ascending edge order
        for (int k = 0; k < nP; k++) { int run = poff[k]; for (int t = 0; t < NT; t++) { const int c = phist[t][k]; phist[t][k] = run; run += c; } }
        parallel_ranges((size_t)nE, NT, [&](int t, size_t jb, size_t je) { int* cur = phist[t].data(); for (size_t j = jb; j < je; j++) if (e_pose[j] >= 0) pedge[cur[e_pose[j]]++] = (int)j; });
    } else { std::vector<int> cur(poff.begin(), poff.end() - 1); for (int j = 0; j < nE; j++) if (e_pose[j] >= 0) pedge[cur[e_pose[j]]++] = j; }
    // landmark of every pose-edge entry: ascending per pose (the edges are sorted by landmark), fixed landmarks (-1) last.  The deterministic Schur
    // kernel merges these lists (a (keyframe, map point) pair that occurs twice -- the reference cannot produce one, MapPoint::mObservations is a std::map
    // keyed by the keyframe -- pairs each of its edges with all edges of the other keyframe on that point: the summed Hpl block of g2o).
    std::vector<int>& plm = hs.plm; plm.resize(pedge.size());
    parallel_ranges((size_t)nP, NT, [&](int, size_t kb, size_t ke) {
        for (size_t k = kb; k < ke; k++)
            for (int ii = poff[k]; ii < poff[k + 1]; ii++) plm[ii] = e_point[pedge[ii]];
    });
    lap("edge arrays + lists");
    std::vector<double>& pose_q = st.q; std::vector<double>& pose_t = st.t; std::vector<double>& pt = st.pt;
    // block-sparse pattern of the reduced camera system: pose pairs that share a landmark (block_solver.hpp:262-292)
    std::vector<int>& bsr_rowptr = hs.bsr_rowptr; std::vector<int>& bsr_col = hs.bsr_col; std::vector<int>& bsr_diag = hs.bsr_diag;
    std::vector<int>& uinfo = hs.uinfo; uinfo.clear();        // (slot, p, q, -) of every block on / above the diagonal
    bsr_rowptr.assign(nP + 1, 0); bsr_col.clear(); bsr_diag.assign(nP, 0);
    static const int small_edges = corb_dev_env("CORB_BA_SMALL_EDGES") ? atoi(corb_dev_env("CORB_BA_SMALL_EDGES")) : BA_SMALL_EDGES;     // (env: development aid)
    const bool fused_small = solver == 1 && sp <= BA_SMALL_SP && nE <= small_edges && nL <= small_edges && (opt == nullptr || opt->solver != 1);
    const bool want_pattern = solver == 2 || !fused_small;
    if (want_pattern) {
        // row k: the free poses that share a landmark with pose k (and k itself).  Gathered per row through the pose -> edges ->
        // landmark -> poses lists with a stamp array: sum_l k_l^2 cheap visits, no global sort of pair keys (1 GB at 50 k keyframes)
        // (rows are independent: worker threads with their own stamp arrays, the row lists concatenated in row order)
        std::vector<std::vector<int>> part_col(NT), part_cnt(NT);
        parallel_ranges((size_t)nP, NT, [&](int t, size_t kb, size_t ke) {
            std::vector<int> stamp(nP, -1), cols; std::vector<int>& out = part_col[t]; std::vector<int>& cnt = part_cnt[t];
            out.reserve((ke - kb) * 32); cnt.reserve(ke - kb);
            for (size_t k = kb; k < ke; k++) {
                cols.clear(); cols.push_back((int)k); stamp[k] = (int)k;
                for (int ii = poff[k]; ii < poff[k + 1]; ii++) {
                    const int l = e_point[pedge[ii]];
                    if (l < 0) continue;
                    const int e0 = loff[l], kk = lnfree[l];
                    for (int a = 0; a < kk; a++) { const int q = e_pose[e0 + a]; if (stamp[q] != (int)k) { stamp[q] = (int)k; cols.push_back(q); } }
                }
                std::sort(cols.begin(), cols.end());
                cnt.push_back((int)cols.size()); out.insert(out.end(), cols.begin(), cols.end());
            }
        });
        { int k = 0; for (int t = 0; t < NT; t++) for (int c : part_cnt[t]) { bsr_rowptr[k + 1] = bsr_rowptr[k] + c; k++; } }
        bsr_col.resize(bsr_rowptr[nP]);
        { size_t o = 0; for (int t = 0; t < NT; t++) { if (!part_col[t].empty()) memcpy(&bsr_col[o], part_col[t].data(), part_col[t].size() * sizeof(int)); o += part_col[t].size(); } }
        for (int k = 0; k < nP; k++)
            for (int sl = bsr_rowptr[k]; sl < bsr_rowptr[k + 1]; sl++) {
                const int q = bsr_col[sl];
                if (q == k) bsr_diag[k] = sl;
                if (q >= k) { uinfo.push_back(sl); uinfo.push_back(k); uinfo.push_back(q); uinfo.push_back(0); }
            }
    }
    const bool use_pairs = want_pattern;
    const int nnzb = (int)bsr_col.size(); r->nnz_blocks = nnzb; r->schur_pairs = 0;
    int bsr_max_row = 0; for (int k = 0; k < nP && want_pattern; k++) bsr_max_row = std::max(bsr_max_row, bsr_rowptr[k + 1] - bsr_rowptr[k]);
    lap("block pattern");
    // ---- device state ----
    std::unique_ptr<Pool> own_pool;
    if (sess) sess->pool.reset(new Pool()); else own_pool.reset(new Pool());
    Pool& pool = sess ? *sess->pool : *own_pool;
    if (!pool.stream) { corb_set_error("BA workspace: stream creation failed"); return CORB_ERR_HIP; }
    hipStream_t s = pool.stream;
    BAFlat f;
    f.nE = nE; f.nP = nP; f.nL = nL; f.nnzb = nnzb; f.bsr_max_row = bsr_max_row; f.nA = loff[nL]; f.have_pattern = want_pattern; f.nu = (int)(uinfo.size() / 4);
    // local windows: the pairs of a landmark with k free-keyframe observations are at most k^2 (k (k + 1) / 2 unless a keyframe observes it twice)
    if (want_pattern && sp > 0 && sp <= 128) { size_t b = 1; for (int l = 0; l < nL; l++) b += (size_t)lnfree[l] * (size_t)lnfree[l]; f.pairs_bound = b; }
    static thread_local std::vector<double> cam; cam_table(p, cam);
    // the estimates (quaternions | translations | points) are one block, so that push() / pop() of a trial are one copy each
    f.n_q = pose_q.size(); f.n_t = pose_t.size(); f.n_pt = pt.size();
    const size_t n_state = f.n_q + f.n_t + f.n_pt;
    HIPCHK(pool.alloc(&f.dq, n_state));
    HIPCHK(pool.alloc(&f.dq_bak, n_state));
    double* dq = f.dq; double* dt = dq + f.n_q; double* dpt = dt + f.n_t;
    {
        // inputs: small problems (local windows) pack everything into one staging block and one copy -- sixteen synchronous copies of a few KB each
        // cost more than the optimisation itself there; large maps copy array by array
        struct Piece { const void* src; size_t bytes; void** dst; };
        const Piece pieces[] = {
            {e_pose.data(), e_pose.size() * 4, (void**)&f.e_pose}, {e_point.data(), e_point.size() * 4, (void**)&f.e_point}, {e_vpose.data(), e_vpose.size() * 4, (void**)&f.e_vpose},
            {e_vpoint.data(), e_vpoint.size() * 4, (void**)&f.e_vpoint}, {e_obs.data(), e_obs.size() * 8, (void**)&f.e_obs}, {e_w.data(), e_w.size() * 8, (void**)&f.e_w},
            {e_dim.data(), e_dim.size(), (void**)&f.e_dim}, {loff.data(), loff.size() * 4, (void**)&f.loff}, {lnfree.data(), lnfree.size() * 4, (void**)&f.lnfree},
            {poff.data(), poff.size() * 4, (void**)&f.poff}, {pedge.data(), pedge.size() * 4, (void**)&f.pedge}, {pose_vertex.data(), pose_vertex.size() * 4, (void**)&f.pose_vertex},
            {point_vertex.data(), point_vertex.size() * 4, (void**)&f.point_vertex}, {cam.data(), cam.size() * 8, (void**)&f.cam}};
        size_t total = 0;
        for (const Piece& pc : pieces) total += (pc.bytes + 255) & ~(size_t)255;
        if (total + n_state * 8 <= ((size_t)4 << 20)) {
            static thread_local std::vector<char> blob;
            blob.resize(total + n_state * 8 + 256);
            char* dblob = nullptr; HIPCHK(pool.alloc(&dblob, total + 256));
            size_t off = 0;
            for (const Piece& pc : pieces) { if (pc.bytes) memcpy(blob.data() + off, pc.src, pc.bytes); *pc.dst = dblob + off; off += (pc.bytes + 255) & ~(size_t)255; }
            if (total) HIPCHK(pool.h2d(dblob, blob.data(), total));                  // (page-locked staging: asynchronous on the lane's stream)
            double* st = reinterpret_cast<double*>(blob.data() + total + (256 - total % 256) % 256);     // (8-byte aligned: total is a multiple of 256)
            if (!pose_q.empty()) memcpy(st, pose_q.data(), pose_q.size() * 8);
            if (!pose_t.empty()) memcpy(st + pose_q.size(), pose_t.data(), pose_t.size() * 8);
            if (!pt.empty()) memcpy(st + pose_q.size() + pose_t.size(), pt.data(), pt.size() * 8);
            if (n_state) HIPCHK(pool.h2d(dq, st, n_state * 8));
        } else {
            HIPCHK(pool.upload(&f.e_pose, e_pose)); HIPCHK(pool.upload(&f.e_point, e_point)); HIPCHK(pool.upload(&f.e_vpose, e_vpose)); HIPCHK(pool.upload(&f.e_vpoint, e_vpoint));
            HIPCHK(pool.upload(&f.e_obs, e_obs)); HIPCHK(pool.upload(&f.e_w, e_w)); HIPCHK(pool.upload(&f.e_dim, e_dim));
            HIPCHK(pool.upload(&f.loff, loff)); HIPCHK(pool.upload(&f.lnfree, lnfree)); HIPCHK(pool.upload(&f.poff, poff)); HIPCHK(pool.upload(&f.pedge, pedge));
            HIPCHK(pool.upload(&f.pose_vertex, pose_vertex)); HIPCHK(pool.upload(&f.point_vertex, point_vertex)); HIPCHK(pool.upload(&f.cam, cam));
            if (!pose_q.empty()) HIPCHK(hipMemcpy(dq, pose_q.data(), pose_q.size() * 8, hipMemcpyHostToDevice));
            if (!pose_t.empty()) HIPCHK(hipMemcpy(dt, pose_t.data(), pose_t.size() * 8, hipMemcpyHostToDevice));
            if (!pt.empty()) HIPCHK(hipMemcpy(dpt, pt.data(), pt.size() * 8, hipMemcpyHostToDevice));
        }
        if (want_pattern) { HIPCHK(pool.upload(&f.bsr_rowptr, bsr_rowptr)); HIPCHK(pool.upload(&f.bsr_col, bsr_col)); HIPCHK(pool.upload(&f.bsr_diag, bsr_diag)); }
        if (use_pairs && nP > 0) { HIPCHK(pool.upload(&f.uinfo, uinfo)); HIPCHK(pool.upload(&f.plm, plm)); }
    }
    lap("uploads");
    BAChoice ch; ch.solver = solver; ch.pc_g = pc_g; ch.pcg_tol = pcg_tol > 0 ? pcg_tol : BA_PCG_TOL_TIGHT; ch.pcg_forcing = !(pcg_tol > 0) && nP > BA_PCG_FORCING_MIN_POSES; ch.pcg_max_iter = pcg_max_iter; ch.fused_small = fused_small; ch.want_pattern = want_pattern;
    ch.multilevel = solver == 2 && pc_g == BA_ML_G && (opt && opt->pc_multilevel ? opt->pc_multilevel == 2 : nP >= BA_ML_AUTO_POSES);
    double* d_e_chi2 = nullptr;
    bool sess_ok = false;                                  // the graph stays on the device for the later optimize() calls of this staged solve
    if (sess && !fused_small && (int)act.size() == p->n_edges) {
        sess_ok = true;
        if (active) for (int i = 0; i < p->n_edges && sess_ok; i++) sess_ok = active[i] != 0;
    }
    const bool dev = sess_ok && sess->want_dev && sess->n_sets > 1;
    if (dev) {                                             // the information weights, the chi2 memory and the active sets of the classifications (BASession)
        HIPCHK(pool.alloc(&sess->d_w0, (size_t)nE)); HIPCHK(pool.alloc(&sess->d_last, (size_t)nE)); HIPCHK(pool.alloc(&sess->d_act, (size_t)sess->n_sets * (nE ? nE : 1)));
        // (set 0 -- every edge -- is never stored: the first classification is told so, and with every edge active it does not read d_last either)
        if (nE) HIPCHK(hipMemcpyAsync(sess->d_w0, f.e_w, sizeof(double) * (size_t)nE, hipMemcpyDeviceToDevice, s));
    }
    rc = ba_lm_device(pool, f, ch, iterations, robust, stop_flag, r, delta2, delta3, lap, &d_e_chi2, sess_ok ? &sess->work : nullptr);
    if (rc) return rc;
    if (dev) {                                             // nothing is read back: the caller's classification and later optimize() calls go on where the estimates are
        sess->f = f; sess->ch = ch; sess->act = act; sess->covers_all = true; sess->ready = true; sess->dev = true; sess->cur_set = 0; sess->d_e_chi2 = d_e_chi2;
        return CORB_OK;
    }
    if (n_state * 8 <= ((size_t)4 << 20)) {              // small state: one copy of the whole block, split on the host
        static thread_local std::vector<double> st;
        st.resize(n_state ? n_state : 1);
        if (n_state) HIPCHK(hipMemcpyAsync(st.data(), dq, n_state * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (!pose_q.empty()) memcpy(pose_q.data(), st.data(), pose_q.size() * 8);
        if (!pose_t.empty()) memcpy(pose_t.data(), st.data() + pose_q.size(), pose_t.size() * 8);
        if (!pt.empty()) memcpy(pt.data(), st.data() + pose_q.size() + pose_t.size(), pt.size() * 8);
    } else {
        HIPCHK(hipMemcpyAsync(pose_q.data(), dq, pose_q.size() * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(pose_t.data(), dt, pose_t.size() * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(pt.data(), dpt, pt.size() * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    if (last_chi2 && nE > 0) {
        std::vector<double> ec(nE);
        HIPCHK(pool.d2h(ec.data(), d_e_chi2, sizeof(double) * (size_t)nE)); HIPCHK(pool.fetch_finish());
        for (int j = 0; j < nE; j++) (*last_chi2)[act[j]] = ec[j];
    }
    lap("read back");
    if (sess_ok) { sess->f = f; sess->ch = ch; sess->act = act; sess->e_w0 = e_w; sess->covers_all = true; sess->ready = true; }
    if (sess && !sess->ready) sess->pool.reset();            // (no session after all: the lane's workspace must be free for the next call)
    return CORB_OK;
}
}  // namespace

extern "C" int corb_ba_solve(const CorbBAProblem* p, int iterations, int robust, volatile int* stop_flag, CorbBAResult* r, int device)
{
    return corb_ba_solve_ex(p, iterations, robust, stop_flag, r, device, nullptr);
}

extern "C" int corb_warmup(int device)
{
    int rc = corb_select_device(device); if (rc) return rc;
    // Rounds 1-2 ran rocSOLVER's factorisations once here, because rocBLAS / rocSOLVER load their kernel libraries lazily (seconds inside the first
    // optimisation of a process).  The library links neither any more: what is left to warm up are the two workspace lanes (stream, events, pinned block).
    for (int lane = 0; lane < 2; lane++) {
        CorbScratch pool(lane);
        if (!pool.stream) { corb_set_error("corb_warmup: workspace creation failed"); return CORB_ERR_HIP; }
    }
    return CORB_OK;
}

// ---- large maps handed over as HOST arrays (round 5) ----
// OptimizerT::BundleAdjustment (host/corb_adapter_orbslam.hpp; Optimizer.cc:150-210) builds its edges map point by map point, so a caller's edge array arrives grouped
// by point -- which is the order corb_ba_solve_device wants.  Such a problem does not need the host flattening (sort, lists, pattern: ~95 ms of threads at 27.5 M
// observations) and its 1.1 GB of flattened uploads: the RAW arrays travel through a page-locked double buffer filled by worker threads (which check the edges' index ranges
// and their grouping on the way: the serial validate() pass over 27.5 M edges is gone too), and the graph is flattened on the device like corb_ba_solve_store's.  The estimates
// of both paths are equal element for element (tests/test_gpu_ba.py::test_device_flattening_equals_host_flattening); wall time of the call at 50 000 keyframes 0.38 -> 0.2x s.
#define BA_HOST_FAST_MIN_EDGES (1 << 20)
#define BA_HOST_FAST_MIN_POSES 257          // the PCG solver's range (auto choice): smaller problems keep the host path and its session / staging features
namespace {
struct HostFastBuf {                         // per device: grown by the calls, given back by corb_release_scratch; one call at a time per device
    std::mutex mu; int device = -1;
    char* dev = nullptr; size_t dev_cap = 0; char* pin[2] = {nullptr, nullptr}; size_t pin_cap = 0;
    hipStream_t stream = nullptr; hipEvent_t ev[2] = {nullptr, nullptr};
    size_t release() {                       // (the caller holds mu and has selected the device)
        size_t freed = dev_cap;
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); stream = nullptr; }
        for (int i = 0; i < 2; i++) { if (ev[i]) { (void)hipEventDestroy(ev[i]); ev[i] = nullptr; } if (pin[i]) { (void)hipHostFree(pin[i]); pin[i] = nullptr; freed += pin_cap; } }
        if (dev) (void)hipFree(dev);
        dev = nullptr; dev_cap = 0; pin_cap = 0; device = -1;
        return freed;
    }
};
HostFastBuf& hostfast(int device) { static HostFastBuf b[64]; return b[device < 0 || device >= 64 ? 0 : device]; }
// off[m] = first edge of point m (edges non-decreasing in .point): a binary search per point
}
void ba_launch_edge_offsets(const CorbBAEdge* edges, int n_edges, int n_points, int* off, hipStream_t s);

// Device and page-locked memory the library keeps between calls goes back to the runtime: the arenas of the device's two workspace lanes and the staging of large host-array
// BA calls.  A lane (or the staging) that a call of another thread holds at this moment is left alone.  The next call that needs them allocates them again.
extern "C" int corb_release_scratch(int device, uint64_t* bytes_released)
{
    int rc = corb_select_device(device); if (rc) return rc;
    uint64_t freed = 0;
    for (int lane = 0; lane < 2; lane++) {
        CorbWorkspace& ws = corb_workspace(device, lane);
        std::unique_lock<std::mutex> lk(ws.mu, std::try_to_lock);
        if (!lk.owns_lock()) continue;
        if (ws.stream) (void)hipStreamSynchronize(ws.stream);
        for (auto& c : ws.chunks) { freed += c.cap; (void)hipFree(c.base); }
        ws.chunks.clear();
        if (ws.hstage) { freed += ws.hcap; (void)hipHostFree(ws.hstage); ws.hstage = nullptr; ws.hcap = 0; ws.hused = 0; ws.hwant = 0; }
    }
    {
        HostFastBuf& B = hostfast(device);
        std::unique_lock<std::mutex> lk(B.mu, std::try_to_lock);
        if (lk.owns_lock()) freed += B.release();
    }
    if (bytes_released) *bytes_released = freed;
    return CORB_OK;
}

static int ba_solve_host_via_device(const CorbBAProblem* p, int iterations, int robust, volatile int* stop_flag, CorbBAResult* r, int device, const CorbBAOptions* opt, bool* taken)
{
    *taken = false;
    HostFastBuf& B = hostfast(device);
    std::unique_lock<std::mutex> lk(B.mu, std::try_to_lock);
    if (!lk.owns_lock()) return CORB_OK;                       // another thread's large call holds the buffers: this one takes the host path
    const size_t K = (size_t)p->n_poses, M = (size_t)p->n_points, E = (size_t)p->n_edges;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_poses = 0, o_pf = o_poses + al(64 * K), o_pts = o_pf + al(K), o_xf = o_pts + al(12 * M), o_intr = o_xf + al(M), o_off = o_intr + al(20 * K),
                 o_edges = o_off + al(4 * (M + 1)), total = o_edges + al(sizeof(CorbBAEdge) * E);
    const size_t CH = (size_t)32 << 20;
    if (B.device != device || B.dev_cap < total || !B.pin[0] || !B.stream) {
        if (B.dev) (void)hipFree(B.dev);
        B.dev = nullptr; B.dev_cap = 0;
        if (hipMalloc((void**)&B.dev, total + (total >> 3)) != hipSuccess) { (void)hipGetLastError(); return CORB_OK; }      // no room: the host path
        B.dev_cap = total + (total >> 3); B.device = device;
        for (int i = 0; i < 2; i++) if (!B.pin[i] && hipHostMalloc((void**)&B.pin[i], CH, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return CORB_OK; }
        B.pin_cap = CH;
        if (!B.stream && hipStreamCreateWithFlags(&B.stream, hipStreamNonBlocking) != hipSuccess) return CORB_ERR_HIP;
        for (int i = 0; i < 2; i++) if (!B.ev[i] && hipEventCreateWithFlags(&B.ev[i], hipEventDisableTiming) != hipSuccess) return CORB_ERR_HIP;
    }
    // the small arrays, then the edges in chunks: worker threads copy a chunk into a page-locked buffer (checking it), the DMA of the previous chunk runs meanwhile
    std::vector<float> intr(5 * K + 1);
    for (size_t k = 0; k < K; k++) for (int a = 0; a < 5; a++) intr[5 * k + a] = p->intr ? p->intr[5 * k + a] : (a == 0 ? p->fx : a == 1 ? p->fy : a == 2 ? p->cx : a == 3 ? p->cy : p->bf);
    struct Piece { size_t off; const char* src; size_t bytes; };
    const Piece pieces[] = { {o_poses, (const char*)p->poses, 64 * K}, {o_pf, (const char*)p->pose_fixed, K}, {o_pts, (const char*)p->points, 12 * M}, {o_xf, (const char*)p->point_fixed, M},
                             {o_intr, (const char*)intr.data(), 20 * K}, {o_edges, (const char*)p->edges, sizeof(CorbBAEdge) * E} };
    const int NT = (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency() / 2));
    std::atomic<int> bad{0};                                       // 1: an index out of range, 2: edges not grouped by point
    int cur = 0; bool used[2] = {false, false};
    for (const Piece& pc : pieces) {
        const bool is_edges = pc.off == o_edges;
        const size_t unit = is_edges ? sizeof(CorbBAEdge) : 1, per_chunk = (CH / unit) * unit;
        for (size_t done = 0; done < pc.bytes; done += per_chunk) {
            const size_t nb = std::min(per_chunk, pc.bytes - done);
            if (used[cur]) HIPCHK(hipEventSynchronize(B.ev[cur]));
            char* dst = B.pin[cur]; const char* src = pc.src + done;
            auto work = [&](int t) {
                const size_t n_units = nb / unit, u0 = n_units * t / NT, u1 = n_units * (t + 1) / NT;
                memcpy(dst + u0 * unit, src + u0 * unit, (u1 - u0) * unit);
                if (is_edges) {
                    const CorbBAEdge* e = reinterpret_cast<const CorbBAEdge*>(src); const size_t first = done / unit;
                    for (size_t i = u0; i < u1; i++) {
                        if (e[i].pose < 0 || e[i].pose >= p->n_poses || e[i].point < 0 || e[i].point >= p->n_points) bad.store(1);
                        else if (first + i > 0 && e[i].point < (reinterpret_cast<const CorbBAEdge*>(pc.src))[first + i - 1].point && bad.load() == 0) bad.store(2);
                    }
                }
            };
            if (nb < ((size_t)1 << 20)) { for (int t = 0; t < NT; t++) work(t); }
            else { std::vector<std::thread> th; for (int t = 1; t < NT; t++) th.emplace_back(work, t); work(0); for (auto& x : th) x.join(); }
            if (bad.load()) break;
            HIPCHK(hipMemcpyAsync(B.dev + pc.off + done, dst, nb, hipMemcpyHostToDevice, B.stream));
            HIPCHK(hipEventRecord(B.ev[cur], B.stream)); used[cur] = true; cur ^= 1;
        }
        if (bad.load()) break;
    }
    if (bad.load() == 1) { HIPCHK(hipStreamSynchronize(B.stream)); corb_set_error("corb_ba_solve: an edge's pose / point index is out of range"); *taken = true; return CORB_ERR_ARG; }
    if (bad.load() == 2) { HIPCHK(hipStreamSynchronize(B.stream)); return CORB_OK; }              // edges not grouped by point: the host path sorts them
    CorbBADeviceProblem dp; memset(&dp, 0, sizeof(dp));
    dp.n_poses = (int)K; dp.n_points = (int)M; dp.n_edges = (int)E;
    dp.poses = (float*)(B.dev + o_poses); dp.pose_fixed = (const uint8_t*)(B.dev + o_pf); dp.points = (float*)(B.dev + o_pts); dp.point_fixed = (const uint8_t*)(B.dev + o_xf);
    dp.intr = (const float*)(B.dev + o_intr); dp.edges = (const CorbBAEdge*)(B.dev + o_edges); dp.edge_off = (const int*)(B.dev + o_off);
    ba_launch_edge_offsets(dp.edges, (int)E, (int)M, (int*)(B.dev + o_off), B.stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(B.stream));
    *taken = true;
    float* user_poses = r->poses; float* user_points = r->points;
    int rc = corb_ba_solve_device(&dp, iterations, robust, stop_flag, r, device, opt);
    r->poses = user_poses; r->points = user_points;
    if (rc) return rc;
    // the estimates back: two page-locked chunks alternate between the DMA and the copy into the caller's arrays
    struct Out { char* dst; size_t off, bytes; } outs[2] = { {(char*)r->poses, o_poses, 64 * K}, {(char*)r->points, o_pts, 12 * M} };
    for (const Out& o : outs) {
        size_t issued = 0, copied = 0; int ci = 0, cc = 0; size_t len[2] = {0, 0};
        while (copied < o.bytes) {
            while (issued < o.bytes && issued - copied < 2 * CH) {
                const size_t nb = std::min(CH, o.bytes - issued);
                HIPCHK(hipMemcpyAsync(B.pin[ci], B.dev + o.off + issued, nb, hipMemcpyDeviceToHost, B.stream));
                HIPCHK(hipEventRecord(B.ev[ci], B.stream)); len[ci] = nb; issued += nb; ci ^= 1;
            }
            HIPCHK(hipEventSynchronize(B.ev[cc]));
            memcpy(o.dst + copied, B.pin[cc], len[cc]); copied += len[cc]; cc ^= 1;
        }
    }
    return CORB_OK;
}

extern "C" int corb_ba_solve_ex(const CorbBAProblem* p, int iterations, int robust, volatile int* stop_flag, CorbBAResult* r, int device, const CorbBAOptions* opt)
{
    if (p && r && r->poses && r->points && p->n_edges >= BA_HOST_FAST_MIN_EDGES && p->n_poses >= BA_HOST_FAST_MIN_POSES && p->n_points > 0 && iterations >= 0 &&
        p->poses && p->pose_fixed && p->points && p->point_fixed && p->edges && (!opt || opt->solver == 0 || opt->solver == 2) && !getenv("CORB_BA_HOST_FLATTEN")) {
        int rc0 = corb_select_device(device); if (rc0) return rc0;
        bool taken = false;
        rc0 = ba_solve_host_via_device(p, iterations, robust, stop_flag, r, device, opt, &taken);
        if (taken || rc0) return rc0;
    }
    int rc = validate(p, r); if (rc) return rc;
    if (iterations < 0) { corb_set_error("corb_ba_solve: negative iteration count"); return CORB_ERR_ARG; }
    rc = corb_select_device(device); if (rc) return rc;
    r->iters_done = 0; r->trials_total = 0; r->ms_total = r->ms_build = r->ms_schur = r->ms_solve = r->ms_update = 0;
    r->solver_used = 0; r->pcg_iterations = 0; r->free_poses = r->free_points = r->active_edges = r->pc_block = r->pc_levels = 0; r->nnz_blocks = r->schur_pairs = 0; r->pcg_residual_max = r->pcg_residual_last = 0.0; r->grad_inf = -1.0; r->pcg_refined_trials = 0; r->reserved0 = 0;
    BAState st; state_from_floats(p, st);
    std::vector<uint8_t> pose_touched(p->n_poses ? p->n_poses : 1, 0), pt_touched(p->n_points ? p->n_points : 1, 0);
    rc = ba_optimize_device(p, nullptr, st, iterations, robust, stop_flag, r, device, opt, nullptr, &pose_touched, &pt_touched,
                            (double)(float)std::sqrt(5.99), (double)(float)std::sqrt(7.815));   // thHuber2D/3D are floats (Optimizer.cc:102-103)
    if (rc) return rc;
    for (auto& v : pose_touched) v = 1;                         // GlobalBundleAdjustemnt writes every non-fixed keyframe back (Optimizer.cc:216-237)
    state_to_floats(p, st, pose_touched, pt_touched, r);
    return CORB_OK;
}

extern "C" int corb_spd_solve(const double* A, int n, const double* b, double* x, int* info, int device)
{
    if (n < 0 || (n > 0 && (!A || !b || !x))) { corb_set_error("corb_spd_solve: bad argument"); return CORB_ERR_ARG; }
    if (info) *info = 0;
    if (n == 0) return CORB_OK;
    int rc = corb_select_device(device); if (rc) return rc;
    CorbScratch pool(0);
    double *dA, *db; int* dinfo;
    HIPCHK(pool.alloc(&dA, (size_t)n * n)); HIPCHK(pool.alloc(&db, (size_t)n)); HIPCHK(pool.alloc(&dinfo, 1));
    HIPCHK(hipMemcpyAsync(dA, A, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice, pool.stream));
    HIPCHK(hipMemcpyAsync(db, b, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, pool.stream));
    double* dws; HIPCHK(pool.alloc(&dws, corb_chol_workspace_doubles(n)));
    corb_launch_chol_solve(dA, n, n, db, dinfo, dws, pool.stream);
    HIPCHK(hipGetLastError());
    int h_info = 0;
    HIPCHK(hipMemcpyAsync(x, db, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, pool.stream));
    HIPCHK(hipMemcpyAsync(&h_info, dinfo, sizeof(int), hipMemcpyDeviceToHost, pool.stream));
    HIPCHK(hipStreamSynchronize(pool.stream));
    if (info) *info = h_info;
    return CORB_OK;
}

// ---- fused single-pose path (pose_kernels.hip) ----------------------------------------------------------------
namespace {
struct PoseBatch {                       // flattened problems of one launch
    std::vector<int> edge_off{0}, stage_limit;      // stage_limit: empty = every problem runs all stages
    std::vector<double> pt, obs, w, cam, pose;
    std::vector<unsigned char> dim;
};
void pose_from_T(const float* T, double* out7)
{
    const double R[9] = { T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10] };
    quat_from_R_host(R, out7);
    out7[4] = T[3]; out7[5] = T[7]; out7[6] = T[11];
}
void pose_to_T(const double* p7, float* T)
{
    double R[9]; quat_to_R_host(p7, R);
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
}  // namespace
// (corb_track.cpp: the same conversions and the same four rounds for a frame that lives in a store record)
void corb_pose_from_T(const float* T, double* out7) { pose_from_T(T, out7); }
void corb_pose_to_T(const double* p7, float* T) { pose_to_T(p7, T); }
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
namespace {
// one free pose, every edge attached to it, every referenced point fixed, <= 8 stages, no stop flag raised
int single_pose_problem(const CorbBAProblem* p, int n_stages)
{
    if (n_stages > CORB_POSE_MAX_STAGES) return -1;
    int freep = -1;
    for (int k = 0; k < p->n_poses; k++) if (!p->pose_fixed[k]) { if (freep >= 0) return -1; freep = k; }
    if (freep < 0) return -1;
    for (int i = 0; i < p->n_edges; i++) if (p->edges[i].pose != freep || !p->point_fixed[p->edges[i].point]) return -1;
    return freep;
}
}  // namespace

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
        double p7[7]; pose_from_T(F.Tcw, p7);
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
    // the four rounds of Optimizer.cc:385-470: chi2 thresholds 5.991 / 7.815, Huber deltas sqrt of those, the last round without kernel
    CorbBAStage st[4];
    for (int s = 0; s < 4; s++) {
        memset(&st[s], 0, sizeof(CorbBAStage));
        st[s].iterations = 10; st[s].robust = s < 3 ? 1 : 0; st[s].chi2_mono = 5.991f; st[s].chi2_stereo = 7.815f;
        st[s].recompute_inactive = 1; st[s].allow_reactivate = 1; st[s].reset_estimates = 1; st[s].float_compare = 1;
        st[s].huber_mono = sqrtf(5.991f); st[s].huber_stereo = sqrtf(7.815f);
    }
    std::vector<double> pose; std::vector<unsigned char> act; std::vector<int> cnt;
    rc = pose_batch_run(b, st, 4, pose, act, cnt, nullptr); if (rc) return rc;
    for (int f = 0; f < n_frames; f++) {
        if (frames[f].n_obs < 3) {                        // plain `return 0`: pose untouched, mvbOutlier as set while the edges were collected (all false)
            memcpy(Tcw_out + 16 * (size_t)f, frames[f].Tcw, 16 * sizeof(float));
            if (outlier && outlier[f]) for (int i = 0; i < frames[f].n_obs; i++) outlier[f][i] = 0;
            if (n_inliers) n_inliers[f] = 0;
            continue;
        }
        if (cnt[4 * (size_t)f + 2]) pose_to_T(&pose[7 * (size_t)f], Tcw_out + 16 * (size_t)f);
        else memcpy(Tcw_out + 16 * (size_t)f, frames[f].Tcw, 16 * sizeof(float));
        if (outlier && outlier[f]) for (int i = 0; i < frames[f].n_obs; i++) outlier[f][i] = act[b.edge_off[f] + i] ? 0 : 1;
        if (n_inliers) n_inliers[f] = cnt[4 * (size_t)f + 3];
    }
    return CORB_OK;
}

// Optimizer::LocalBundleAdjustment / PoseOptimization style multi-stage optimisation (see include/corb_accel.h)
static int ba_staged_window_host(const CorbBAProblem* p, const CorbBAStage* stages, int n_stages, volatile int* stop_flag, CorbBAResult* r, uint8_t* edge_outlier,
                                 const CorbBAOptions* opt, int* applicable);
extern "C" int corb_ba_solve_staged(const CorbBAProblem* p, const CorbBAStage* stages, int n_stages, volatile int* stop_flag,
                                    CorbBAResult* r, uint8_t* edge_outlier, int device, const CorbBAOptions* opt)
{
    int rc = validate(p, r); if (rc) return rc;
    if (!stages || n_stages < 1) { corb_set_error("corb_ba_solve_staged: no stages"); return CORB_ERR_ARG; }
    rc = corb_select_device(device); if (rc) return rc;
    r->iters_done = 0; r->trials_total = 0; r->ms_total = r->ms_build = r->ms_schur = r->ms_solve = r->ms_update = 0;
    r->solver_used = 0; r->pcg_iterations = 0; r->free_poses = r->free_points = r->active_edges = r->pc_block = r->pc_levels = 0; r->nnz_blocks = r->schur_pairs = 0; r->pcg_residual_max = r->pcg_residual_last = 0.0; r->grad_inf = -1.0; r->pcg_refined_trials = 0; r->reserved0 = 0;
    double* chi_hist = r->chi2; double* lam_hist = r->lambda; r->chi2 = nullptr; r->lambda = nullptr;     // histories are per optimize() call
    const int E = p->n_edges;
    const int solver_opt = opt ? opt->solver : 0;
    const int freep = (solver_opt == 0 || solver_opt == 3) && !(stop_flag && *stop_flag) ? single_pose_problem(p, n_stages) : -1;
    if (freep >= 0) {                     // one free pose, fixed points: the whole staged optimisation is one kernel
        PoseBatch b;
        double p7[7]; pose_from_T(p->poses + 16 * (size_t)freep, p7);
        b.pose.assign(p7, p7 + 7);
        std::vector<double> camt; cam_table(p, camt);
        b.cam.assign(&camt[5 * (size_t)freep], &camt[5 * (size_t)freep] + 5);
        for (int i = 0; i < E; i++) {
            const CorbBAEdge& e = p->edges[i];
            for (int a = 0; a < 3; a++) b.pt.push_back((double)p->points[3 * (size_t)e.point + a]);
            b.obs.push_back(e.u); b.obs.push_back(e.v); b.obs.push_back(e.u_right); b.w.push_back(e.inv_sigma2); b.dim.push_back(e.u_right < 0 ? 2 : 3);
        }
        b.edge_off.push_back(E);
        std::vector<double> pose; std::vector<unsigned char> act; std::vector<int> cnt;
        rc = pose_batch_run(b, stages, n_stages, pose, act, cnt, &r->ms_total);
        r->chi2 = chi_hist; r->lambda = lam_hist;
        if (rc) return rc;
        r->iters_done = cnt[0]; r->trials_total = cnt[1]; r->solver_used = 3;
        memcpy(r->poses, p->poses, sizeof(float) * 16 * (size_t)p->n_poses);
        memcpy(r->points, p->points, sizeof(float) * 3 * (size_t)p->n_points);
        if (cnt[2]) pose_to_T(pose.data(), r->poses + 16 * (size_t)freep);
        if (edge_outlier) for (int i = 0; i < E; i++) edge_outlier[i] = act[i] ? 0 : 1;
        return CORB_OK;
    }
    if (solver_opt == 3) { corb_set_error("corb_ba_solve_staged: solver 3 (fused single-pose kernel) needs one free pose, fixed points, <= %d stages", CORB_POSE_MAX_STAGES); return CORB_ERR_ARG; }
    if (stop_flag && *stop_flag) {                       // `if(pbStopFlag) if(*pbStopFlag) return;` before the first optimize() (Optimizer.cc:706-708): nothing is touched
        r->chi2 = chi_hist; r->lambda = lam_hist;
        memcpy(r->poses, p->poses, sizeof(float) * 16 * (size_t)p->n_poses); memcpy(r->points, p->points, sizeof(float) * 3 * (size_t)p->n_points);
        if (edge_outlier) memset(edge_outlier, 0, (size_t)E);
        return CORB_OK;
    }
    {   // local windows whose edges come grouped by point: flattened, optimised and classified on the device (round 5; see ba_staged_window_host)
        int applicable = 0;
        rc = ba_staged_window_host(p, stages, n_stages, stop_flag, r, edge_outlier, opt, &applicable);
        if (rc || applicable) { r->chi2 = chi_hist; r->lambda = lam_hist; return rc; }
    }
    BAState st; state_from_floats(p, st);
    const BAState st0 = st;
    std::vector<uint8_t> active(E ? E : 1, 1), pose_touched(p->n_poses ? p->n_poses : 1, 0), pt_touched(p->n_points ? p->n_points : 1, 0);
    std::vector<double> last(E ? E : 1, 0.0), fresh, depth;
    // the chi2 thresholds are decimal literals (5.991, 7.815) that the reference compares as doubles unless it first narrows chi2 to float
    auto th_double = [](float t) { return std::round((double)t * 1e6) / 1e6; };
    BASession sess;                                        // the first optimize() leaves its graph on the device for the later ones
    {
        bool resets = false; for (int s = 1; s < n_stages; s++) resets = resets || stages[s].reset_estimates != 0;
        static const bool host_stages = getenv("CORB_BA_HOST_STAGES") != nullptr;      // (the classifications on the host, as before round 5: for A/B timing)
        sess.want_dev = n_stages > 1 && !resets && !host_stages; sess.n_sets = n_stages + 1;
    }
    int n_opt = 0;                                         // optimize() calls done
    for (int s = 0; s < n_stages; s++) {
        if (stages[s].reset_estimates) st = st0;
        if (sess.ready && sess.dev) rc = ba_optimize_session_dev(sess, stages[s].iterations, stages[s].robust, stop_flag, r, (double)stages[s].huber_mono, (double)stages[s].huber_stereo);
        else
        rc = ba_optimize_device(p, active.data(), st, stages[s].iterations, stages[s].robust, stop_flag, r, device, opt, &last, &pose_touched, &pt_touched,
                                (double)stages[s].huber_mono, (double)stages[s].huber_stereo, n_stages > 1 ? &sess : nullptr);
        if (rc) break;
        n_opt++;
        // pbStopFlag raised during / after this optimize(): the remaining optimize() calls (and the classifications between them) are skipped, but the
        // caller's FINAL test still runs on every edge with the chi2 it last computed and a fresh depth (LocalBundleAdjustment: bDoMore = false
        // only skips the second round, the "Check inlier observations" pass that fills vToErase and the write-back follow; Optimizer.cc:712-800)
        const bool stopped = stop_flag && *stop_flag;
        const CorbBAStage& cs = stopped ? stages[n_stages - 1] : stages[s];
        if (sess.ready && sess.dev) { rc = ba_classify_session_dev(sess, cs); if (rc || stopped) break; continue; }
        const bool need_eval = cs.check_depth || cs.recompute_inactive;
        if (need_eval) { rc = sess.ready ? ba_eval_session(p, sess, fresh, depth) : ba_eval_edges_device(p, st.q, st.t, st.pt, fresh, depth); if (rc) break; }
        for (int i = 0; i < E; i++) {
            if (!active[i] && cs.recompute_inactive) last[i] = fresh[i];
            if (!active[i] && !cs.allow_reactivate) continue;
            const float thf = p->edges[i].u_right < 0 ? cs.chi2_mono : cs.chi2_stereo;
            bool out = cs.float_compare ? ((float)last[i] > thf) : (last[i] > th_double(thf));
            if (cs.check_depth && !(depth[i] > 0.0)) out = true;
            active[i] = out ? 0 : 1;
        }
        if (stopped) break;
    }
    r->chi2 = chi_hist; r->lambda = lam_hist;
    if (rc) return rc;
    if (sess.ready && sess.dev) {                          // the one read-back of a dev session: the estimates and the active sets
        BAFlat& f = sess.f; Pool& pool = *sess.pool;
        const size_t n_state = f.n_q + f.n_t + f.n_pt; const int nE = f.nE, n_sets = sess.cur_set + 1;
        static thread_local std::vector<double> back; static thread_local std::vector<uint8_t> sets;
        back.resize(n_state ? n_state : 1); sets.resize((size_t)n_sets * (nE ? nE : 1));
        if (n_state) HIPCHK(pool.d2h(back.data(), f.dq, n_state * 8));
        if (nE && n_sets > 1) HIPCHK(pool.d2h(sets.data() + nE, sess.d_act + nE, (size_t)(n_sets - 1) * nE));
        if (nE) memset(sets.data(), 1, (size_t)nE);
        HIPCHK(pool.fetch_finish());
        if (f.n_q) memcpy(st.q.data(), back.data(), f.n_q * 8);
        if (f.n_t) memcpy(st.t.data(), back.data() + f.n_q, f.n_t * 8);
        if (f.n_pt) memcpy(st.pt.data(), back.data() + f.n_q + f.n_t, f.n_pt * 8);
        // optimize() call k ran on set k (set 0 = every edge: the flattening marked its vertices)
        for (int k = 1; k < n_opt && k < n_sets; k++) {
            const uint8_t* a = sets.data() + (size_t)k * nE; int n_active = 0;
            for (int j = 0; j < nE; j++) if (a[j]) { const CorbBAEdge& e = p->edges[sess.act[j]]; pose_touched[e.pose] = 1; pt_touched[e.point] = 1; n_active++; }
            if (k == n_opt - 1) r->active_edges = n_active;
        }
        const uint8_t* fin = sets.data() + (size_t)sess.cur_set * nE;
        for (int j = 0; j < nE; j++) active[sess.act[j]] = fin[j];
    }
    if (edge_outlier) for (int i = 0; i < E; i++) edge_outlier[i] = active[i] ? 0 : 1;
    state_to_floats(p, st, pose_touched, pt_touched, r);
    return CORB_OK;
}

// ---- problems whose arrays live in device memory (corb_ba_store.cpp) ----
#include "ba_device_problem.h"
#include "ba_flatten.h"
#include "device_util.h"
// solver / preconditioner choice of a call (the rules of ba_optimize_device, stated once for the device path)
static int ba_choose(const CorbBAOptions* opt, int nP, int nE, int nL, BAChoice& ch)
{
    int solver = opt ? opt->solver : 0;
    if (solver < 0 || solver > 2) { corb_set_error("corb_ba_solve: bad solver option"); return CORB_ERR_ARG; }
    if (solver == 0) solver = nP <= 256 ? 1 : 2;
    ch.pcg_forcing = !(opt && opt->pcg_tol > 0) && nP > BA_PCG_FORCING_MIN_POSES; ch.pcg_tol = (opt && opt->pcg_tol > 0) ? opt->pcg_tol : BA_PCG_TOL_TIGHT;
    ch.pcg_max_iter = (opt && opt->pcg_max_iter > 0) ? opt->pcg_max_iter : 4000;
    int pc_g = (opt && opt->pc_block > 0) ? opt->pc_block : (nP >= 128 ? 16 : 1);
    if (pc_g > 1 && pc_g != 8 && pc_g != 16) { corb_set_error("corb_ba_solve: pc_block must be 1, 8 or 16"); return CORB_ERR_ARG; }
    if (solver != 2) pc_g = 1;
    const int sp = 6 * nP;
    if (solver == 1 && (double)sp * sp * 8.0 > 96e9) { corb_set_error("corb_ba_solve: %d free poses need a %.1f GB dense reduced system; use the PCG solver", nP, (double)sp * sp * 8e-9); return CORB_ERR_ARG; }
    ch.solver = solver; ch.pc_g = pc_g;
    ch.multilevel = solver == 2 && pc_g == BA_ML_G && (opt && opt->pc_multilevel ? opt->pc_multilevel == 2 : nP >= BA_ML_AUTO_POSES);
    static const int small_edges = corb_dev_env("CORB_BA_SMALL_EDGES") ? atoi(corb_dev_env("CORB_BA_SMALL_EDGES")) : BA_SMALL_EDGES;
    ch.fused_small = solver == 1 && sp <= BA_SMALL_SP && nE <= small_edges && nL <= small_edges && (opt == nullptr || opt->solver != 1);
    return CORB_OK;
}

int corb_ba_solve_device(const CorbBADeviceProblem* dp, int iterations, int robust, volatile int* stop_flag, CorbBAResult* r, int device, const CorbBAOptions* opt)
{
    if (!dp || !r || dp->n_poses < 0 || dp->n_points < 0 || dp->n_edges < 0 || iterations < 0) { corb_set_error("corb_ba_solve_device: bad argument"); return CORB_ERR_ARG; }
    int rc = corb_select_device(device); if (rc) return rc;
    r->iters_done = 0; r->trials_total = 0; r->ms_total = r->ms_build = r->ms_schur = r->ms_solve = r->ms_update = 0;
    r->solver_used = 0; r->pcg_iterations = 0; r->free_poses = r->free_points = r->active_edges = r->pc_block = r->pc_levels = 0; r->nnz_blocks = r->schur_pairs = 0; r->pcg_residual_max = r->pcg_residual_last = 0.0; r->grad_inf = -1.0; r->pcg_refined_trials = 0; r->reserved0 = 0;
    Lap lap;
    const int K = dp->n_poses, M = dp->n_points;
    Pool pool;
    if (!pool.stream) { corb_set_error("BA workspace: stream creation failed"); return CORB_ERR_HIP; }
    hipStream_t s = pool.stream;
    BAFlattenDev d; memset(&d, 0, sizeof(d));
    d.K = K; d.M = M; d.E = dp->n_edges;
    d.poses = dp->poses; d.pose_fixed = dp->pose_fixed; d.points = dp->points; d.point_fixed = dp->point_fixed; d.edges = dp->edges; d.intr = dp->intr; d.edge_off = dp->edge_off;
    HIPCHK(pool.alloc(&d.lflag, (size_t)M + 1)); HIPCHK(pool.alloc(&d.cntA, (size_t)M + 1)); HIPCHK(pool.alloc(&d.cntB, (size_t)M + 1)); HIPCHK(pool.alloc(&d.nfree_pt, (size_t)M + 1));
    HIPCHK(pool.alloc(&d.lidx, (size_t)M + 1)); HIPCHK(pool.alloc(&d.eoffA, (size_t)M + 1)); HIPCHK(pool.alloc(&d.eoffB, (size_t)M + 1));
    HIPCHK(pool.alloc(&d.pflag, (size_t)K + 1)); HIPCHK(pool.alloc(&d.pidx, (size_t)K + 1)); HIPCHK(pool.alloc(&d.pt_touched, (size_t)M + 1));
    HIPCHK(pool.alloc(&d.scal, FLAT_NSCAL));
    int* scan_tmp; HIPCHK(pool.alloc(&scan_tmp, corb_scan_scratch_ints((size_t)std::max(std::max(K, M), 1))));
    HIPCHK(hipMemsetAsync(d.scal, 0, sizeof(int) * FLAT_NSCAL, s));
    // 1. active edges per point; hessian indices; edge offsets
    flat_launch_points(d, s);
    corb_launch_exclusive_scan(d.lflag, d.lidx, (size_t)M, scan_tmp, s);
    corb_launch_exclusive_scan(d.cntA, d.eoffA, (size_t)M, scan_tmp, s);
    corb_launch_exclusive_scan(d.cntB, d.eoffB, (size_t)M, scan_tmp, s);
    corb_launch_exclusive_scan(d.pflag, d.pidx, (size_t)K, scan_tmp, s);
    HIPCHK(hipGetLastError());
    int* h = static_cast<int*>(pool.pinned());
    HIPCHK(hipMemcpyAsync(h + 0, d.lidx + M, 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(h + 1, d.eoffA + M, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h + 2, d.eoffB + M, 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(h + 3, d.pidx + K, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    BAFlat f;
    f.nL = h[0]; f.nE = h[1] + h[2]; f.nP = h[3]; f.nA = h[1];
    const int nE = f.nE, nP = f.nP, nL = f.nL;
    if (h[1] < 0 || h[2] < 0 || nE < 0) { corb_set_error("corb_ba_solve_device: more than 2^31 observations"); return CORB_ERR_ARG; }
    BAChoice ch; rc = ba_choose(opt, nP, nE, nL, ch); if (rc) return rc;
    r->solver_used = ch.solver; r->free_poses = nP; r->free_points = nL; r->pc_block = ch.solver == 2 ? ch.pc_g : 0; r->active_edges = nE;
    lap("device: counts");
    // 2. the sorted structure-of-arrays edges, landmark ranges, estimates
    f.n_q = 4 * (size_t)K; f.n_t = 3 * (size_t)K; f.n_pt = 3 * (size_t)M;
    const size_t n_state = f.n_q + f.n_t + f.n_pt;
    HIPCHK(pool.alloc(&f.dq, n_state)); HIPCHK(pool.alloc(&f.dq_bak, n_state));
    HIPCHK(pool.alloc(&f.e_pose, (size_t)nE)); HIPCHK(pool.alloc(&f.e_point, (size_t)nE)); HIPCHK(pool.alloc(&f.e_vpose, (size_t)nE)); HIPCHK(pool.alloc(&f.e_vpoint, (size_t)nE));
    HIPCHK(pool.alloc(&f.e_obs, 3 * (size_t)nE)); HIPCHK(pool.alloc(&f.e_w, (size_t)nE)); HIPCHK(pool.alloc(&f.e_dim, (size_t)nE));
    HIPCHK(pool.alloc(&f.loff, (size_t)nL + 1)); HIPCHK(pool.alloc(&f.lnfree, (size_t)nL + 1)); HIPCHK(pool.alloc(&f.poff, (size_t)nP + 1));
    HIPCHK(pool.alloc(&f.pose_vertex, (size_t)nP + 1)); HIPCHK(pool.alloc(&f.point_vertex, (size_t)nL + 1)); HIPCHK(pool.alloc(&f.cam, 5 * (size_t)std::max(K, 1)));
    HIPCHK(pool.alloc(&d.pcnt, (size_t)nP + 1)); HIPCHK(pool.alloc(&d.pcur, (size_t)nP + 1));
    HIPCHK(hipMemsetAsync(d.pcnt, 0, sizeof(int) * ((size_t)nP + 1), s)); HIPCHK(hipMemsetAsync(d.pcur, 0, sizeof(int) * ((size_t)nP + 1), s));
    HIPCHK(hipMemsetAsync(f.loff, 0, sizeof(int) * ((size_t)nL + 1), s));
    d.e_pose = f.e_pose; d.e_point = f.e_point; d.e_vpose = f.e_vpose; d.e_vpoint = f.e_vpoint; d.e_obs = f.e_obs; d.e_w = f.e_w; d.e_dim = f.e_dim;
    d.loff = f.loff; d.lnfree = f.lnfree; d.poff = f.poff; d.pose_vertex = f.pose_vertex; d.point_vertex = f.point_vertex; d.cam = f.cam; d.state = f.dq;
    // maps: counts and places from one pass with workgroup-aggregated atomics (flat_pose_count_kernel); small graphs keep the per-edge / per-wavefront atomics
    const bool agg_lists = nE >= (1 << 18);
    if (agg_lists) HIPCHK(pool.alloc(&d.erel, (size_t)nE));
    flat_launch_state_in(d, s);
    flat_launch_edges(d, s);
    if (agg_lists) flat_launch_pose_count(d, nE, s);
    // 3. per-keyframe edge lists, ascending
    corb_launch_exclusive_scan(d.pcnt, f.poff, (size_t)nP, scan_tmp, s);
    HIPCHK(hipGetLastError());
    int n_pe = 0;
    HIPCHK(hipMemcpyAsync(h + 4, f.poff + nP, 4, hipMemcpyDeviceToHost, s));
    if (agg_lists) HIPCHK(hipMemcpyAsync(h + 5, d.scal + FLAT_MAXLIST, 4, hipMemcpyDeviceToHost, s));      // (the longest list is known with the counts: one wait less)
    HIPCHK(hipStreamSynchronize(s));
    n_pe = h[4];
    HIPCHK(pool.alloc(&f.pedge, (size_t)n_pe)); HIPCHK(pool.alloc(&f.plm, (size_t)n_pe));
    d.pedge = f.pedge; d.plm = f.plm;
    if (agg_lists) flat_launch_pose_fill(d, nE, s);
    else {
    flat_launch_pose_lists(d, nE, s);
    HIPCHK(hipMemcpyAsync(h + 5, d.scal + FLAT_MAXLIST, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    }
    if (flat_launch_pose_sort(d, nP, h[5], s) != 0) { corb_set_error("corb_ba_solve_device: a keyframe has %d observations (the device flattening sorts up to 16 384 per keyframe)", h[5]); return CORB_ERR_CAPACITY; }
    HIPCHK(hipGetLastError());
    lap("device: edges + lists");
    // 4. block pattern of the reduced camera system
    const bool want_pattern = ch.solver == 2 || !ch.fused_small;
    ch.want_pattern = want_pattern; f.have_pattern = want_pattern;
    if (want_pattern && nP > 0) {
        if ((size_t)((nP + 31) / 32) * 4 > 64 * 1024) { corb_set_error("corb_ba_solve_device: more than 524 288 free keyframes"); return CORB_ERR_CAPACITY; }
        HIPCHK(pool.alloc(&d.rowcnt, (size_t)nP + 1)); HIPCHK(pool.alloc(&d.ucnt, (size_t)nP + 1)); HIPCHK(pool.alloc(&d.ubase, (size_t)nP + 1));
        HIPCHK(pool.alloc(&f.bsr_rowptr, (size_t)nP + 1)); HIPCHK(pool.alloc(&f.bsr_diag, (size_t)nP));
        d.bsr_rowptr = f.bsr_rowptr; d.bsr_diag = f.bsr_diag;
        flat_launch_rows(d, nP, false, s);
        corb_launch_exclusive_scan(d.rowcnt, f.bsr_rowptr, (size_t)nP, scan_tmp, s);
        corb_launch_exclusive_scan(d.ucnt, d.ubase, (size_t)nP, scan_tmp, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h + 7, f.bsr_rowptr + nP, 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(h + 8, d.ubase + nP, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h + 9, d.scal + FLAT_MAXROW, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (h[7] < 0) { corb_set_error("corb_ba_solve_device: more than 2^31 blocks in the reduced camera system"); return CORB_ERR_ARG; }
        f.nnzb = h[7]; f.nu = h[8]; f.bsr_max_row = h[9];
        HIPCHK(pool.alloc(&f.bsr_col, (size_t)f.nnzb)); HIPCHK(pool.alloc(&f.uinfo, 4 * (size_t)f.nu));
        d.bsr_col = f.bsr_col; d.uinfo = f.uinfo;
        flat_launch_rows(d, nP, true, s);
        HIPCHK(hipGetLastError());
    }
    r->nnz_blocks = f.nnzb; r->schur_pairs = 0;
    lap("device: block pattern");
    // 5. optimize(), then the estimates back into the problem's float arrays
    rc = ba_lm_device(pool, f, ch, iterations, robust, stop_flag, r, (double)(float)std::sqrt(5.99), (double)(float)std::sqrt(7.815), lap, nullptr);
    if (rc) return rc;
    flat_launch_state_out(d, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    lap("device: write back");
    return CORB_OK;
}

bool corb_ba_staged_device_wanted(const CorbBAStage* stages, int n_stages)
{
    static const bool host_route = getenv("CORB_LBA_HOST_FLATTEN") != nullptr;      // (the round-4 route -- problem to the host, host flattening --: for A/B timing)
    if (host_route || n_stages < 1 || n_stages > FLAT_MAX_STAGES) return false;     // (flat_launch_fixed_edge_outliers replays every stage that ran)
    for (int s = 1; s < n_stages; s++) if (stages[s].reset_estimates) return false;
    return true;
}
static int ba_staged_window(BASession& sess, const CorbBADeviceProblem* dp, const CorbBAStage* stages, int n_stages, volatile int* stop_flag, CorbBAResult* r, uint8_t* d_outlier,
                            const int* d_status, int* n_edges_out, int* status_out, const CorbBAOptions* opt, int* applicable);
int corb_ba_staged_device(const CorbBADeviceProblem* dp, const CorbBAStage* stages, int n_stages, volatile int* stop_flag, CorbBAResult* r, uint8_t* d_outlier,
                          hipEvent_t ready, const int* d_status, int* n_edges_out, int* status_out, int device, const CorbBAOptions* opt, int* applicable)
{
    if (!dp || !r || !stages || !applicable || !d_outlier || !n_edges_out || !status_out || n_stages < 1 || dp->n_poses <= 0 || dp->n_points <= 0) { corb_set_error("corb_ba_staged_device: bad argument"); return CORB_ERR_ARG; }
    *applicable = 0; *n_edges_out = dp->n_edges; *status_out = 0;
    int rc = corb_select_device(device); if (rc) return rc;
    BASession sess; sess.pool.reset(new Pool());
    if (!sess.pool->stream) { corb_set_error("BA workspace: stream creation failed"); return CORB_ERR_HIP; }
    if (ready) HIPCHK(hipStreamWaitEvent(sess.pool->stream, ready, 0));
    return ba_staged_window(sess, dp, stages, n_stages, stop_flag, r, d_outlier, d_status, n_edges_out, status_out, opt, applicable);
}
// The same for a window given in HOST memory (corb_ba_solve_staged: the host-pointer form of LocalBundleAdjustment), when its edges come grouped by point -- the order in
// which Optimizer.cc:560-640 creates them (per local map point its observations).  The raw arrays go up as one block (32 bytes per edge: less than the flattened arrays
// the host route uploads), the flattening runs on the device, and the estimates and flags come back in one block: the host flattening (0.2 - 0.3 ms of a window's call)
// is not on the path.  *applicable = 0: declined, nothing written.
static int ba_staged_window_host(const CorbBAProblem* p, const CorbBAStage* stages, int n_stages, volatile int* stop_flag, CorbBAResult* r, uint8_t* edge_outlier,
                                 const CorbBAOptions* opt, int* applicable)
{
    *applicable = 0;
    const int K = p->n_poses, M = p->n_points, E = p->n_edges;
    if (!corb_ba_staged_device_wanted(stages, n_stages) || K <= 0 || M <= 0 || E <= BA_SMALL_EDGES || E > (1 << 20) || (stop_flag && *stop_flag)) return CORB_OK;
    int n_free = 0; for (int k = 0; k < K; k++) n_free += p->pose_fixed[k] ? 0 : 1;
    if (n_free <= 0 || n_free > 64 || (opt && opt->solver == 2)) return CORB_OK;
    for (int i = 1; i < E; i++) if (p->edges[i].point < p->edges[i - 1].point) return CORB_OK;      // (not grouped by point: the host flattening sorts)
    BASession sess; sess.pool.reset(new Pool());
    Pool& pool = *sess.pool;
    if (!pool.stream) { corb_set_error("BA workspace: stream creation failed"); return CORB_ERR_HIP; }
    hipStream_t s = pool.stream;
    static thread_local std::vector<float> intr;
    intr.resize(5 * (size_t)K);
    for (int k = 0; k < K; k++) for (int a = 0; a < 5; a++) intr[5 * (size_t)k + a] = p->intr ? p->intr[5 * (size_t)k + a] : (a == 0 ? p->fx : a == 1 ? p->fy : a == 2 ? p->cx : a == 3 ? p->cy : p->bf);
    CorbBADeviceProblem dp; memset(&dp, 0, sizeof(dp));
    dp.n_poses = K; dp.n_points = M; dp.n_edges = E;
    float *d_poses, *d_points, *d_intr; uint8_t *d_pf, *d_xf, *d_outl; CorbBAEdge* d_edges; int* d_off;
    HIPCHK(pool.upload_block({{(void**)&d_poses, p->poses, sizeof(float) * 16 * (size_t)K}, {(void**)&d_points, p->points, sizeof(float) * 3 * (size_t)M}, {(void**)&d_intr, intr.data(), sizeof(float) * 5 * (size_t)K},
                              {(void**)&d_pf, p->pose_fixed, (size_t)K}, {(void**)&d_xf, p->point_fixed, (size_t)M}, {(void**)&d_edges, p->edges, sizeof(CorbBAEdge) * (size_t)E}}));
    HIPCHK(pool.alloc(&d_off, (size_t)M + 1)); HIPCHK(pool.alloc(&d_outl, (size_t)E));
    ba_launch_edge_offsets(d_edges, E, M, d_off, s);
    HIPCHK(hipGetLastError());
    dp.poses = d_poses; dp.pose_fixed = d_pf; dp.points = d_points; dp.point_fixed = d_xf; dp.edges = d_edges; dp.intr = d_intr; dp.edge_off = d_off;
    int n_edges = E, status = 0;
    int rc = ba_staged_window(sess, &dp, stages, n_stages, stop_flag, r, d_outl, nullptr, &n_edges, &status, opt, applicable);
    if (rc || !*applicable) return rc;
    HIPCHK(pool.d2h(r->poses, d_poses, sizeof(float) * 16 * (size_t)K)); HIPCHK(pool.d2h(r->points, d_points, sizeof(float) * 3 * (size_t)M));
    if (edge_outlier) HIPCHK(pool.d2h(edge_outlier, d_outl, (size_t)E));
    HIPCHK(pool.fetch_finish());
    return CORB_OK;
}
static int ba_staged_window(BASession& sess, const CorbBADeviceProblem* dp, const CorbBAStage* stages, int n_stages, volatile int* stop_flag, CorbBAResult* r, uint8_t* d_outlier,
                            const int* d_status, int* n_edges_out, int* status_out, const CorbBAOptions* opt, int* applicable)
{
    const int K = dp->n_poses, M = dp->n_points;
    int rc = CORB_OK;
    Lap lap;
    Pool& pool = *sess.pool;
    hipStream_t s = pool.stream;
    BAFlattenDev d; memset(&d, 0, sizeof(d));
    d.K = K; d.M = M; d.E = dp->n_edges;
    d.poses = dp->poses; d.pose_fixed = dp->pose_fixed; d.points = dp->points; d.point_fixed = dp->point_fixed; d.edges = dp->edges; d.intr = dp->intr; d.edge_off = dp->edge_off;
    HIPCHK(pool.alloc(&d.lflag, (size_t)M + 1)); HIPCHK(pool.alloc(&d.cntA, (size_t)M + 1)); HIPCHK(pool.alloc(&d.cntB, (size_t)M + 1)); HIPCHK(pool.alloc(&d.nfree_pt, (size_t)M + 1));
    HIPCHK(pool.alloc(&d.lidx, (size_t)M + 1)); HIPCHK(pool.alloc(&d.eoffA, (size_t)M + 1)); HIPCHK(pool.alloc(&d.eoffB, (size_t)M + 1));
    HIPCHK(pool.alloc(&d.pflag, (size_t)K + 1)); HIPCHK(pool.alloc(&d.pidx, (size_t)K + 1)); HIPCHK(pool.alloc(&d.pt_touched, (size_t)M + 1));
    HIPCHK(pool.alloc(&d.scal, FLAT_NSCAL));
    int* scan_tmp; HIPCHK(pool.alloc(&scan_tmp, corb_scan_scratch_ints((size_t)std::max(std::max(K, M), 1))));
    HIPCHK(hipMemsetAsync(d.scal, 0, sizeof(int) * FLAT_NSCAL, s));
    // 1. active edges per point; hessian indices; edge offsets -- and the one read-back of the flattening: the counts
    flat_launch_points(d, s);
    {
        const int* in4[4] = {d.lflag, d.cntA, d.cntB, d.pflag}; int* out4[4] = {d.lidx, d.eoffA, d.eoffB, d.pidx}; const size_t n4[4] = {(size_t)M, (size_t)M, (size_t)M, (size_t)K};
        if (!corb_launch_exclusive_scan4(in4, out4, n4, 4, s)) {
            corb_launch_exclusive_scan(d.lflag, d.lidx, (size_t)M, scan_tmp, s);
            corb_launch_exclusive_scan(d.cntA, d.eoffA, (size_t)M, scan_tmp, s);
            corb_launch_exclusive_scan(d.cntB, d.eoffB, (size_t)M, scan_tmp, s);
            corb_launch_exclusive_scan(d.pflag, d.pidx, (size_t)K, scan_tmp, s);
        }
    }
    HIPCHK(hipGetLastError());
    int* h = static_cast<int*>(pool.pinned());
    int* d_counts; HIPCHK(pool.alloc(&d_counts, 8));
    flat_launch_counts(d, d_status, d_counts, s);
    HIPCHK(hipMemcpyAsync(h, d_counts, 8 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    BAFlat f;
    f.nL = h[0]; f.nE = h[1] + h[2]; f.nP = h[3]; f.nA = h[1];
    const int nE = f.nE, nP = f.nP, nL = f.nL; const int pairs_sum = h[4];
    const int n_edges = h[5];
    *n_edges_out = n_edges; *status_out = h[6];
    if (h[6] != 0 || n_edges <= 0 || (dp->n_edges >= 0 && dp->n_edges != n_edges) || (stop_flag && *stop_flag)) return CORB_OK;      // (the caller looks at the status word; declined: nothing was touched)
    if (h[1] < 0 || h[2] < 0 || nE <= 0 || nP <= 0 || nL <= 0 || nP > 64 || pairs_sum < 0 || pairs_sum > (1 << 22)) return CORB_OK;
    BAChoice ch; rc = ba_choose(opt, nP, nE, nL, ch); if (rc) return rc;
    if (ch.solver != 1 || ch.fused_small) return CORB_OK;
    *applicable = 1;
    r->iters_done = 0; r->trials_total = 0; r->ms_total = r->ms_build = r->ms_schur = r->ms_solve = r->ms_update = 0;
    r->pcg_iterations = 0; r->pc_levels = 0; r->schur_pairs = 0; r->pcg_residual_max = r->pcg_residual_last = 0.0; r->grad_inf = -1.0; r->pcg_refined_trials = 0; r->reserved0 = 0;
    r->solver_used = ch.solver; r->free_poses = nP; r->free_points = nL; r->pc_block = 0; r->active_edges = nE; r->reserved0 = 1;      // (the device route ran)
    double* chi_hist = r->chi2; double* lam_hist = r->lambda; r->chi2 = nullptr; r->lambda = nullptr;     // histories are per optimize() call
    struct Hist { CorbBAResult* r; double* c; double* l; ~Hist() { r->chi2 = c; r->lambda = l; } } hist_back{r, chi_hist, lam_hist};
    lap("window: counts");
    // 2. the sorted structure-of-arrays edges, landmark ranges, estimates; per-keyframe lists (their total is at most nE, the longest at most max_list)
    f.n_q = 4 * (size_t)K; f.n_t = 3 * (size_t)K; f.n_pt = 3 * (size_t)M;
    const size_t n_state = f.n_q + f.n_t + f.n_pt;
    HIPCHK(pool.alloc(&f.dq, n_state)); HIPCHK(pool.alloc(&f.dq_bak, n_state));
    HIPCHK(pool.alloc(&f.e_pose, (size_t)nE)); HIPCHK(pool.alloc(&f.e_point, (size_t)nE)); HIPCHK(pool.alloc(&f.e_vpose, (size_t)nE)); HIPCHK(pool.alloc(&f.e_vpoint, (size_t)nE));
    HIPCHK(pool.alloc(&f.e_obs, 3 * (size_t)nE)); HIPCHK(pool.alloc(&f.e_w, (size_t)nE)); HIPCHK(pool.alloc(&f.e_dim, (size_t)nE)); HIPCHK(pool.alloc(&d.e_src, (size_t)nE));
    HIPCHK(pool.alloc(&f.loff, (size_t)nL + 1)); HIPCHK(pool.alloc(&f.lnfree, (size_t)nL + 1)); HIPCHK(pool.alloc(&f.poff, (size_t)nP + 1));
    HIPCHK(pool.alloc(&f.pose_vertex, (size_t)nP + 1)); HIPCHK(pool.alloc(&f.point_vertex, (size_t)nL + 1)); HIPCHK(pool.alloc(&f.cam, 5 * (size_t)std::max(K, 1)));
    HIPCHK(pool.alloc(&d.pcnt, 2 * ((size_t)nP + 1))); d.pcur = d.pcnt + nP + 1;
    HIPCHK(hipMemsetAsync(d.pcnt, 0, sizeof(int) * 2 * ((size_t)nP + 1), s));
    HIPCHK(hipMemsetAsync(f.loff, 0, sizeof(int) * ((size_t)nL + 1), s));
    d.e_pose = f.e_pose; d.e_point = f.e_point; d.e_vpose = f.e_vpose; d.e_vpoint = f.e_vpoint; d.e_obs = f.e_obs; d.e_w = f.e_w; d.e_dim = f.e_dim;
    d.loff = f.loff; d.lnfree = f.lnfree; d.poff = f.poff; d.pose_vertex = f.pose_vertex; d.point_vertex = f.point_vertex; d.cam = f.cam; d.state = f.dq;
    flat_launch_state_in(d, s);
    flat_launch_edges(d, s, nP);
    corb_launch_exclusive_scan(d.pcnt, f.poff, (size_t)nP, scan_tmp, s);
    HIPCHK(pool.alloc(&f.pedge, (size_t)nE)); HIPCHK(pool.alloc(&f.plm, (size_t)nE));
    d.pedge = f.pedge; d.plm = f.plm;
    flat_launch_pose_lists_ordered(d, nP, nE, s);          // (a workgroup per keyframe compacts its edges in order: the global path's atomics + sort took 75 us of a window's call)
    // 3. the full block pattern (the reduced system is dense: a block without a shared landmark has an empty pair list and stays zero)
    f.have_pattern = true; ch.want_pattern = true;
    f.nnzb = nP * nP; f.nu = nP * (nP + 1) / 2; f.bsr_max_row = nP; f.pairs_bound = (size_t)pairs_sum + 1;
    HIPCHK(pool.alloc(&f.bsr_rowptr, (size_t)nP + 1)); HIPCHK(pool.alloc(&f.bsr_diag, (size_t)nP)); HIPCHK(pool.alloc(&f.bsr_col, (size_t)f.nnzb)); HIPCHK(pool.alloc(&f.uinfo, 4 * (size_t)f.nu));
    d.bsr_rowptr = f.bsr_rowptr; d.bsr_diag = f.bsr_diag; d.bsr_col = f.bsr_col; d.uinfo = f.uinfo;
    flat_launch_full_pattern(d, nP, s);
    HIPCHK(hipGetLastError());
    r->nnz_blocks = f.nnzb;
    // 4. the session: information weights, chi2 memory, active sets (BASession); optimize() / classify, stage by stage
    sess.want_dev = true; sess.n_sets = n_stages + 1;
    HIPCHK(pool.alloc(&sess.d_w0, (size_t)nE)); HIPCHK(pool.alloc(&sess.d_last, (size_t)nE)); HIPCHK(pool.alloc(&sess.d_act, (size_t)sess.n_sets * nE));
    HIPCHK(hipMemcpyAsync(sess.d_w0, f.e_w, sizeof(double) * (size_t)nE, hipMemcpyDeviceToDevice, s));
    sess.f = f; sess.ch = ch; sess.covers_all = true; sess.ready = true; sess.dev = true; sess.cur_set = 0;
    lap("window: flattening enqueued");
    int n_opt = 0;
    std::vector<CorbBAStage> used_stages;                  // the classifications that ran, for the edges outside the graph (see flat_launch_fixed_edge_outliers)
    for (int st = 0; st < n_stages; st++) {
        rc = ba_optimize_session_dev(sess, stages[st].iterations, stages[st].robust, stop_flag, r, (double)stages[st].huber_mono, (double)stages[st].huber_stereo);
        if (rc) return rc;
        n_opt++;
        const bool stopped = stop_flag && *stop_flag;
        rc = ba_classify_session_dev(sess, stopped ? stages[n_stages - 1] : stages[st]); if (rc) return rc;
        used_stages.push_back(stopped ? stages[n_stages - 1] : stages[st]);
        if (stopped) break;
    }
    // 5. the estimates into the problem's float arrays, the outlier flags in the problem's edge order, the last optimize()'s active-edge count
    flat_launch_state_out(d, s);
    HIPCHK(hipMemsetAsync(d_outlier, 0, (size_t)n_edges, s));
    flat_launch_outliers(sess.d_act + (size_t)sess.cur_set * nE, d.e_src, nE, d_outlier, s);
    if (nE != n_edges) {                                   // (edges between two fixed vertices)
        BAFlattenDev dd = d; dd.E = n_edges;
        if (flat_launch_fixed_edge_outliers(dd, used_stages.data(), (int)used_stages.size(), d_outlier, s)) { corb_set_error("staged BA: %d stages, the device route replays at most %d", (int)used_stages.size(), FLAT_MAX_STAGES); return CORB_ERR_ARG; }
    }
    HIPCHK(hipGetLastError());
    if (n_opt > 1) {
        static thread_local std::vector<uint8_t> set; set.resize((size_t)nE);
        HIPCHK(pool.d2h(set.data(), sess.d_act + (size_t)(n_opt - 1) * nE, (size_t)nE));
        HIPCHK(pool.fetch_finish());
        int n_active = 0; for (int j = 0; j < nE; j++) n_active += set[j] ? 1 : 0;
        r->active_edges = n_active;
    } else HIPCHK(hipStreamSynchronize(s));
    lap("window: stages");
    return CORB_OK;
}

// the device flattening against the host flattening (tests): flattens a problem given in HOST memory on the device path -- upload, group by point, solve, download
extern "C" int corb_ba_solve_devflat(const CorbBAProblem* p, int iterations, int robust, CorbBAResult* r, int device, const CorbBAOptions* opt)
{
    int rc = validate(p, r); if (rc) return rc;
    if (!p->intr && p->n_poses > 0) { /* shared camera: replicate */ }
    rc = corb_select_device(device); if (rc) return rc;
    const size_t K = (size_t)p->n_poses, M = (size_t)p->n_points, E = (size_t)p->n_edges;
    // group the edges by point (stable), as corb_ba_solve_store's records deliver them
    std::vector<int> off(M + 1, 0); std::vector<CorbBAEdge> ge(E + 1);
    for (size_t i = 0; i < E; i++) off[(size_t)p->edges[i].point + 1]++;
    for (size_t m = 0; m < M; m++) off[m + 1] += off[m];
    { std::vector<int> cur(off.begin(), off.end() - 1); for (size_t i = 0; i < E; i++) ge[(size_t)cur[(size_t)p->edges[i].point]++] = p->edges[i]; }
    std::vector<float> intr(5 * K + 1);
    for (size_t k = 0; k < K; k++) for (int a = 0; a < 5; a++) intr[5 * k + a] = p->intr ? p->intr[5 * k + a] : (a == 0 ? p->fx : a == 1 ? p->fy : a == 2 ? p->cx : a == 3 ? p->cy : p->bf);
    struct Dev { std::vector<void*> v; ~Dev() { for (void* q : v) (void)hipFree(q); } void* get(size_t bytes) { void* q = nullptr; if (hipMalloc(&q, bytes ? bytes : 1) != hipSuccess) return nullptr; v.push_back(q); return q; } } dev;
    CorbBADeviceProblem dp; memset(&dp, 0, sizeof(dp));
    dp.n_poses = (int)K; dp.n_points = (int)M; dp.n_edges = (int)E;
    dp.poses = (float*)dev.get(64 * K); uint8_t* dpf = (uint8_t*)dev.get(K); dp.points = (float*)dev.get(12 * M); uint8_t* dxf = (uint8_t*)dev.get(M);
    CorbBAEdge* de = (CorbBAEdge*)dev.get(sizeof(CorbBAEdge) * E); float* di = (float*)dev.get(20 * K); int* doff = (int*)dev.get(4 * (M + 1));
    if (!dp.poses || !dpf || !dp.points || !dxf || !de || !di || !doff) { corb_set_error("corb_ba_solve_devflat: allocation failed"); return CORB_ERR_HIP; }
    dp.pose_fixed = dpf; dp.point_fixed = dxf; dp.edges = de; dp.intr = di; dp.edge_off = doff;
    if (K) { HIPCHK(hipMemcpy(dp.poses, p->poses, 64 * K, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dpf, p->pose_fixed, K, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(di, intr.data(), 20 * K, hipMemcpyHostToDevice)); }
    if (M) { HIPCHK(hipMemcpy(dp.points, p->points, 12 * M, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dxf, p->point_fixed, M, hipMemcpyHostToDevice)); }
    if (E) HIPCHK(hipMemcpy(de, ge.data(), sizeof(CorbBAEdge) * E, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(doff, off.data(), 4 * (M + 1), hipMemcpyHostToDevice));
    rc = corb_ba_solve_device(&dp, iterations, robust, nullptr, r, device, opt);
    if (rc) return rc;
    if (K) HIPCHK(hipMemcpy(r->poses, dp.poses, 64 * K, hipMemcpyDeviceToHost));
    if (M) HIPCHK(hipMemcpy(r->points, dp.points, 12 * M, hipMemcpyDeviceToHost));
    return CORB_OK;
}

// corb_ba.cpp -- C-ABI host side of the global bundle adjustment (see include/corb_accel.h).
// Follows Optimizer::BundleAdjustment (corbslam_client/src/Optimizer.cc:54-270): graph flattening, the
// g2o index mapping (free poses, then free landmarks, ascending id; G/core/sparse_optimizer.cpp:166-190),
// and the Levenberg-Marquardt control flow (G/core/optimization_algorithm_levenberg.cpp:61-164).  All
// per-edge / per-vertex arithmetic runs in ba_kernels.hip; the dense reduced camera system is factorised
// by the hand-written blocked Cholesky of dense_chol.hip.  The host only sequences launches and reads back 3 scalars per trial.
#include "ba_host.h"
#include "owned_hip.h"
#include <algorithm>
#include <atomic>
#include <mutex>

int ba_validate(const CorbBAProblem* p, const CorbBAResult* r)
{
    if (!p || !r || !r->poses || !r->points || p->n_poses < 0 || p->n_points < 0 || p->n_edges < 0 ||
        (p->n_poses > 0 && (!p->poses || !p->pose_fixed)) || (p->n_points > 0 && (!p->points || !p->point_fixed)) || (p->n_edges > 0 && !p->edges)) {
        corb_set_error("corb_ba_solve: bad argument"); return CORB_ERR_ARG;
    }
    for (int i = 0; i < p->n_edges; i++)
        if (p->edges[i].pose < 0 || p->edges[i].pose >= p->n_poses || p->edges[i].point < 0 || p->edges[i].point >= p->n_points) { corb_set_error("corb_ba_solve: edge %d out of range", i); return CORB_ERR_ARG; }
    return CORB_OK;
}

void ba_result_reset(CorbBAResult* r)
{
    r->iters_done = 0; r->trials_total = 0; r->ms_total = r->ms_build = r->ms_schur = r->ms_solve = r->ms_update = 0;
    r->solver_used = 0; r->pcg_iterations = 0; r->free_poses = r->free_points = r->active_edges = r->pc_block = r->pc_levels = 0; r->nnz_blocks = r->schur_pairs = 0;
    r->pcg_residual_max = r->pcg_residual_last = 0.0; r->grad_inf = -1.0; r->pcg_refined_trials = 0; r->reserved0 = 0;
}

void ba_intrinsics(const CorbBAProblem* p, int k, float* c5)
{
    for (int a = 0; a < 5; a++) c5[a] = p->intr ? p->intr[5 * (size_t)k + a] : (a == 0 ? p->fx : a == 1 ? p->fy : a == 2 ? p->cx : a == 3 ? p->cy : p->bf);
}
// intrinsics of every pose vertex as doubles (e->fx = pKF->fx ... e->bf = pKF->mbf: float -> double, Optimizer.cc:160-163, 189-193)
void ba_cam_table(const CorbBAProblem* p, std::vector<double>& cam)
{
    cam.resize(5 * (size_t)(p->n_poses > 0 ? p->n_poses : 1));
    for (int k = 0; k < p->n_poses; k++) { float c[5]; ba_intrinsics(p, k, c); for (int a = 0; a < 5; a++) cam[5 * (size_t)k + a] = c[a]; }
}

// Converter::toSE3Quat per keyframe, the points as doubles
void ba_state_from_floats(const CorbBAProblem* p, BAState& st)
{
    const int K = p->n_poses, M = p->n_points;
    st.q.resize(4 * (size_t)K); st.t.resize(3 * (size_t)K); st.pt.resize(3 * (size_t)M);
    for (int k = 0; k < K; k++) {
        double p7[7]; corb_pose_from_T(p->poses + 16 * (size_t)k, p7);
        memcpy(&st.q[4 * (size_t)k], p7, 4 * sizeof(double)); memcpy(&st.t[3 * (size_t)k], p7 + 4, 3 * sizeof(double));
    }
    for (size_t i = 0; i < 3 * (size_t)M; i++) st.pt[i] = p->points[i];
}

// write-back: Converter::toCvMat (double -> float); fixed / never-optimised vertices are passed through
void ba_state_to_floats(const CorbBAProblem* p, const BAState& st, const std::vector<uint8_t>& pose_touched, const std::vector<uint8_t>& pt_touched, CorbBAResult* r)
{
    for (int k = 0; k < p->n_poses; k++) {
        float* T = r->poses + 16 * (size_t)k;
        if (p->pose_fixed[k] || !pose_touched[k]) { memcpy(T, p->poses + 16 * (size_t)k, 16 * sizeof(float)); continue; }
        double p7[7]; memcpy(p7, &st.q[4 * (size_t)k], 4 * sizeof(double)); memcpy(p7 + 4, &st.t[3 * (size_t)k], 3 * sizeof(double));
        corb_pose_to_T(p7, T);
    }
    for (int m = 0; m < p->n_points; m++) {
        const bool keep = p->point_fixed[m] || !pt_touched[m];
        for (int a = 0; a < 3; a++) r->points[3 * (size_t)m + a] = keep ? p->points[3 * (size_t)m + a] : (float)st.pt[3 * (size_t)m + a];
    }
}

// Solver / preconditioner choice of a call, for every route (host flattening, device flattening, windows).
// Dense or PCG: tools/ba_solver_sweep.py (round 3, dense_chol.hip: 17 / 36 / 62 ms per 10 iterations at 160 / 320 / 512 poses against 38 / 48 / 57 for PCG).
// Block-Jacobi block size in poses (tools/ba_pc_sweep.py, 1 200 keyframes, 10 LM iterations): 1 / 8 / 16 / 32 / 64 poses per block need
// 5 891 / 4 329 / 3 283 / 2 538 / 1 889 CG iterations; the batched potrf + potri of the blocks costs 0.4 / 1.1 / 2.9 ms at 16 / 32 / 64 and is paid on
// every 3rd trial only (ba_lm_device): 79 ms with 6x6 blocks, 54 / 51.7 / 56 ms with 16 / 32 / 64.  Below ~500 poses the setup is not repaid.
// From 4096 poses on (measured at 10 000 and 50 000) the SpMV is HBM-bound, the bytes of the larger blocks count and a stale inverse costs 30-40 % more
// iterations: 16-pose blocks refreshed on every trial are faster there (176 vs 216 ms per 5 LM iterations at 50 000 keyframes).
// Late in round 4 (blocks inverted in registers: a set-up is 0.1 ms at these sizes; the coarse levels on): 280 / 400 / 600 keyframes per 10 LM iterations with 6 x 6
// blocks 36.8 / 44.9 / - ms, 16-keyframe blocks 20.0 / 23.4 / 26.7, 16-keyframe blocks + coarse levels 12.4 / 11.9 / 14.0 (tools/ml_small.py): 16 from 128 poses on.
int ba_choose(const CorbBAOptions* opt, int nP, int nE, int nL, BAChoice& ch)
{
    int solver = opt ? opt->solver : 0;
    if (solver < 0 || solver > 2) { corb_set_error("corb_ba_solve: bad solver option"); return CORB_ERR_ARG; }
    if (solver == 0) solver = nP <= 256 ? 1 : 2;
    ch.pcg_forcing = !(opt && opt->pcg_tol > 0) && nP > BA_PCG_FORCING_MIN_POSES; ch.pcg_tol = (opt && opt->pcg_tol > 0) ? opt->pcg_tol : BA_PCG_TOL_TIGHT;     // no tolerance given: the default policy
    ch.pcg_max_iter = (opt && opt->pcg_max_iter > 0) ? opt->pcg_max_iter : 4000;
    int pc_g = (opt && opt->pc_block > 0) ? opt->pc_block : (nP >= 128 ? 16 : 1);
    if (pc_g > 1 && pc_g != 8 && pc_g != 16) { corb_set_error("corb_ba_solve: pc_block must be 1, 8 or 16"); return CORB_ERR_ARG; }
    if (solver != 2) pc_g = 1;
    const int sp = 6 * nP;
    if (solver == 1 && (double)sp * sp * 8.0 > 96e9) { corb_set_error("corb_ba_solve: %d free poses need a %.1f GB dense reduced system; use the PCG solver", nP, (double)sp * sp * 8e-9); return CORB_ERR_ARG; }
    ch.solver = solver; ch.pc_g = pc_g;
    ch.multilevel = solver == 2 && pc_g == BA_ML_G && (opt && opt->pc_multilevel ? opt->pc_multilevel == 2 : nP >= BA_ML_AUTO_POSES);
    static const int small_edges = corb_dev_env("CORB_BA_SMALL_EDGES") ? atoi(corb_dev_env("CORB_BA_SMALL_EDGES")) : BA_SMALL_EDGES;     // (env: development aid)
    ch.fused_small = solver == 1 && sp <= BA_SMALL_SP && nE <= small_edges && nL <= small_edges && (opt == nullptr || opt->solver != 1);
    ch.want_pattern = solver == 2 || !ch.fused_small;      // (the one-workgroup optimiser needs no block pattern)
    return CORB_OK;
}

// optimizer.initializeOptimization(0) + optimize(iterations) over the edges with active[i] != 0 (NULL = all), from and to
// the double-precision state.  last_chi2 (orig-indexed, optional) receives chi2 of every computeError() on an active edge.
// sess (optional, not ready): the graph stays on the device for the later optimize() calls of a staged solve.
int ba_optimize_device(const CorbBAProblem* p, const uint8_t* active, BAState& st, int iterations, int robust, volatile int* stop_flag,
                       CorbBAResult* r, const CorbBAOptions* opt, std::vector<double>* last_chi2,
                       std::vector<uint8_t>* pose_touched, std::vector<uint8_t>* pt_touched, double delta2, double delta3, BASession* sess)
{
    Lap lap;
    BAChoice ch; BAHostFlat* flat = nullptr;
    int rc = ba_flatten_host(p, active, opt, pose_touched, pt_touched, lap, ch, &flat); if (rc) return rc;
    const BAHostFlat& h = *flat; const int nE = h.nE;
    r->solver_used = ch.solver; r->free_poses = h.nP; r->free_points = h.nL; r->pc_block = ch.solver == 2 ? ch.pc_g : 0;
    r->active_edges = nE; r->nnz_blocks = h.nnzb; r->schur_pairs = 0;
    // ---- device state ----
    std::unique_ptr<Pool> own_pool;
    if (sess) sess->pool.reset(new Pool()); else own_pool.reset(new Pool());
    Pool& pool = sess ? *sess->pool : *own_pool;
    if (!pool.stream) { corb_set_error("BA workspace: stream creation failed"); return CORB_ERR_HIP; }
    hipStream_t s = pool.stream;
    BAFlat f;
    rc = ba_upload_flat(pool, h, st, ch, f); if (rc) return rc;
    const size_t n_state = f.n_state();
    lap("uploads");
    double* d_e_chi2 = nullptr;
    bool sess_ok = false;                                  // the graph stays on the device for the later optimize() calls of this staged solve
    if (sess && !ch.fused_small && nE == p->n_edges) {
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
        sess->f = f; sess->ch = ch; sess->act = h.act; sess->covers_all = true; sess->ready = true; sess->dev = true; sess->cur_set = 0; sess->d_e_chi2 = d_e_chi2;
        return CORB_OK;
    }
    if (n_state * 8 <= ((size_t)4 << 20)) {              // small state: one copy of the whole block, split on the host
        static thread_local std::vector<double> back;
        back.resize(n_state ? n_state : 1);
        if (n_state) HIPCHK(hipMemcpyAsync(back.data(), f.dq, n_state * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ba_state_unpack(back.data(), st);
    } else {
        HIPCHK(hipMemcpyAsync(st.q.data(), f.dq, f.n_q * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(st.t.data(), f.dq + f.n_q, f.n_t * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(st.pt.data(), f.dq + f.n_q + f.n_t, f.n_pt * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    if (last_chi2 && nE > 0) {
        std::vector<double> ec(nE);
        HIPCHK(pool.d2h(ec.data(), d_e_chi2, sizeof(double) * (size_t)nE)); HIPCHK(pool.fetch_finish());
        for (int j = 0; j < nE; j++) (*last_chi2)[h.act[j]] = ec[j];
    }
    lap("read back");
    if (sess_ok) { sess->f = f; sess->ch = ch; sess->act = h.act; sess->e_w0 = h.e_w; sess->covers_all = true; sess->ready = true; }
    if (sess && !sess->ready) sess->pool.reset();            // (no session after all: the lane's workspace must be free for the next call)
    return CORB_OK;
}

// ---- problems whose arrays live in device memory (corb_ba_store.cpp) ----
int corb_ba_solve_device(const CorbBADeviceProblem* dp, int iterations, int robust, volatile int* stop_flag, CorbBAResult* r, int device, const CorbBAOptions* opt)
{
    if (!dp || !r || dp->n_poses < 0 || dp->n_points < 0 || dp->n_edges < 0 || iterations < 0) { corb_set_error("corb_ba_solve_device: bad argument"); return CORB_ERR_ARG; }
    int rc = corb_select_device(device); if (rc) return rc;
    ba_result_reset(r);
    Lap lap;
    const int K = dp->n_poses, M = dp->n_points;
    Pool pool;
    if (!pool.stream) { corb_set_error("BA workspace: stream creation failed"); return CORB_ERR_HIP; }
    hipStream_t s = pool.stream;
    // 1. active edges per point; hessian indices; edge offsets
    BAFlattenDev d; int* scan_tmp;
    rc = ba_flat_dev_begin(d, dp, pool, &scan_tmp); if (rc) return rc;
    ba_flat_dev_scans(d, scan_tmp, s);
    HIPCHK(hipGetLastError());
    int* h = static_cast<int*>(pool.pinned());
    HIPCHK(hipMemcpyAsync(h + 0, d.lidx + M, 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(h + 1, d.eoffA + M, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h + 2, d.eoffB + M, 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(h + 3, d.pidx + K, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    BAFlat f; ba_flat_dev_counts(f, h);
    const int nE = f.nE, nP = f.nP, nL = f.nL;
    if (h[1] < 0 || h[2] < 0 || nE < 0) { corb_set_error("corb_ba_solve_device: more than 2^31 observations"); return CORB_ERR_ARG; }
    BAChoice ch; rc = ba_choose(opt, nP, nE, nL, ch); if (rc) return rc;
    r->solver_used = ch.solver; r->free_poses = nP; r->free_points = nL; r->pc_block = ch.solver == 2 ? ch.pc_g : 0; r->active_edges = nE;
    lap("device: counts");
    // 2. the sorted structure-of-arrays edges, landmark ranges, estimates
    rc = ba_flat_dev_alloc(d, f, pool, false); if (rc) return rc;
    HIPCHK(pool.alloc(&d.pcnt, (size_t)nP + 1)); HIPCHK(pool.alloc(&d.pcur, (size_t)nP + 1));
    HIPCHK(hipMemsetAsync(d.pcnt, 0, sizeof(int) * ((size_t)nP + 1), s)); HIPCHK(hipMemsetAsync(d.pcur, 0, sizeof(int) * ((size_t)nP + 1), s));
    rc = ba_flat_dev_wire(d, f, pool); if (rc) return rc;
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
    const bool want_pattern = f.have_pattern = ch.want_pattern;
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

// ---- large maps handed over as HOST arrays (round 5) ----
// OptimizerT::BundleAdjustment (host/corb_adapter_orbslam.hpp; Optimizer.cc:150-210) builds its edges map point by map point, so a caller's edge array arrives grouped
// by point -- which is the order corb_ba_solve_device wants.  Such a problem does not need the host flattening (sort, lists, pattern: ~95 ms of threads at 27.5 M
// observations) and its 1.1 GB of flattened uploads: the RAW arrays travel through a page-locked double buffer filled by worker threads (which check the edges' index ranges
// and their grouping on the way: the serial validate() pass over 27.5 M edges is gone too), and the graph is flattened on the device like corb_ba_solve_store's.  The estimates
// of both paths are equal element for element (tests/test_gpu_ba.py::test_device_flattening_equals_host_flattening); wall time of the call at 50 000 keyframes 0.38 -> 0.2x s.
#define BA_HOST_FAST_MIN_EDGES (1 << 20)
#define BA_HOST_FAST_MIN_POSES 257          // the PCG solver's range (auto choice): smaller problems keep the host path and its session / staging features
struct HostFastBuf {                         // per device: grown by the calls, given back by corb_release_scratch; one call at a time per device
    std::mutex mu; int device = -1;
    OwnedStream stream; OwnedEvent ev[2];
    DevMem dev; PinnedMem pin[2];
    size_t release() {                       // (the caller holds mu and has selected the device)
        size_t freed = dev.cap() + pin[0].cap() + pin[1].cap();
        if (stream) (void)hipStreamSynchronize(stream);
        stream.reset();
        for (int i = 0; i < 2; i++) { ev[i].reset(); pin[i].reset(); }
        dev.reset(); device = -1;
        return freed;
    }
};
// (never deleted: the buffers go with corb_release_scratch or with the process, not with static destructors that would run after the HIP runtime's)
static HostFastBuf& hostfast(int device) { static HostFastBuf* const b = new HostFastBuf[64]; return b[device < 0 || device >= 64 ? 0 : device]; }
size_t ba_host_fast_release(int device)
{
    HostFastBuf& B = hostfast(device);
    std::unique_lock<std::mutex> lk(B.mu, std::try_to_lock);
    return lk.owns_lock() ? B.release() : 0;
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
    if (B.device != device || B.dev.cap() < total || !B.pin[0] || !B.stream) {
        B.dev.reset();
        if (B.dev.room(total + (total >> 3)) != hipSuccess) { (void)hipGetLastError(); return CORB_OK; }      // no room: the host path
        B.device = device;
        for (int i = 0; i < 2; i++) if (B.pin[i].room(CH) != hipSuccess) { (void)hipGetLastError(); return CORB_OK; }
        if (!B.stream && B.stream.create() != hipSuccess) return CORB_ERR_HIP;
        for (int i = 0; i < 2; i++) if (!B.ev[i] && B.ev[i].create(hipEventDisableTiming) != hipSuccess) return CORB_ERR_HIP;
    }
    char* const dev = B.dev.as<char>(); char* const pin[2] = {B.pin[0].as<char>(), B.pin[1].as<char>()};
    // the small arrays, then the edges in chunks: worker threads copy a chunk into a page-locked buffer (checking it), the DMA of the previous chunk runs meanwhile
    std::vector<float> intr(5 * K + 1);
    for (size_t k = 0; k < K; k++) ba_intrinsics(p, (int)k, &intr[5 * k]);
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
            char* dst = pin[cur]; const char* src = pc.src + done;
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
            HIPCHK(hipMemcpyAsync(dev + pc.off + done, dst, nb, hipMemcpyHostToDevice, B.stream));
            HIPCHK(hipEventRecord(B.ev[cur], B.stream)); used[cur] = true; cur ^= 1;
        }
        if (bad.load()) break;
    }
    if (bad.load() == 1) { HIPCHK(hipStreamSynchronize(B.stream)); corb_set_error("corb_ba_solve: an edge's pose / point index is out of range"); *taken = true; return CORB_ERR_ARG; }
    if (bad.load() == 2) { HIPCHK(hipStreamSynchronize(B.stream)); return CORB_OK; }              // edges not grouped by point: the host path sorts them
    CorbBADeviceProblem dp; memset(&dp, 0, sizeof(dp));
    dp.n_poses = (int)K; dp.n_points = (int)M; dp.n_edges = (int)E;
    dp.poses = (float*)(dev + o_poses); dp.pose_fixed = (const uint8_t*)(dev + o_pf); dp.points = (float*)(dev + o_pts); dp.point_fixed = (const uint8_t*)(dev + o_xf);
    dp.intr = (const float*)(dev + o_intr); dp.edges = (const CorbBAEdge*)(dev + o_edges); dp.edge_off = (const int*)(dev + o_off);
    ba_launch_edge_offsets(dp.edges, (int)E, (int)M, (int*)(dev + o_off), B.stream);
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
                HIPCHK(hipMemcpyAsync(pin[ci], dev + o.off + issued, nb, hipMemcpyDeviceToHost, B.stream));
                HIPCHK(hipEventRecord(B.ev[ci], B.stream)); len[ci] = nb; issued += nb; ci ^= 1;
            }
            HIPCHK(hipEventSynchronize(B.ev[cc]));
            memcpy(o.dst + copied, pin[cc], len[cc]); copied += len[cc]; cc ^= 1;
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
    int rc = ba_validate(p, r); if (rc) return rc;
    if (iterations < 0) { corb_set_error("corb_ba_solve: negative iteration count"); return CORB_ERR_ARG; }
    rc = corb_select_device(device); if (rc) return rc;
    ba_result_reset(r);
    BAState st; ba_state_from_floats(p, st);
    std::vector<uint8_t> pose_touched(p->n_poses ? p->n_poses : 1, 0), pt_touched(p->n_points ? p->n_points : 1, 0);
    rc = ba_optimize_device(p, nullptr, st, iterations, robust, stop_flag, r, opt, nullptr, &pose_touched, &pt_touched,
                            (double)(float)std::sqrt(5.99), (double)(float)std::sqrt(7.815));   // thHuber2D/3D are floats (Optimizer.cc:102-103)
    if (rc) return rc;
    for (auto& v : pose_touched) v = 1;                         // GlobalBundleAdjustemnt writes every non-fixed keyframe back (Optimizer.cc:216-237)
    ba_state_to_floats(p, st, pose_touched, pt_touched, r);
    return CORB_OK;
}

extern "C" int corb_ba_solve(const CorbBAProblem* p, int iterations, int robust, volatile int* stop_flag, CorbBAResult* r, int device)
{
    return corb_ba_solve_ex(p, iterations, robust, stop_flag, r, device, nullptr);
}

// the device flattening against the host flattening (tests): flattens a problem given in HOST memory on the device path -- upload, group by point, solve, download
extern "C" int corb_ba_solve_devflat(const CorbBAProblem* p, int iterations, int robust, CorbBAResult* r, int device, const CorbBAOptions* opt)
{
    int rc = ba_validate(p, r); if (rc) return rc;
    rc = corb_select_device(device); if (rc) return rc;
    const size_t K = (size_t)p->n_poses, M = (size_t)p->n_points, E = (size_t)p->n_edges;
    // group the edges by point (stable), as corb_ba_solve_store's records deliver them
    std::vector<int> off(M + 1, 0); std::vector<CorbBAEdge> ge(E + 1);
    for (size_t i = 0; i < E; i++) off[(size_t)p->edges[i].point + 1]++;
    for (size_t m = 0; m < M; m++) off[m + 1] += off[m];
    { std::vector<int> cur(off.begin(), off.end() - 1); for (size_t i = 0; i < E; i++) ge[(size_t)cur[(size_t)p->edges[i].point]++] = p->edges[i]; }
    std::vector<float> intr(5 * K + 1);
    for (size_t k = 0; k < K; k++) ba_intrinsics(p, (int)k, &intr[5 * k]);
    DevList dev_mem; auto dev_get = [&](size_t bytes) -> void* { char* q = nullptr; return dev_mem.add(&q, bytes) == hipSuccess ? q : nullptr; };
    CorbBADeviceProblem dp; memset(&dp, 0, sizeof(dp));
    dp.n_poses = (int)K; dp.n_points = (int)M; dp.n_edges = (int)E;
    dp.poses = (float*)dev_get(64 * K); uint8_t* dpf = (uint8_t*)dev_get(K); dp.points = (float*)dev_get(12 * M); uint8_t* dxf = (uint8_t*)dev_get(M);
    CorbBAEdge* de = (CorbBAEdge*)dev_get(sizeof(CorbBAEdge) * E); float* di = (float*)dev_get(20 * K); int* doff = (int*)dev_get(4 * (M + 1));
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

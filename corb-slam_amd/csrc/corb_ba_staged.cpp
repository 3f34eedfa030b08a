// corb_ba_staged.cpp -- Optimizer::LocalBundleAdjustment / PoseOptimization style multi-stage optimisation (corb_ba_solve_staged, see include/corb_accel.h):
// the session that keeps the first optimize()'s graph on the device, and the two window routes that flatten on the device.
#include "ba_host.h"
#include "pose_internal.h"
#include <algorithm>

// fresh e->computeError() / isDepthPositive() of EVERY edge at the given estimates (classification between stages)
static int ba_eval_edges_device(const CorbBAProblem* p, const std::vector<double>& q, const std::vector<double>& t, const std::vector<double>& pt,
                         std::vector<double>& chi2, std::vector<double>& depth)
{
    const int E = p->n_edges;
    chi2.assign(E ? E : 1, 0.0); depth.assign(E ? E : 1, 0.0);
    if (E == 0) return CORB_OK;
    std::vector<int> vp(E), vx(E); std::vector<double> obs(3 * (size_t)E), w(E); std::vector<unsigned char> dim(E);
    for (int i = 0; i < E; i++) { const CorbBAEdge& e = p->edges[i]; vp[i] = e.pose; vx[i] = e.point; dim[i] = e.u_right < 0 ? 2 : 3;
                                  obs[3 * (size_t)i] = e.u; obs[3 * (size_t)i + 1] = e.v; obs[3 * (size_t)i + 2] = e.u_right; w[i] = e.inv_sigma2; }
    Pool pool;
    std::vector<double> cam; ba_cam_table(p, cam);
    int *dvp, *dvx; double *dobs, *dw, *dq, *dt, *dpt, *dchi, *ddep, *dcam; unsigned char* ddim;
    // one staging block in, one block (chi2 | depth) out: for a local window the eight separate copies cost more than the evaluation
    HIPCHK(pool.upload_block({{(void**)&dvp, vp.data(), vp.size() * 4}, {(void**)&dvx, vx.data(), vx.size() * 4}, {(void**)&dobs, obs.data(), obs.size() * 8}, {(void**)&dw, w.data(), w.size() * 8},
                              {(void**)&ddim, dim.data(), dim.size()}, {(void**)&dq, q.data(), q.size() * 8}, {(void**)&dt, t.data(), t.size() * 8}, {(void**)&dpt, pt.data(), pt.size() * 8},
                              {(void**)&dcam, cam.data(), cam.size() * 8}}));
    HIPCHK(pool.alloc(&dchi, (size_t)2 * E)); ddep = dchi + E;
    ba_launch_edge_eval(ba_edge_view(E, dvp, dvx, dobs, dw, ddim, dq, dt, dpt, dcam), dchi, ddep, pool.stream);
    HIPCHK(hipGetLastError());
    HIPCHK(pool.d2h(chi2.data(), dchi, sizeof(double) * (size_t)E)); HIPCHK(pool.d2h(depth.data(), ddep, sizeof(double) * (size_t)E));
    HIPCHK(pool.fetch_finish());
    return CORB_OK;
}
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
    CorbBADev d = ba_edge_view(f, S.d_w0); d.e_chi2 = S.d_e_chi2;
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
    const size_t n_state = f.n_state();
    static thread_local std::vector<double> blob;
    blob.resize((size_t)nE + n_state + 1);
    int n_active = 0;
    for (int j = 0; j < nE; j++) {
        const int i = S.act[j]; const bool on = !active || active[i];
        blob[j] = on ? S.e_w0[j] : 0.0;
        if (on) { n_active++; const CorbBAEdge& e = p->edges[i]; if (pose_touched) (*pose_touched)[e.pose] = 1; if (pt_touched) (*pt_touched)[e.point] = 1; }
    }
    double* stp = blob.data() + nE;
    ba_state_pack(st, stp);
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
    ba_state_unpack(back.data(), st);
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
    ba_launch_edge_eval(ba_edge_view(f, dw0), dchi, ddep, pool.stream);
    HIPCHK(hipGetLastError());
    std::vector<double> both((size_t)2 * f.nE);
    HIPCHK(pool.d2h(both.data(), dchi, sizeof(double) * (size_t)2 * f.nE));
    HIPCHK(pool.fetch_finish());
    for (int j = 0; j < f.nE; j++) { chi2[S.act[j]] = both[j]; depth[S.act[j]] = both[(size_t)f.nE + j]; }
    return CORB_OK;
}

// one free pose, every edge attached to it, every referenced point fixed, <= 8 stages, no stop flag raised
static int single_pose_problem(const CorbBAProblem* p, int n_stages)
{
    if (n_stages > CORB_POSE_MAX_STAGES) return -1;
    int freep = -1;
    for (int k = 0; k < p->n_poses; k++) if (!p->pose_fixed[k]) { if (freep >= 0) return -1; freep = k; }
    if (freep < 0) return -1;
    for (int i = 0; i < p->n_edges; i++) if (p->edges[i].pose != freep || !p->point_fixed[p->edges[i].point]) return -1;
    return freep;
}

bool corb_ba_staged_device_wanted(const CorbBAStage* stages, int n_stages)
{
    static const bool host_route = getenv("CORB_LBA_HOST_FLATTEN") != nullptr;      // (the round-4 route -- problem to the host, host flattening --: for A/B timing)
    if (host_route) BA_TRACE("window: host flattening (CORB_LBA_HOST_FLATTEN)");
    if (host_route || n_stages < 1 || n_stages > FLAT_MAX_STAGES) return false;     // (flat_launch_fixed_edge_outliers replays every stage that ran)
    for (int s = 1; s < n_stages; s++) if (stages[s].reset_estimates) return false;
    return true;
}
static int ba_staged_window(BASession& sess, const CorbBADeviceProblem* dp, const CorbBAStage* stages, int n_stages, volatile int* stop_flag, CorbBAResult* r, uint8_t* d_outlier,
                            const int* d_status, int* n_edges_out, int* status_out, const CorbBAOptions* opt, int* applicable)
{
    const int K = dp->n_poses, M = dp->n_points;
    int rc = CORB_OK;
    Lap lap;
    Pool& pool = *sess.pool;
    hipStream_t s = pool.stream;
    // 1. active edges per point; hessian indices; edge offsets -- and the one read-back of the flattening: the counts
    BAFlattenDev d; int* scan_tmp;
    rc = ba_flat_dev_begin(d, dp, pool, &scan_tmp); if (rc) return rc;
    {
        const int* in4[4] = {d.lflag, d.cntA, d.cntB, d.pflag}; int* out4[4] = {d.lidx, d.eoffA, d.eoffB, d.pidx}; const size_t n4[4] = {(size_t)M, (size_t)M, (size_t)M, (size_t)K};
        if (!corb_launch_exclusive_scan4(in4, out4, n4, 4, s)) ba_flat_dev_scans(d, scan_tmp, s);
    }
    HIPCHK(hipGetLastError());
    int* h = static_cast<int*>(pool.pinned());
    int* d_counts; HIPCHK(pool.alloc(&d_counts, 8));
    flat_launch_counts(d, d_status, d_counts, s);
    HIPCHK(hipMemcpyAsync(h, d_counts, 8 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    BAFlat f; ba_flat_dev_counts(f, h);
    const int nE = f.nE, nP = f.nP, nL = f.nL; const int pairs_sum = h[4];
    const int n_edges = h[5];
    *n_edges_out = n_edges; *status_out = h[6];
    if (h[6] != 0 || n_edges <= 0 || (dp->n_edges >= 0 && dp->n_edges != n_edges) || (stop_flag && *stop_flag)) return CORB_OK;      // (the caller looks at the status word; declined: nothing was touched)
    if (h[1] < 0 || h[2] < 0 || nE <= 0 || nP <= 0 || nL <= 0 || nP > 64 || pairs_sum < 0 || pairs_sum > (1 << 22)) return CORB_OK;
    BAChoice ch; rc = ba_choose(opt, nP, nE, nL, ch); if (rc) return rc;
    if (ch.solver != 1 || ch.fused_small) return CORB_OK;
    *applicable = 1;
    BA_TRACE("window: device flattening");
    { const int nnzb = r->nnz_blocks; ba_result_reset(r); r->nnz_blocks = nnzb; }      // (left as it is until the pattern below is laid out)
    r->solver_used = ch.solver; r->free_poses = nP; r->free_points = nL; r->pc_block = 0; r->active_edges = nE; r->reserved0 = 1;      // (the device route ran)
    double* chi_hist = r->chi2; double* lam_hist = r->lambda; r->chi2 = nullptr; r->lambda = nullptr;     // histories are per optimize() call
    struct Hist { CorbBAResult* r; double* c; double* l; ~Hist() { r->chi2 = c; r->lambda = l; } } hist_back{r, chi_hist, lam_hist};
    lap("window: counts");
    // 2. the sorted structure-of-arrays edges, landmark ranges, estimates; per-keyframe lists (their total is at most nE, the longest at most max_list)
    rc = ba_flat_dev_alloc(d, f, pool, true); if (rc) return rc;
    HIPCHK(pool.alloc(&d.pcnt, 2 * ((size_t)nP + 1))); d.pcur = d.pcnt + nP + 1;
    HIPCHK(hipMemsetAsync(d.pcnt, 0, sizeof(int) * 2 * ((size_t)nP + 1), s));
    rc = ba_flat_dev_wire(d, f, pool); if (rc) return rc;
    flat_launch_state_in(d, s);
    flat_launch_edges(d, s, nP);
    corb_launch_exclusive_scan(d.pcnt, f.poff, (size_t)nP, scan_tmp, s);
    HIPCHK(pool.alloc(&f.pedge, (size_t)nE)); HIPCHK(pool.alloc(&f.plm, (size_t)nE));
    d.pedge = f.pedge; d.plm = f.plm;
    flat_launch_pose_lists_ordered(d, nP, nE, s);          // (a workgroup per keyframe compacts its edges in order: the global path's atomics + sort took 75 us of a window's call)
    // 3. the full block pattern (the reduced system is dense: a block without a shared landmark has an empty pair list and stays zero)
    f.have_pattern = true;                               // (ch.want_pattern: a dense solve outside the one-workgroup optimiser always has one)
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
    for (int k = 0; k < K; k++) ba_intrinsics(p, k, &intr[5 * (size_t)k]);
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

// Optimizer::LocalBundleAdjustment / PoseOptimization style multi-stage optimisation (see include/corb_accel.h)
extern "C" int corb_ba_solve_staged(const CorbBAProblem* p, const CorbBAStage* stages, int n_stages, volatile int* stop_flag,
                                    CorbBAResult* r, uint8_t* edge_outlier, int device, const CorbBAOptions* opt)
{
    int rc = ba_validate(p, r); if (rc) return rc;
    if (!stages || n_stages < 1) { corb_set_error("corb_ba_solve_staged: no stages"); return CORB_ERR_ARG; }
    rc = corb_select_device(device); if (rc) return rc;
    ba_result_reset(r);
    double* chi_hist = r->chi2; double* lam_hist = r->lambda; r->chi2 = nullptr; r->lambda = nullptr;     // histories are per optimize() call
    const int E = p->n_edges;
    const int solver_opt = opt ? opt->solver : 0;
    const int freep = (solver_opt == 0 || solver_opt == 3) && !(stop_flag && *stop_flag) ? single_pose_problem(p, n_stages) : -1;
    if (freep >= 0) {                     // one free pose, fixed points: the whole staged optimisation is one kernel
        PoseBatch b;
        double p7[7]; corb_pose_from_T(p->poses + 16 * (size_t)freep, p7);
        b.pose.assign(p7, p7 + 7);
        std::vector<double> camt; ba_cam_table(p, camt);
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
        if (cnt[2]) corb_pose_to_T(pose.data(), r->poses + 16 * (size_t)freep);
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
    BAState st; ba_state_from_floats(p, st);
    const BAState st0 = st;
    std::vector<uint8_t> active(E ? E : 1, 1), pose_touched(p->n_poses ? p->n_poses : 1, 0), pt_touched(p->n_points ? p->n_points : 1, 0);
    std::vector<double> last(E ? E : 1, 0.0), fresh, depth;
    BASession sess;                                        // the first optimize() leaves its graph on the device for the later ones
    {
        bool resets = false; for (int s = 1; s < n_stages; s++) resets = resets || stages[s].reset_estimates != 0;
        static const bool host_stages = getenv("CORB_BA_HOST_STAGES") != nullptr;      // (the classifications on the host, as before round 5: for A/B timing)
        sess.want_dev = n_stages > 1 && !resets && !host_stages; sess.n_sets = n_stages + 1;
        if (n_stages > 1 && !resets) BA_TRACE(host_stages ? "stages: classified on the host (CORB_BA_HOST_STAGES)" : "stages: classified on the device");
    }
    int n_opt = 0;                                         // optimize() calls done
    for (int s = 0; s < n_stages; s++) {
        if (stages[s].reset_estimates) st = st0;
        if (sess.ready && sess.dev) rc = ba_optimize_session_dev(sess, stages[s].iterations, stages[s].robust, stop_flag, r, (double)stages[s].huber_mono, (double)stages[s].huber_stereo);
        else if (sess.ready) rc = ba_optimize_session(p, active.data(), st, stages[s].iterations, stages[s].robust, stop_flag, r, sess, &last, &pose_touched, &pt_touched,
                                                      (double)stages[s].huber_mono, (double)stages[s].huber_stereo);
        else
        rc = ba_optimize_device(p, active.data(), st, stages[s].iterations, stages[s].robust, stop_flag, r, opt, &last, &pose_touched, &pt_touched,
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
        const size_t n_state = f.n_state(); const int nE = f.nE, n_sets = sess.cur_set + 1;
        static thread_local std::vector<double> back; static thread_local std::vector<uint8_t> sets;
        back.resize(n_state ? n_state : 1); sets.resize((size_t)n_sets * (nE ? nE : 1));
        if (n_state) HIPCHK(pool.d2h(back.data(), f.dq, n_state * 8));
        if (nE && n_sets > 1) HIPCHK(pool.d2h(sets.data() + nE, sess.d_act + nE, (size_t)(n_sets - 1) * nE));
        if (nE) memset(sets.data(), 1, (size_t)nE);
        HIPCHK(pool.fetch_finish());
        ba_state_unpack(back.data(), st);
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
    ba_state_to_floats(p, st, pose_touched, pt_touched, r);
    return CORB_OK;
}

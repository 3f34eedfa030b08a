// ba_lm.cpp -- the Levenberg-Marquardt driver of every bundle-adjustment route (G/core/optimization_algorithm_levenberg.cpp:61-164).  All per-edge / per-vertex
// arithmetic runs in ba_kernels.hip; the dense reduced camera system is factorised by the hand-written blocked Cholesky of dense_chol.hip.  The host only
// sequences launches and reads back 3 scalars per trial.
#include "ba_host.h"
#include "dense_chol.h"
#include <algorithm>
#include <cfloat>

// optimizer.optimize(iterations) on a flattened graph: allocates the work arrays from the lane's arena, runs g2o's Levenberg-Marquardt control
// (G/core/optimization_algorithm_levenberg.cpp:61-164) and leaves the estimates in f.dq.  *e_chi2_out (optional) = chi2 of every edge's last computeError().
int ba_lm_device(Pool& pool, BAFlat& f, const BAChoice& ch, int iterations, int robust, volatile int* stop_flag, CorbBAResult* r, double delta2, double delta3,
                 Lap& lap, double** e_chi2_out, LMWork* work)
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
    const size_t n_state = f.n_state();
    double* dq = f.dq; double* dq_bak = f.dq_bak;
    // per-workgroup partial sums of the chi2 / scale reductions: small problems use ONE workgroup, which writes the result directly
    const int nparts = std::max(1, std::min(256, (std::max(nE, sp + 3 * nL) + 1023) / 1024));
    const int n_upd_blocks = (std::max(nP, nL) + 255) / 256;
    if (reuse) {
        d = work->d; d_partial = work->d_partial; d_scal = work->d_scal; d_bad = reinterpret_cast<int*>(d_scal + 6); d_info = d_bad + 1;
        HIPCHK(hipMemsetAsync(d_bad, 0, 2 * sizeof(int), s));
    } else {
    d = ba_edge_view(f, f.e_w); d.nP = nP; d.nL = nL; d.sp = sp;
    // scalars [0..5] and the two status words (as the 7th double) are one block: one read-back per trial
    // (the reductions' ticket lives behind them, so that one fill clears it and the status words)
    HIPCHK(pool.alloc(&d_partial, (size_t)std::max(nparts, n_upd_blocks <= BA_FUSED_UPDATE_BLOCKS ? n_upd_blocks : 1))); HIPCHK(pool.alloc(&d_scal, 16)); d_bad = reinterpret_cast<int*>(d_scal + 6); d_info = d_bad + 1;
    d.red_tick = reinterpret_cast<int*>(d_scal + 8);
    HIPCHK(hipMemsetAsync(d_bad, 0, 3 * sizeof(double), s));      // (d_bad holds the number of the trial that failed: never cleared again)
    d.e_pose = f.e_pose; d.e_point = f.e_point; d.loff = f.loff; d.lnfree = f.lnfree; d.poff = f.poff; d.pedge = f.pedge; d.pose_vertex = f.pose_vertex; d.point_vertex = f.point_vertex;
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
            BA_TRACE(v_edge ? "V blocks: edge order (CORB_BA_V_EDGE / CORB_BA_ROW_UNITS)" : "V blocks: keyframe-list order");
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
            BA_TRACE(row_per_unit ? "row schur: per-unit kernel (CORB_BA_ROW_UNITS)" : "row schur: stream kernel");
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
            BA_TRACE(pc_square ? "pc step: square blocks (CORB_BA_PC_SQUARE)" : "pc step: packed upper triangles");
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
    BA_TRACE(no_graph ? "cg chunk: kernel by kernel (CORB_BA_NO_GRAPH)" : "cg chunk: graph replay");
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
    const bool chain_able = solver == 1 && small_solve && fused_update && d.lean && !phase_ev && sp > 0;
    const bool chain_ok = chain_able && !no_chain;
    if (chain_able && !chain_ok) BA_TRACE("lm: host-driven loop (CORB_BA_NO_CHAIN)");
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
            BA_TRACEF("lm: device-decided chain of up to %d iterations", chain_len);
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
                if (j == 0) BA_TRACE(ctl_launch ? "lm ctl: its own launch (CORB_BA_CTL_LAUNCH)" : "lm ctl: in the chi2 launch");
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

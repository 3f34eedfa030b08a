// ba_flatten_host.cpp -- graph flattening of a CorbBAProblem on the host, and its upload.  Follows Optimizer::BundleAdjustment (corbslam_client/src/Optimizer.cc:54-270)
// and the g2o index mapping (free poses, then free landmarks, ascending id; G/core/sparse_optimizer.cpp:166-190).
#include "ba_host.h"
#include <algorithm>

// worker threads of the host-side graph flattening for n observations: 8 / 16 / 32 from ~2 / 4 / 16 M on (27.5 M observations: 0.45 s serial of a 1.3 s call), 4 from
// ~260 k on (660 k observations: 12.5 ms serial beside 40 ms of device time); local windows stay serial.  CORB_BA_HOST_THREADS=n forces a count
// (tests: the threaded paths produce the serial paths' lists, element for element).
int ba_host_threads(size_t n, bool sort_stage)
{
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    if (const char* f = getenv("CORB_BA_HOST_THREADS")) { const int v = atoi(f); if (v > 0) return (int)std::min((unsigned)v, std::max(hw, 2u)); }
    // (the filter + two-level sort only pay from ~2 M observations: 2.5 ms serial, 4.2 ms on 4 threads at 660 k)
    // (27.5 M observations: 163 / 105 / 75 ms of flattening on 8 / 16 / 32 threads)
    return (int)std::min(hw, n >= ((size_t)1 << 24) ? 32u : n >= ((size_t)1 << 22) ? 16u : n >= ((size_t)1 << 21) ? 8u : (n >= ((size_t)1 << 18) && !sort_stage) ? 4u : 1u);
}

// optimizer.initializeOptimization(0) of the edges with active[i] != 0 (NULL = all): the active edges in the solver's order, the index mapping, the per-landmark and
// per-keyframe lists, the block pattern of the reduced camera system -- and, once the sizes are known, the route (ba_choose).  *out: this thread's arrays.
int ba_flatten_host(const CorbBAProblem* p, const uint8_t* active, const CorbBAOptions* opt, std::vector<uint8_t>* pose_touched, std::vector<uint8_t>* pt_touched,
                    Lap& lap, BAChoice& ch, BAHostFlat** out)
{
    const int K = p->n_poses, M = p->n_points;
    // host staging vectors live per thread and keep their capacity: at 16 M observations most of the flattening time was first-touch page
    // faults of freshly allocated vectors (every element below is (re)written on every call)
    static thread_local BAHostFlat hs;
    *out = &hs;
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
    const int nP = hs.nP = (int)pose_vertex.size(), nL = hs.nL = (int)point_vertex.size();
    { const int rc = ba_choose(opt, nP, (int)act.size(), nL, ch); if (rc) return rc; }
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
    const int nE = hs.nE = (int)act.size();
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
    // block-sparse pattern of the reduced camera system: pose pairs that share a landmark (block_solver.hpp:262-292)
    std::vector<int>& bsr_rowptr = hs.bsr_rowptr; std::vector<int>& bsr_col = hs.bsr_col; std::vector<int>& bsr_diag = hs.bsr_diag;
    std::vector<int>& uinfo = hs.uinfo; uinfo.clear();        // (slot, p, q, -) of every block on / above the diagonal
    bsr_rowptr.assign(nP + 1, 0); bsr_col.clear(); bsr_diag.assign(nP, 0);
    const bool want_pattern = ch.want_pattern;
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
    hs.nnzb = (int)bsr_col.size();
    hs.bsr_max_row = 0; for (int k = 0; k < nP && want_pattern; k++) hs.bsr_max_row = std::max(hs.bsr_max_row, bsr_rowptr[k + 1] - bsr_rowptr[k]);
    lap("block pattern");
    ba_cam_table(p, hs.cam);
    return CORB_OK;
}

// the flattened graph and the estimates into device memory
int ba_upload_flat(Pool& pool, const BAHostFlat& h, const BAState& st, const BAChoice& ch, BAFlat& f)
{
    const int nP = h.nP, nL = h.nL, sp = 6 * nP;
    const bool want_pattern = ch.want_pattern;
    f.nE = h.nE; f.nP = nP; f.nL = nL; f.nnzb = h.nnzb; f.bsr_max_row = h.bsr_max_row; f.nA = h.loff[nL]; f.have_pattern = want_pattern; f.nu = (int)(h.uinfo.size() / 4);
    // local windows: the pairs of a landmark with k free-keyframe observations are at most k^2 (k (k + 1) / 2 unless a keyframe observes it twice)
    if (want_pattern && sp > 0 && sp <= 128) { size_t b = 1; for (int l = 0; l < nL; l++) b += (size_t)h.lnfree[l] * (size_t)h.lnfree[l]; f.pairs_bound = b; }
    // the estimates (quaternions | translations | points) are one block, so that push() / pop() of a trial are one copy each
    f.n_q = st.q.size(); f.n_t = st.t.size(); f.n_pt = st.pt.size();
    const size_t n_state = f.n_state();
    HIPCHK(pool.alloc(&f.dq, n_state));
    HIPCHK(pool.alloc(&f.dq_bak, n_state));
    const CorbScratch::Piece pieces[] = {
        {(void**)&f.e_pose, h.e_pose.data(), h.e_pose.size() * 4}, {(void**)&f.e_point, h.e_point.data(), h.e_point.size() * 4}, {(void**)&f.e_vpose, h.e_vpose.data(), h.e_vpose.size() * 4},
        {(void**)&f.e_vpoint, h.e_vpoint.data(), h.e_vpoint.size() * 4}, {(void**)&f.e_obs, h.e_obs.data(), h.e_obs.size() * 8}, {(void**)&f.e_w, h.e_w.data(), h.e_w.size() * 8},
        {(void**)&f.e_dim, h.e_dim.data(), h.e_dim.size()}, {(void**)&f.loff, h.loff.data(), h.loff.size() * 4}, {(void**)&f.lnfree, h.lnfree.data(), h.lnfree.size() * 4},
        {(void**)&f.poff, h.poff.data(), h.poff.size() * 4}, {(void**)&f.pedge, h.pedge.data(), h.pedge.size() * 4}, {(void**)&f.pose_vertex, h.pose_vertex.data(), h.pose_vertex.size() * 4},
        {(void**)&f.point_vertex, h.point_vertex.data(), h.point_vertex.size() * 4}, {(void**)&f.cam, h.cam.data(), h.cam.size() * 8}};
    const size_t n_pieces = sizeof(pieces) / sizeof(pieces[0]);
    size_t total = 0;
    for (const auto& pc : pieces) total += (pc.bytes + 255) & ~(size_t)255;
    if (total + n_state * 8 <= ((size_t)4 << 20)) {
        // small problems (local windows): one staging block and one copy (256-byte aligned pieces in this order), then the estimates -- sixteen synchronous copies
        // of a few KB each cost more than the optimisation itself there
        HIPCHK(pool.upload_block(pieces, n_pieces));
        static thread_local std::vector<double> blk;
        blk.resize(n_state ? n_state : 1); ba_state_pack(st, blk.data());
        if (n_state) HIPCHK(pool.h2d(f.dq, blk.data(), n_state * 8));
    } else {
        // large maps copy array by array
        for (const auto& pc : pieces) { HIPCHK(pool.alloc((char**)pc.dst, pc.bytes)); HIPCHK(pool.h2d(*pc.dst, pc.src, pc.bytes)); }
        if (f.n_q) HIPCHK(hipMemcpy(f.dq, st.q.data(), f.n_q * 8, hipMemcpyHostToDevice));
        if (f.n_t) HIPCHK(hipMemcpy(f.dq + f.n_q, st.t.data(), f.n_t * 8, hipMemcpyHostToDevice));
        if (f.n_pt) HIPCHK(hipMemcpy(f.dq + f.n_q + f.n_t, st.pt.data(), f.n_pt * 8, hipMemcpyHostToDevice));
    }
    if (want_pattern) { HIPCHK(pool.upload(&f.bsr_rowptr, h.bsr_rowptr)); HIPCHK(pool.upload(&f.bsr_col, h.bsr_col)); HIPCHK(pool.upload(&f.bsr_diag, h.bsr_diag)); }
    if (want_pattern && nP > 0) { HIPCHK(pool.upload(&f.uinfo, h.uinfo)); HIPCHK(pool.upload(&f.plm, h.plm)); }      // (the pair lists of the deterministic Schur kernel)
    return CORB_OK;
}

// ba_ml_host.cpp -- multilevel preconditioner: structure (ba_multilevel.h).  Host side, once per optimize() call: the hierarchy depends on the number of free
// keyframes and the block pattern only.
#include "ba_host.h"
#include <algorithm>

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
void ba_ml_host(int nP, MLHostAll& H)
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
int ba_ml_upload(Pool& pool, int nP, const MLHostAll& H, BAMLDev& m)
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

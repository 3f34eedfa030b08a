// corb_pnp_ransac.cpp -- C-ABI host side of the PnPsolver RANSAC (include/corb_accel.h, last section): the host-array form (corb_pnp_ransac) and the form on records
// (corb_pnp_ransac_store).  All candidates of a call are queued on one stream with one synchronisation and one read-back (ransac_run of ransac_common.h); SetRansacParameters' adjustments and the list of records are assembled here, after the read-back.
#include "pnp_ransac_internal.h"
#include "record_call.h"
#include <cstring>
#include <vector>
#include <algorithm>

namespace {
#define PNR_MAX_ITERATIONS 65535

struct PnrParams { double probability; int min_inliers, max_iterations, min_set; float epsilon, th2; int tail; const int32_t* rand_values; int max_records; };
struct PnrOut {
    int32_t* ransac_max_its; int32_t* ransac_min_inliers; int32_t* n_records; CorbPnPRansacRecord* records; uint8_t* best_flags; uint8_t* refined_flags; int flags_stride;
    int32_t* counts; double* pose_out; double* refine_pose_out;
};

// the parameters and outputs; nothing is written unless this passes
bool pnr_args_ok(const char* who, int n_cand, const PnrParams& a, const PnrOut& o)
{
    if (n_cand < 0 || a.min_set < 4 || a.min_set > 8 || a.min_inliers < a.min_set || !(a.probability > 0 && a.probability < 1) || !(a.epsilon > 0 && a.epsilon <= 1) ||
        a.max_iterations < 1 || a.max_iterations > PNR_MAX_ITERATIONS || a.tail < 0 || a.tail > PNR_MAX_ITERATIONS || a.max_records < 0 || !(a.th2 == a.th2) ||
        (n_cand > 0 && (!a.rand_values || !o.ransac_max_its || !o.ransac_min_inliers || !o.n_records)) ||
        (n_cand > 0 && a.max_records > 0 && (!o.records || !o.best_flags || !o.refined_flags))) {
        corb_set_error("%s: bad argument (4 <= min_set <= 8, min_inliers >= min_set, probability in (0, 1), epsilon in (0, 1], 1 <= max_iterations <= %d, 0 <= tail_iterations <= %d)",
                       who, PNR_MAX_ITERATIONS, PNR_MAX_ITERATIONS);
        return false;
    }
    return ransac_rand_values_ok(who, a.rand_values, (size_t)n_cand * (a.max_iterations + a.tail) * a.min_set);
}
// SetRansacParameters (:166-197), its adjustments of nMinInliers and epsilon before the shared cap: returns mRansacMaxIts (0 = iterate() sets bNoMore at once, :218-222) and
// the adjusted mRansacMinInliers
int pnr_parameters(int N, const PnrParams& a, int* min_inliers)
{
    float epsilon = a.epsilon;
    int nMinInliers = (int)((float)N * epsilon);
    if (nMinInliers < a.min_inliers) nMinInliers = a.min_inliers;
    if (nMinInliers < a.min_set) nMinInliers = a.min_set;
    *min_inliers = nMinInliers;
    if (N < nMinInliers || N <= 0) return 0;
    if (epsilon < (float)nMinInliers / (float)N) epsilon = (float)nMinInliers / (float)N;
    return ransac_iteration_cap(N, nMinInliers, epsilon, a.probability, a.max_iterations);
}
// Rcw.convertTo(CV_32F), tcw.convertTo(CV_32F) into rows 0-2 of a 4 x 4 (:262-268, :339-345)
void pnr_tcw(const PnpPose& p, float* T)
{
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T[4 * i + j] = (float)p.R[3 * i + j]; T[4 * i + 3] = (float)p.t[i]; }
}
// the records of one candidate from its read-back: iteration i is a record iff c_i >= m and c_i > every earlier c_j >= m
void pnr_records(int c, int N, int cap_its, int m, const PnrHyp* hyp, const unsigned long long* mask, const PnrHyp* ref, const unsigned long long* ref_mask, int words,
                 const int* index, const PnrParams& a, const PnrOut& o)
{
    const int stride = a.max_iterations + a.tail, its = cap_its > 0 ? cap_its + a.tail : 0;
    o.ransac_max_its[c] = cap_its; o.ransac_min_inliers[c] = m;
    if (o.counts) for (int i = 0; i < its; i++) o.counts[(size_t)c * stride + i] = hyp[i].count;
    if (o.pose_out) for (int i = 0; i < its; i++) memcpy(o.pose_out + ((size_t)c * stride + i) * 16, &hyp[i].pose, sizeof(PnpPose));
    int best = 0, n_rec = 0;
    for (int i = 0; i < its; i++) {
        const int ci = hyp[i].count;
        if (ci < m || ci <= best) continue;
        best = ci;
        if (n_rec < a.max_records) {
            const size_t r = (size_t)c * a.max_records + n_rec;
            CorbPnPRansacRecord& e = o.records[r];
            e.iteration = i + 1; e.n_inliers = ci; e.n_refined = ref[i].count; e.refine_ok = ref[i].count > m ? 1 : 0;
            pnr_tcw(hyp[i].pose, e.Tcw_best); pnr_tcw(ref[i].pose, e.Tcw_refined);
            ransac_scatter_flags(mask + (size_t)i * words, N, index, o.flags_stride, o.best_flags + r * o.flags_stride);
            ransac_scatter_flags(ref_mask + (size_t)i * words, N, index, o.flags_stride, o.refined_flags + r * o.flags_stride);
            if (o.refine_pose_out) memcpy(o.refine_pose_out + r * 16, &ref[i].pose, sizeof(PnpPose));
        }
        n_rec++;
    }
    o.n_records[c] = n_rec;
}
void pnr_clear(int n_cand, const PnrParams& a, const PnrOut& o)
{
    const size_t stride = (size_t)a.max_iterations + a.tail;
    for (int c = 0; c < n_cand; c++) { o.ransac_max_its[c] = 0; o.ransac_min_inliers[c] = 0; o.n_records[c] = 0; }
    if (a.max_records > 0 && n_cand > 0) {
        memset(o.records, 0, (size_t)n_cand * a.max_records * sizeof(CorbPnPRansacRecord));
        memset(o.best_flags, 0, (size_t)n_cand * a.max_records * o.flags_stride);
        memset(o.refined_flags, 0, (size_t)n_cand * a.max_records * o.flags_stride);
        if (o.refine_pose_out) memset(o.refine_pose_out, 0, (size_t)n_cand * a.max_records * 16 * sizeof(double));
    }
    if (o.counts) memset(o.counts, 0, (size_t)n_cand * stride * 4);
    if (o.pose_out) memset(o.pose_out, 0, (size_t)n_cand * stride * 16 * sizeof(double));
}
}  // namespace

extern "C" int corb_pnp_ransac(const CorbPnPRansacProblem* problems, int n_problems, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                               float th2, int tail_iterations, const int32_t* rand_values, int max_records, int flags_stride, int32_t* ransac_max_its,
                               int32_t* ransac_min_inliers, int32_t* n_records, CorbPnPRansacRecord* records, uint8_t* best_flags, uint8_t* refined_flags, int32_t* counts,
                               double* pose_out, double* refine_pose_out, int device)
{
    const char* who = "corb_pnp_ransac";
    const PnrParams a{probability, min_inliers, max_iterations, min_set, epsilon, th2, tail_iterations, rand_values, max_records};
    const PnrOut o{ransac_max_its, ransac_min_inliers, n_records, records, best_flags, refined_flags, flags_stride, counts, pose_out, refine_pose_out};
    if (n_problems > 0 && !problems) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    int cap = 0; size_t rows = 0;
    for (int c = 0; c < n_problems; c++) {
        const CorbPnPRansacProblem& p = problems[c];
        if (p.n < 0 || p.n > flags_stride || (p.n > 0 && (!p.p3dw || !p.p2d || !p.sigma2))) { corb_set_error("%s: problem %d: NULL array, or n outside [0, flags_stride]", who, c); return CORB_ERR_ARG; }
        cap = std::max(cap, p.n); rows += (size_t)p.n;
    }
    if (!pnr_args_ok(who, n_problems, a, o)) return CORB_ERR_ARG;
    int rc = corb_select_device(device); if (rc) return rc;
    pnr_clear(n_problems, a, o);
    std::vector<PnrCand> cand((size_t)n_problems); std::vector<int> cap_its((size_t)n_problems), h_n((size_t)n_problems), m_of((size_t)n_problems);
    static thread_local std::vector<float> in; in.resize(rows * 6);
    int grid_its = 0; size_t row = 0;
    for (int c = 0; c < n_problems; c++) {
        const CorbPnPRansacProblem& p = problems[c]; PnrCand& cd = cand[c];
        memset(&cd, 0, sizeof(cd));
        cap_its[c] = pnr_parameters(p.n, a, &m_of[c]);
        cd.n = p.n; h_n[c] = p.n; cd.its = cap_its[c] > 0 ? cap_its[c] + a.tail : 0; cd.in_off = (int)row;
        cd.K[0] = p.fx; cd.K[1] = p.fy; cd.K[2] = p.cx; cd.K[3] = p.cy;
        for (int i = 0; i < p.n; i++, row++) {
            float* r = &in[row * 6];
            for (int k = 0; k < 3; k++) r[k] = p.p3dw[3 * (size_t)i + k];
            r[3] = p.p2d[2 * (size_t)i]; r[4] = p.p2d[2 * (size_t)i + 1]; r[5] = p.sigma2[i];
        }
        ransac_min_inliers[c] = m_of[c];
        grid_its = std::max(grid_its, cd.its);
    }
    if (grid_its == 0) return CORB_OK;                       // every problem has N < mRansacMinInliers: bNoMore at once, nothing to run
    CorbScratch pool(0);
    PnrDev d; memset(&d, 0, sizeof(d));
    d.n_cand = n_problems; d.cap = cap; d.stride_its = max_iterations + tail_iterations; d.min_set = min_set; d.th2 = th2;
    d.min_inliers = min_inliers; d.epsilon = epsilon;
    HIPCHK(pool.upload_block({{(void**)&d.cand, cand.data(), cand.size() * sizeof(PnrCand)}, {(void**)&d.in, in.data(), rows * 24}, {(void**)&d.set.ncorr, h_n.data(), h_n.size() * 4},
                              {(void**)&d.rand_values, rand_values, (size_t)n_problems * d.stride_its * min_set * 4}}));
    static thread_local std::vector<PnrHyp> h_hyp, h_ref; static thread_local std::vector<unsigned long long> h_mask, h_ref_mask;
    rc = ransac_run<PnrHyp>(pool, d, false, (size_t)n_problems * d.stride_its, corb_launch_pnp_ransac, grid_its, {{&d.out, &h_hyp, &h_mask}, {&d.ref, &h_ref, &h_ref_mask}}, nullptr, nullptr);
    if (rc) return rc;
    for (int c = 0; c < n_problems; c++) {
        const size_t h0 = (size_t)c * d.stride_its;
        pnr_records(c, problems[c].n, cap_its[c], m_of[c], h_hyp.data() + h0, h_mask.data() + h0 * d.words, h_ref.data() + h0, h_ref_mask.data() + h0 * d.words,
                    d.words, nullptr, a, o);
    }
    return CORB_OK;
}

extern "C" int corb_pnp_ransac_store(CorbKfStore* frames, int slot, CorbMpStore* map, const CorbTrackCamera* cam, const uint64_t* matched_ids, int n_candidates,
                                     double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2, int tail_iterations,
                                     const int32_t* rand_values, int max_records, int32_t* ransac_max_its, int32_t* ransac_min_inliers, int32_t* n_records,
                                     CorbPnPRansacRecord* records, uint8_t* best_flags, uint8_t* refined_flags, int32_t* n_corr, int32_t* index, int32_t* counts,
                                     double* pose_out, double* refine_pose_out)
{
    const char* who = "corb_pnp_ransac_store";
    if (!frames || !map || !cam || slot < 0 || slot >= frames->capacity || frames->device != map->device || n_candidates < 0 || (n_candidates > 0 && (!matched_ids || !n_corr)) ||
        cam->nlevels < 1 || cam->nlevels > CORB_MAX_LEVELS) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    int rc = corb_select_device(frames->device); if (rc) return rc;
    RecordCall call; call.hold(nullptr, frames, nullptr, map);
    const int n1 = record_slot_count(who, frames, slot); if (n1 < 0) return CORB_ERR_ARG;
    rc = record_need_index(who, map); if (rc) return rc;
    const PnrParams a{probability, min_inliers, max_iterations, min_set, epsilon, th2, tail_iterations, rand_values, max_records};
    const PnrOut o{ransac_max_its, ransac_min_inliers, n_records, records, best_flags, refined_flags, n1, counts, pose_out, refine_pose_out};
    if (!pnr_args_ok(who, n_candidates, a, o)) return CORB_ERR_ARG;
    pnr_clear(n_candidates, a, o);
    ransac_corr_preset(n_candidates, n1, n_corr, index);
    if (n_candidates == 0 || n1 == 0) return CORB_OK;
    rc = call.join(); if (rc) return rc;
    const int stride_its = max_iterations + tail_iterations;
    std::vector<PnrCand> cand((size_t)n_candidates);
    for (int c = 0; c < n_candidates; c++) { PnrCand& cd = cand[c]; memset(&cd, 0, sizeof(cd)); cd.n = n1; cd.its = stride_its; }
    CorbScratch pool(0);
    PnrDev d; memset(&d, 0, sizeof(d));
    d.n_cand = n_candidates; d.cap = n1; d.stride_its = stride_its; d.min_set = min_set; d.th2 = th2; d.min_inliers = min_inliers; d.epsilon = epsilon;
    d.kf = frames->rec(slot); d.F = frames->F; d.nlevels = cam->nlevels;
    for (int l = 0; l < CORB_MAX_LEVELS; l++) d.scale[l] = l < cam->nlevels ? cam->scale[l] : 1.f;
    d.mp_base = map->base(); d.mp_bytes = map->L.bytes; d.idt = map->idt;
    HIPCHK(pool.upload_block({{(void**)&d.cand, cand.data(), cand.size() * sizeof(PnrCand)}, {(void**)&d.matched, matched_ids, (size_t)n_candidates * n1 * 8},
                              {(void**)&d.rand_values, rand_values, (size_t)n_candidates * stride_its * min_set * 4}}));
    static thread_local std::vector<PnrHyp> h_hyp, h_ref; static thread_local std::vector<unsigned long long> h_mask, h_ref_mask; std::vector<int> h_n, h_index;
    rc = ransac_run<PnrHyp>(pool, d, true, (size_t)n_candidates * stride_its, corb_launch_pnp_ransac, stride_its, {{&d.out, &h_hyp, &h_mask}, {&d.ref, &h_ref, &h_ref_mask}}, &h_n, &h_index);
    if (rc) return rc;
    for (int c = 0; c < n_candidates; c++) {
        const int N = ransac_corr_out(h_n.data(), h_index.data(), c, n1, n_corr, index);
        int m = 0; const int cap_its = pnr_parameters(N, a, &m);
        const size_t h0 = (size_t)c * stride_its;
        pnr_records(c, N, cap_its, m, h_hyp.data() + h0, h_mask.data() + h0 * d.words, h_ref.data() + h0, h_ref_mask.data() + h0 * d.words, d.words,
                    h_index.data() + (size_t)c * n1, a, o);
    }
    return CORB_OK;
}

// corb_sim3_ransac.cpp -- C-ABI host side of the Sim3Solver RANSAC (include/corb_accel.h, last section): the host-array form (corb_sim3_ransac) and the form on
// records (corb_sim3_ransac_store).  All candidates of a call are queued on one stream with one synchronisation and one read-back (ransac_run); the rule that turns
// the per-hypothesis inlier counts into iterate()'s returns is stated once, here, for both.  What the PnP route shares is in ransac_common.h.
#include "sim3_ransac_internal.h"
#include "record_call.h"
#include <cstring>
#include <vector>
#include <algorithm>

namespace {
#define S3R_MAX_ITERATIONS 65535

struct S3rParams { double probability; int min_inliers, max_iterations, fix_scale; const int32_t* rand_values; int max_events; };
struct S3rOut { int32_t* ransac_max_its; int32_t* n_events; CorbSim3RansacEvent* events; uint8_t* inlier_flags; int flags_stride; int32_t* counts; float* q_out; };

// the parameters and outputs both routes share; nothing is written unless this passes
bool s3r_args_ok(const char* who, int n_cand, const S3rParams& a, const S3rOut& o)
{
    if (n_cand < 0 || !(a.probability > 0 && a.probability < 1) || a.min_inliers < 3 || a.max_iterations < 1 || a.max_iterations > S3R_MAX_ITERATIONS || a.max_events < 0 ||
        (n_cand > 0 && (!a.rand_values || !o.ransac_max_its || !o.n_events)) || (n_cand > 0 && a.max_events > 0 && (!o.events || !o.inlier_flags))) {
        corb_set_error("%s: bad argument (probability in (0, 1), min_inliers >= 3, 1 <= max_iterations <= %d)", who, S3R_MAX_ITERATIONS); return false;
    }
    return ransac_rand_values_ok(who, a.rand_values, (size_t)n_cand * a.max_iterations * 3);
}
// SetRansacParameters (:114-138): epsilon = (float)nMinInliers / N (N >= 1 wherever it is read)
int s3r_cap(int N, const S3rParams& a) { return ransac_iteration_cap(N, a.min_inliers, (float)a.min_inliers / std::max(N, 1), a.probability, a.max_iterations); }
// iterate() (:158-201) over the counts c_i of one candidate: iteration i returns iff c_i > minInliers and c_i >= max_{j<i} c_j.  hyp / mask: this candidate's
// read-back; index1 (record route): mvnIndices1, through which the flags are scattered (:195-197).
void s3r_events(int c, int N, int cap_its, const S3rHyp* hyp, const unsigned long long* mask, int words, const int* index1, const S3rParams& a, const S3rOut& o)
{
    o.ransac_max_its[c] = cap_its;
    if (o.counts) for (int i = 0; i < a.max_iterations; i++) o.counts[(size_t)c * a.max_iterations + i] = i < cap_its ? hyp[i].count : 0;
    if (o.q_out) for (int i = 0; i < a.max_iterations; i++) for (int k = 0; k < 4; k++) o.q_out[((size_t)c * a.max_iterations + i) * 4 + k] = i < cap_its ? hyp[i].q[k] : 0.f;
    int best = 0, n_ev = 0;
    for (int i = 0; i < cap_its; i++) {
        const int ci = hyp[i].count;
        if (ci < best) continue;
        best = ci;
        if (ci <= a.min_inliers) continue;
        if (n_ev < a.max_events) {
            CorbSim3RansacEvent& e = o.events[(size_t)c * a.max_events + n_ev];
            e.iteration = i + 1; e.n_inliers = ci; e.s12 = hyp[i].s;
            memcpy(e.R12, hyp[i].R, sizeof(e.R12)); memcpy(e.t12, hyp[i].t, sizeof(e.t12));
            ransac_scatter_flags(mask + (size_t)i * words, N, index1, o.flags_stride, o.inlier_flags + ((size_t)c * a.max_events + n_ev) * o.flags_stride);
        }
        n_ev++;
    }
    o.n_events[c] = n_ev;
}
void s3r_clear(int n_cand, const S3rParams& a, const S3rOut& o)
{
    for (int c = 0; c < n_cand; c++) { o.ransac_max_its[c] = 0; o.n_events[c] = 0; }
    if (a.max_events > 0 && n_cand > 0) {
        memset(o.events, 0, (size_t)n_cand * a.max_events * sizeof(CorbSim3RansacEvent));
        memset(o.inlier_flags, 0, (size_t)n_cand * a.max_events * o.flags_stride);
    }
    if (o.counts) memset(o.counts, 0, (size_t)n_cand * a.max_iterations * 4);
    if (o.q_out) memset(o.q_out, 0, (size_t)n_cand * a.max_iterations * 16);
}
}  // namespace

extern "C" int corb_sim3_ransac(const CorbSim3RansacProblem* problems, int n_problems, double probability, int min_inliers, int max_iterations, int fix_scale,
                                const int32_t* rand_values, int max_events, int flags_stride, int32_t* ransac_max_its, int32_t* n_events, CorbSim3RansacEvent* events,
                                uint8_t* inlier_flags, int32_t* counts, float* q_out, int device)
{
    const char* who = "corb_sim3_ransac";
    const S3rParams a{probability, min_inliers, max_iterations, fix_scale ? 1 : 0, rand_values, max_events};
    const S3rOut o{ransac_max_its, n_events, events, inlier_flags, flags_stride, counts, q_out};
    if (n_problems > 0 && !problems) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    int cap = 0; size_t rows = 0;
    for (int c = 0; c < n_problems; c++) {
        const CorbSim3RansacProblem& p = problems[c];
        if (p.n < 0 || p.n > flags_stride || (p.n > 0 && (!p.p1c || !p.p2c || !p.sigma2_1 || !p.sigma2_2))) { corb_set_error("%s: problem %d: NULL array, or n outside [0, flags_stride]", who, c); return CORB_ERR_ARG; }
        cap = std::max(cap, p.n); rows += (size_t)p.n;
    }
    if (!s3r_args_ok(who, n_problems, a, o)) return CORB_ERR_ARG;
    int rc = corb_select_device(device); if (rc) return rc;
    s3r_clear(n_problems, a, o);
    std::vector<S3rCand> cand((size_t)n_problems); std::vector<int> h_n((size_t)n_problems);
    static thread_local std::vector<float> in; in.resize(rows * 8);
    int grid_its = 0; size_t row = 0;
    for (int c = 0; c < n_problems; c++) {
        const CorbSim3RansacProblem& p = problems[c]; S3rCand& cd = cand[c];
        memset(&cd, 0, sizeof(cd));
        cd.n = p.n; cd.its = s3r_cap(p.n, a); cd.in_off = (int)row; h_n[c] = p.n;
        cd.K1[0] = p.fx1; cd.K1[1] = p.fy1; cd.K1[2] = p.cx1; cd.K1[3] = p.cy1; cd.K2[0] = p.fx2; cd.K2[1] = p.fy2; cd.K2[2] = p.cx2; cd.K2[3] = p.cy2;
        for (int i = 0; i < p.n; i++, row++) {
            float* r = &in[row * 8];
            for (int k = 0; k < 3; k++) { r[k] = p.p1c[3 * (size_t)i + k]; r[3 + k] = p.p2c[3 * (size_t)i + k]; }
            r[6] = p.sigma2_1[i]; r[7] = p.sigma2_2[i];
        }
        grid_its = std::max(grid_its, cd.its);
    }
    if (grid_its == 0) return CORB_OK;                       // every problem has N < min_inliers: bNoMore at once, nothing to run
    CorbScratch pool(0);
    S3rDev d; memset(&d, 0, sizeof(d));
    d.n_cand = n_problems; d.cap = cap; d.max_its = max_iterations; d.min_inliers = min_inliers; d.fix_scale = a.fix_scale;
    HIPCHK(pool.upload_block({{(void**)&d.cand, cand.data(), cand.size() * sizeof(S3rCand)}, {(void**)&d.in, in.data(), rows * 32}, {(void**)&d.set.ncorr, h_n.data(), h_n.size() * 4},
                              {(void**)&d.rand_values, rand_values, (size_t)n_problems * max_iterations * 12}}));
    static thread_local std::vector<S3rHyp> h_hyp; static thread_local std::vector<unsigned long long> h_mask;
    rc = ransac_run<S3rHyp>(pool, d, false, (size_t)n_problems * max_iterations, corb_launch_sim3_ransac, grid_its, {{&d.out, &h_hyp, &h_mask}}, nullptr, nullptr); if (rc) return rc;
    for (int c = 0; c < n_problems; c++)
        s3r_events(c, h_n[c], cand[c].its, h_hyp.data() + (size_t)c * max_iterations, h_mask.data() + (size_t)c * max_iterations * d.words, d.words, nullptr, a, o);
    return CORB_OK;
}

extern "C" int corb_sim3_ransac_store(CorbKfStore* kf, int slot1, const int32_t* slots2, int n_candidates, CorbMpStore* map, const CorbTrackCamera* cam1,
                                      const CorbTrackCamera* cam2, const uint64_t* matched12_ids, double probability, int min_inliers, int max_iterations, int fix_scale,
                                      const int32_t* rand_values, int max_events, int32_t* ransac_max_its, int32_t* n_events, CorbSim3RansacEvent* events,
                                      uint8_t* inlier_flags, int32_t* n_corr, int32_t* index1, int32_t* counts, float* q_out)
{
    const char* who = "corb_sim3_ransac_store";
    if (!kf || !map || !cam1 || slot1 < 0 || slot1 >= kf->capacity || kf->device != map->device || n_candidates < 0 ||
        (n_candidates > 0 && (!slots2 || !cam2 || !matched12_ids || !n_corr)) || cam1->nlevels < 1 || cam1->nlevels > CORB_MAX_LEVELS) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    for (int c = 0; c < n_candidates; c++)
        if (slots2[c] < 0 || slots2[c] >= kf->capacity || slots2[c] == slot1 || cam2[c].nlevels < 1 || cam2[c].nlevels > CORB_MAX_LEVELS) { corb_set_error("%s: candidate %d: bad slot or camera", who, c); return CORB_ERR_ARG; }
    int rc = corb_select_device(kf->device); if (rc) return rc;
    RecordCall call; call.hold(nullptr, kf, nullptr, map);
    const int n1 = record_slot_count(who, kf, slot1); if (n1 < 0) return CORB_ERR_ARG;
    for (int c = 0; c < n_candidates; c++) if (kf->host[slots2[c]].n < 0) { corb_set_error("%s: candidate slot %d is empty", who, slots2[c]); return CORB_ERR_ARG; }
    rc = record_need_index(who, map); if (rc) return rc;
    const S3rParams a{probability, min_inliers, max_iterations, fix_scale ? 1 : 0, rand_values, max_events};
    const S3rOut o{ransac_max_its, n_events, events, inlier_flags, n1, counts, q_out};
    if (!s3r_args_ok(who, n_candidates, a, o)) return CORB_ERR_ARG;
    s3r_clear(n_candidates, a, o);
    ransac_corr_preset(n_candidates, n1, n_corr, index1);
    if (n_candidates == 0 || n1 == 0) return CORB_OK;
    rc = call.join(); if (rc) return rc;
    std::vector<S3rCand> cand((size_t)n_candidates);
    for (int c = 0; c < n_candidates; c++) {
        S3rCand& cd = cand[c]; memset(&cd, 0, sizeof(cd));
        cd.n = n1; cd.its = max_iterations; cd.kf2 = kf->rec(slots2[c]); cd.n2 = kf->host[slots2[c]].n; cd.nlevels2 = cam2[c].nlevels;
        for (int l = 0; l < CORB_MAX_LEVELS; l++) cd.scale2[l] = l < cam2[c].nlevels ? cam2[c].scale[l] : 1.f;
    }
    CorbScratch pool(0);
    S3rDev d; memset(&d, 0, sizeof(d));
    d.n_cand = n_candidates; d.cap = n1; d.max_its = max_iterations; d.min_inliers = min_inliers; d.fix_scale = a.fix_scale;
    d.kf1 = kf->rec(slot1); d.F = kf->F; d.nlevels1 = cam1->nlevels;
    for (int l = 0; l < CORB_MAX_LEVELS; l++) d.scale1[l] = l < cam1->nlevels ? cam1->scale[l] : 1.f;
    d.mp_base = map->base(); d.mp_bytes = map->L.bytes; d.max_obs = map->O; d.idt = map->idt;
    HIPCHK(pool.upload_block({{(void**)&d.cand, cand.data(), cand.size() * sizeof(S3rCand)}, {(void**)&d.matched12, matched12_ids, (size_t)n_candidates * n1 * 8},
                              {(void**)&d.rand_values, rand_values, (size_t)n_candidates * max_iterations * 12}}));
    static thread_local std::vector<S3rHyp> h_hyp; static thread_local std::vector<unsigned long long> h_mask; std::vector<int> h_n, h_index1;
    rc = ransac_run<S3rHyp>(pool, d, true, (size_t)n_candidates * max_iterations, corb_launch_sim3_ransac, max_iterations, {{&d.out, &h_hyp, &h_mask}}, &h_n, &h_index1); if (rc) return rc;
    for (int c = 0; c < n_candidates; c++) {
        const int N = ransac_corr_out(h_n.data(), h_index1.data(), c, n1, n_corr, index1);
        s3r_events(c, N, s3r_cap(N, a), h_hyp.data() + (size_t)c * max_iterations, h_mask.data() + (size_t)c * max_iterations * d.words, d.words,
                   h_index1.data() + (size_t)c * n1, a, o);
    }
    return CORB_OK;
}

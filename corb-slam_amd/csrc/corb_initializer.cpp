// corb_initializer.cpp -- C-ABI host side of the monocular Initializer (include/corb_accel.h, last section): corb_mono_initialize.  The call's set-up -- Normalize of
// both key sets (a serial float sum in ascending order), the packed matches, the two cosine thresholds that stand for the parallax tests -- is done here; all problems
// are queued on one stream with one synchronisation and one read-back, and the reported parallax is computed from the returned cosines.
#include "init_internal.h"
#include "corb_workspace.h"
#include <cstring>
#include <vector>
#include <algorithm>

#include "host_util.h"

static_assert(sizeof(InitResult) == sizeof(CorbInitResult) && sizeof(CorbInitResult) == 264, "CorbInitResult is InitResult, field for field");
static_assert(INIT_OK == CORB_INIT_OK && INIT_NO_MODEL == CORB_INIT_NO_MODEL && INIT_H_DEGENERATE == CORB_INIT_H_DEGENERATE && INIT_AMBIGUOUS == CORB_INIT_AMBIGUOUS &&
              INIT_FEW_POINTS == CORB_INIT_FEW_POINTS && INIT_LOW_PARALLAX == CORB_INIT_LOW_PARALLAX, "status values");

extern "C" int corb_mono_initialize(const CorbInitProblem* problems, int n_problems, float sigma, int max_iterations, float min_parallax, int min_triangulated,
                                    const int32_t* rand_values, int p3d_stride, int flags_stride, CorbInitResult* results, float* p3d, uint8_t* triangulated,
                                    uint8_t* inliers_h, uint8_t* inliers_f, float* scores, int device)
{
    const char* who = "corb_mono_initialize";
    if (n_problems < 0 || n_problems > 65535 || max_iterations < 1 || max_iterations > 65535 || !(sigma > 0) || !(min_parallax == min_parallax) ||
        (n_problems > 0 && (!problems || !rand_values || !results || !p3d || !triangulated))) {
        corb_set_error("%s: bad argument (0 <= n_problems <= 65535, 1 <= max_iterations <= 65535, sigma > 0)", who);
        return CORB_ERR_ARG;
    }
    if (n_problems == 0) return CORB_OK;
    static thread_local std::vector<InitProb> prob; static thread_local std::vector<InitMatch> match;
    prob.assign((size_t)n_problems, InitProb{}); match.clear();
    int capN = 0, cap1 = 0;
    for (int c = 0; c < n_problems; c++) {
        const CorbInitProblem& q = problems[c]; InitProb& p = prob[c];
        if (q.n1 < 1 || q.n2 < 1 || !q.keys1 || !q.keys2 || !q.matches12 || q.n1 > p3d_stride) {
            corb_set_error("%s: problem %d: NULL array, no keys, or n1 above p3d_stride", who, c); return CORB_ERR_ARG;
        }
        p.n1 = q.n1; p.match_off = (int)match.size(); p.fx = q.fx; p.fy = q.fy; p.cx = q.cx; p.cy = q.cy;
        for (int i = 0; i < q.n1; i++) {                                                // mvMatches12 (:54-63)
            const int j = q.matches12[i];
            if (j < -1 || j >= q.n2) { corb_set_error("%s: problem %d: matches12[%d] = %d is outside [-1, n2)", who, c, i, j); return CORB_ERR_ARG; }
            if (j >= 0) match.push_back({q.keys1[i].x, q.keys1[i].y, q.keys2[j].x, q.keys2[j].y, i, j});
        }
        p.N = (int)match.size() - p.match_off;
        if (p.N < 8) { corb_set_error("%s: problem %d has %d matches; the 8-point sets need 8", who, c, p.N); return CORB_ERR_ARG; }
        if ((inliers_h || inliers_f) && p.N > flags_stride) { corb_set_error("%s: problem %d has %d matches, above flags_stride", who, c, p.N); return CORB_ERR_ARG; }
        capN = std::max(capN, p.N); cap1 = std::max(cap1, q.n1);
    }
    const size_t n_rand = (size_t)n_problems * max_iterations * 8;
    if (!ransac_rand_values_ok(who, rand_values, n_rand)) return CORB_ERR_ARG;
    int rc = corb_select_device(device); if (rc) return rc;
    for (int c = 0; c < n_problems; c++) {                                              // Normalize over all keys of each frame (:132-133)
        const CorbInitProblem& q = problems[c];
        init_normalize(&q.keys1[0].x, (int)(sizeof(CorbKeyPoint) / sizeof(float)), q.n1, prob[c].nrm1);
        init_normalize(&q.keys2[0].x, (int)(sizeof(CorbKeyPoint) / sizeof(float)), q.n2, prob[c].nrm2);
    }
    CorbScratch pool(0);
    InitDev d; memset(&d, 0, sizeof(d));
    d.n_problems = n_problems; d.max_iterations = max_iterations; d.words = (capN + 63) / 64; d.cap1 = cap1; d.p3d_stride = p3d_stride; d.flags_stride = flags_stride;
    d.min_triangulated = min_triangulated; d.sigma = sigma; d.min_parallax = min_parallax;
    d.cos_thr_f = init_cos_threshold(min_parallax, true); d.cos_thr_h = init_cos_threshold(min_parallax, false);
    HIPCHK(pool.upload_block({{(void**)&d.prob, prob.data(), prob.size() * sizeof(InitProb)}, {(void**)&d.match, match.data(), match.size() * sizeof(InitMatch)},
                              {(void**)&d.rand_values, rand_values, n_rand * 4}}));
    const size_t nh = (size_t)n_problems * max_iterations * 2, nc = (size_t)n_problems * 8, capM = (size_t)d.words * 64;
    const size_t n_p3d = (size_t)n_problems * p3d_stride * 3, n_tri = (size_t)n_problems * p3d_stride, n_fl = (size_t)n_problems * flags_stride;
    HIPCHK(pool.alloc(&d.scores, nh)); HIPCHK(pool.alloc(&d.hyp_m, nh * 9)); HIPCHK(pool.alloc(&d.mask, nh * d.words)); HIPCHK(pool.alloc(&d.sel, (size_t)n_problems));
    HIPCHK(pool.alloc(&d.cand_p3d, nc * cap1 * 3)); HIPCHK(pool.alloc(&d.cand_good, nc * cap1)); HIPCHK(pool.alloc(&d.cand_cos, nc * capM)); HIPCHK(pool.alloc(&d.cand_pushed, nc * capM));
    HIPCHK(pool.alloc(&d.res, (size_t)n_problems)); HIPCHK(pool.alloc(&d.p3d, n_p3d)); HIPCHK(pool.alloc(&d.tri, n_tri));
    if (inliers_h) HIPCHK(pool.alloc(&d.inl_h, n_fl));
    if (inliers_f) HIPCHK(pool.alloc(&d.inl_f, n_fl));
    HIPCHK(hipMemsetAsync(d.cand_p3d, 0, nc * cap1 * 3 * sizeof(float), pool.stream)); HIPCHK(hipMemsetAsync(d.cand_good, 0, nc * cap1, pool.stream));
    HIPCHK(hipMemsetAsync(d.p3d, 0, n_p3d * sizeof(float), pool.stream)); HIPCHK(hipMemsetAsync(d.tri, 0, n_tri, pool.stream));
    if (inliers_h) HIPCHK(hipMemsetAsync(d.inl_h, 0, n_fl, pool.stream));
    if (inliers_f) HIPCHK(hipMemsetAsync(d.inl_f, 0, n_fl, pool.stream));
    corb_launch_mono_initialize(d, pool.stream);
    HIPCHK(hipGetLastError());
    HIPCHK(pool.d2h(results, d.res, (size_t)n_problems * sizeof(CorbInitResult))); HIPCHK(pool.d2h(p3d, d.p3d, n_p3d * sizeof(float))); HIPCHK(pool.d2h(triangulated, d.tri, n_tri));
    if (inliers_h) HIPCHK(pool.d2h(inliers_h, d.inl_h, n_fl));
    if (inliers_f) HIPCHK(pool.d2h(inliers_f, d.inl_f, n_fl));
    if (scores) HIPCHK(pool.d2h(scores, d.scores, nh * sizeof(float)));
    HIPCHK(pool.fetch_finish());
    for (int c = 0; c < n_problems; c++) init_fill_parallax(*reinterpret_cast<InitResult*>(&results[c]));     // :901 on the host, from the returned cosine
    return CORB_OK;
}

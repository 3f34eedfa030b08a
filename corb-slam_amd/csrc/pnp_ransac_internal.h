// pnp_ransac_internal.h -- device-side argument blocks of the PnPsolver RANSAC (pnp_ransac_kernels.hip, corb_pnp_ransac.cpp)
#pragma once
#include "corb_internal.h"
#include "store_internal.h"
#include "device_util.h"
#include "pnp_math.h"
#include "ransac_common.h"

// what one hypothesis, or one record's Refine(), leaves (mask words apart)
struct PnrHyp { int count, pad; PnpPose pose; };
// one candidate (uploaded per call)
struct PnrCand {
    int n;                                // host-array route: correspondences given; record route: features of the frame
    int its;                              // hypotheses to evaluate: host-array route mRansacMaxIts + tail_iterations, record route all of stride_its (N is the device's)
    float K[4];                           // host-array route: fx, fy, cx, cy (record route: the record's meta)
    int in_off;                           // host-array route: first row of this problem in PnrDev::in
};
struct PnrDev {
    int n_cand, cap, stride_its, min_set, words;      // cap = correspondence slots per candidate, stride_its = max_iterations + tail_iterations, words = ceil(cap / 64)
    int min_inliers; float epsilon, th2;              // SetRansacParameters' arguments: mRansacMinInliers = max(int(N * epsilon), min_inliers, min_set) (:179-184)
    const PnrCand* cand;
    const float* in;                      // host-array route: rows of (p3dw[3], p2d[2], sigma2)
    // record route (kf != nullptr)
    const char* kf; int F; float scale[CORB_MAX_LEVELS]; int nlevels;
    const char* mp_base; size_t mp_bytes; CorbIdTable idt;
    const unsigned long long* matched;    // [n_cand][cap] vpMapPointMatches as MapPoint ids
    // both routes
    RansacCorrSet<PnpCorr> set;           // per feature of the frame; corr = the N accepted correspondences in ascending feature order, index = mvKeyPointIndices
    const int* rand_values;               // [n_cand][stride_its][min_set]
    RansacHyps<PnrHyp> out, ref;          // [n_cand][stride_its]: the hypotheses, and the same for Refine() (written at records only)
};
// prepare (+ scan + compaction on the record route; scan_scratch: corb_scan_scratch_ints(n_cand * cap) ints), then one wavefront per (iteration, candidate) for the
// hypotheses and again for Refine()
void corb_launch_pnp_ransac(const PnrDev& d, int grid_its, int* scan_scratch, hipStream_t s);

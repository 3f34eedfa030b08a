// sim3_ransac_internal.h -- device-side argument blocks of the Sim3Solver RANSAC (sim3_ransac_kernels.hip, corb_sim3_ransac.cpp)
#pragma once
#include "corb_internal.h"
#include "store_internal.h"
#include "device_util.h"
#include "ransac_common.h"

// one correspondence as CheckInliers reads it: mvX3Dc1 / mvX3Dc2, mvP1im1 / mvP2im2, mvnMaxError1 / mvnMaxError2 (the truncated integers, held as floats)
struct S3rCorr { float x1[3], x2[3], p1[2], p2[2], th1, th2; };
// what one hypothesis leaves (mask words apart)
struct S3rHyp { int count; float s; float q[4]; float R[9]; float t[3]; };
// one candidate (uploaded per call)
struct S3rCand {
    int n;                                // host-array route: correspondences given; record route: features of keyframe 1
    int its;                              // hypotheses to evaluate (the grid may hold more)
    float K1[4], K2[4];                   // host-array route: fx, fy, cx, cy of both cameras (record route: the records' meta)
    int in_off;                           // host-array route: first row of this problem in S3rDev::in
    int n2; const char* kf2;              // record route: keyframe 2's record and feature count
    float scale2[CORB_MAX_LEVELS]; int nlevels2;
};
struct S3rDev {
    int n_cand, cap, max_its, min_inliers, fix_scale, words;      // cap = correspondence slots per candidate, words = ceil(cap / 64)
    const S3rCand* cand;
    const float* in;                      // host-array route: rows of (p1c[3], p2c[3], sigma2_1, sigma2_2)
    // record route (kf1 != nullptr)
    const char* kf1; int F; float scale1[CORB_MAX_LEVELS]; int nlevels1;
    const char* mp_base; size_t mp_bytes; int max_obs; CorbIdTable idt;
    const unsigned long long* matched12;  // [n_cand][cap] vpMatched12 as MapPoint ids
    // both routes
    RansacCorrSet<S3rCorr> set;           // per feature of keyframe 1; corr = the N accepted correspondences in ascending i1, index = mvnIndices1
    const int* rand_values;               // [n_cand][max_its][3]
    RansacHyps<S3rHyp> out;               // [n_cand][max_its]
};
// prepare (+ scan + compaction on the record route; scan_scratch: corb_scan_scratch_ints(n_cand * cap) ints), then one wavefront per (candidate, iteration)
void corb_launch_sim3_ransac(const S3rDev& d, int grid_its, int* scan_scratch, hipStream_t s);

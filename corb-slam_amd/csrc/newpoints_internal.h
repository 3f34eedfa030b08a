// newpoints_internal.h -- device-side argument blocks of LocalMapping::CreateNewMapPoints (newpoints_kernels.hip, corb_newpoints.cpp)
#pragma once
#include "corb_internal.h"
#include "store_internal.h"

#define CORB_NP_NONE 0xFFu                // record form, dense arrays: this (neighbour, feature) entry holds no pair

// one keyframe as the triangulation reads it: feature arrays in device memory; pose and intrinsics from the record's header (hdr != nullptr) or by value
struct NpSide {
    const CorbKeyPoint* kp; const float* ur; const float* depth;
    const KfHeader* hdr;
    float Tcw[16]; float fx, fy, cx, cy, bf;
    float mb; int nlevels; float scale[CORB_MAX_LEVELS];       // mb, mvScaleFactors (mvLevelSigma2 = scale^2 in float)
};
struct NpDev {
    NpSide s1, s2;
    const int* pairs;                     // host-array form: n x (idx1, idx2)
    const int* match;                     // record form: idx2 per feature of keyframe 1, -1 = no pair (pairs == nullptr)
    int n, n2;                            // work items (pairs, or features of keyframe 1); features of keyframe 2
    float* x3d; unsigned char* status; unsigned char* source;      // per work item
    unsigned char* flags1;                // record form: the evolving has-a-map-point flags of keyframe 1 (set where a pair is CORB_NP_OK); may be nullptr
    int* winner;                          // record form: per feature of keyframe 2 the largest idx1 of an OK pair (AddMapPoint keeps the later one); may be nullptr
    int* n_new;
};
void corb_launch_newpoints(const NpDev& d, hipStream_t s);

// record form, after the last neighbour: ranks of the OK pairs in (neighbour, idx1) order, then the records
struct NpApplyDev {
    int n_nb, n1, apply;
    const int* match; const float* x3d; const unsigned char* status;      // dense [n_nb][n1]
    const int* winner;                    // [n_nb][F]
    int* rank;                            // [n_nb][n1] out: k of an OK pair
    int* totals;                          // [0] = n_new, [1] = 1 if the map store is too small
    char* kf_base; size_t kf_bytes; int F; int cur_slot; const int* nb_slots;
    char* mp_base; size_t mp_bytes; int max_obs; int mp_capacity; int first_mp_slot; unsigned long long first_mp_id; int client_id;
    float scale[CORB_MAX_LEVELS]; int nlevels;
};
void corb_launch_newpoints_apply(const NpApplyDev& d, hipStream_t s);

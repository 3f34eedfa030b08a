// essgraph_internal.h -- Optimizer::OptimizeEssentialGraph on records (corb_essgraph.cpp, essgraph_kernels.hip; include/corb_essential_graph.h states the
// definition): the loop-edge sets, one call's device block and the launchers.
//
// Arithmetic: the Sim3 parts are FP64 in the operation order of sim3_math.h, which every kernel here goes through; the library is built with -ffp-contract=off and
// the few sums written out in essgraph_kernels.hip use __dmul_rn / __fma_rn only where a float product is exact in double (the rule of loopfix_internal.h), so
// nothing is contracted and numpy reproduces every bit (tests/essgraph_reference.py).
#pragma once
#include "covis_internal.h"
#include "graph_internal.h"
#include "corb_essential_graph.h"

#define ESS_LOOP_CAP CORB_COVIS_MAX_LOOP_EDGES

// mspLoopEdges of every slot, beside the rows and the tree
struct EssLoopSets {
    unsigned long long* id;                  // [capacity][ESS_LOOP_CAP] ascending
    int* n;                                  // [capacity]
};

// head[] of a plan: what the host reads back once
enum { ESS_H_VERTICES = 0, ESS_H_HELD = 1, ESS_H_KIND = 2, ESS_H_DROPPED = 6, ESS_H_LC_BELOW = 7, ESS_H_SUPPRESSED = 8, ESS_H_POSES = 14, ESS_H_MOVED = 15, ESS_H_KEPT = 16,
       ESS_H_SKIPPED = 17, ESS_H_FIXED_REF = 18, ESS_H_INTS = 20 };

struct EssPlanDev {
    int loop_slot, cur_slot, min_weight, n_pairs;
    const int* cpos;                         // [kf_capacity] position of the slot in corr_slots, or -1
    const double* corr; const double* ncorr; // [n_corr][8]
    const int* lc_i; const int* lc_j;        // [n_pairs] the loop connections flattened to (key, member) slots
    EssLoopSets loops;
    unsigned long long* key;                 // [kf_capacity] id of the keyframe the slot holds, COVIS_NO_ID for a slot that holds none
    unsigned char* bad;                      // [kf_capacity]
    int *hrank, *vrank;                      // [kf_capacity] position among the held keyframes / the vertices in ascending id, -1: none
    int *hslot, *vslot;                      // [kf_capacity] the inverse: held keyframes, vertices (v_slots)
    double *S, *snc; unsigned char* fixed;   // [kf_capacity][8], [kf_capacity]
    int* head;                               // [ESS_H_INTS]
    int *lc_flag, *lc_pos;                   // [n_pairs] 0 below the weight, 1 emitted, 2 dropped; edge index of an emitted pair
    unsigned long long* ins;                 // [n_pairs][2] sInsertedEdges as (lo, hi), ascending
    int* n_ins;                              // [1]
    int *cnt, *off;                          // [kf_capacity + 1] edges of the h-th held keyframe, their exclusive scan
    int* scan_scratch;
    // the fill's outputs (allocated once the counts are known)
    int *vi, *vj; unsigned char* kind; double* meas; int n_edges;
};

void ess_launch_loop_op(const EssLoopSets& L, const CovisStores& S, int op, int slot, int other, int* status, hipStream_t s);
// vertices (key, ranks, S / snc / fixed), loop connections (flags, positions, sInsertedEdges), per-keyframe edge counts and their scan: nothing but scratch is written
void ess_launch_count(const CovisRows& R, const CovisTree& T, const CovisStores& S, const EssPlanDev& d, hipStream_t s);
void ess_launch_fill(const CovisRows& R, const CovisTree& T, const CovisStores& S, const EssPlanDev& d, hipStream_t s);
// poses of the K vertices from the final estimates V, then the points (V0: the initial values); counts into d.head
void ess_launch_commit(const CovisStores& S, const EssPlanDev& d, int K, const double* V0, const double* V, int mp_first, int mp_n, float scale_factor, hipStream_t s);

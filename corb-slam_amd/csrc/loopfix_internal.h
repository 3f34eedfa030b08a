// loopfix_internal.h -- a loop event on the device (corb_loopfix.cpp, loopfix_kernels.hip): the map update that follows a global bundle adjustment and CorrectLoop's
// propagation; one call's scratch and the launchers
//
// Arithmetic convention of this file's kernels (tests/loopfix_reference.py states it again): every product of float matrices and vectors the reference makes on cv::Mat
// (Tchild*Twc, Tchildc*TcwGBA, Rcw*p, Rwc*Xc, Rwc*tcw) is computed per entry as rebase_records_kernel does -- the exact products summed in double, left to right, rounded
// to float once -- written with __dmul_rn / __fma_rn so that nothing is contracted; a product of two floats is exact in double, so the fused and the unfused sum round
// alike and numpy reproduces every bit.  `A*x + b` is that product followed by one float add (__fadd_rn).  KeyFrame::SetPose's Rwc = Rcw^T, Ow = -(Rwc*tcw) follow the
// same rule, and Twc is [Rwc | Ow] over the row 0 0 0 1.
#pragma once
#include "covis_internal.h"

#define LOOPFIX_UNSEEN 0x7F7F7F7F            // preset of the per-slot minimum arrays (hipMemset 0x7F): no queue position reaches it (corb_gba_propagate_store refuses such a queue_cap)

// what the walk and the point pass leave for the host; the first 28 bytes are CorbGbaPropagation
struct GbaHead { int n_popped, n_reached, n_propagated, n_revisited, n_points_set, n_points_moved, n_points_skipped; int status; };   // status 1: the walk needs more than queue_cap entries
struct GbaDev {
    float *Tcw, *GBA, *Bef;                  // [kf_capacity][16] GetPose(), mTcwGBA, mTcwBefGBA of every slot: the state the walk works on
    int* mark;                               // [kf_capacity] mnBAGlobalForKF == nLoopKF
    int *cnt, *off;                          // [kf_capacity] the held children of a slot: child[off .. off + cnt), ascending id
    int* child;                              // slots
    int* total;                              // [2] held children of all slots, the fill's cursor
    int* npop;                               // [kf_capacity] pops of the slot, zeroed
    int *winner, *first;                     // [kf_capacity] lowest queue position that lists the (unmarked) slot as a child / that pops the slot in this generation; preset LOOPFIX_UNSEEN
    int* queue; int queue_cap;               // lpKFtoCheck as slots: nothing is ever removed, the front is an index
    int n_origins;                           // queue[0 .. n_origins) on entry
    unsigned long long loop_kf;
    GbaHead* head;
};

// ---- CorrectLoop's propagation (corb_loop_correct_store) ----
// The g2o::Sim3 parts (G/types/sim3.h: the constructor from (R, t, s) through Eigen::Quaterniond(Matrix3d), operator*, inverse(), map(), rotation().toRotationMatrix())
// are FP64 in the reference's operation order (sim3_math.h); their results are rounded to float once.  Tic = Tiw*Twc is the float convention above.
#define LOOPFIX_SIM3_DOUBLES 24              // per member of the set: CorrectedSiw, NonCorrectedSiw, CorrectedSwi (8 doubles each: quaternion x y z w, t, s)
struct LcDev {
    const int* q_slots; const int* q_n;      // GetVectorCovisibleKeyFrames() of the current keyframe as corb_covis_query answers it
    const double* Scw;                       // [8] mg2oScw
    int cur_slot, cap; float scale_factor;
    int* set;                                // [max_connections + 1] the set in walk order (ascending keyframe id)
    int* count;                              // [2] members of the set, points corrected
    int* pos;                                // [kf_capacity] position of a slot in the walk, preset LOOPFIX_UNSEEN
    double* sim3;                            // [max_connections + 1][LOOPFIX_SIM3_DOUBLES]
    float* newT;                             // [max_connections + 1][16] the corrected pose [R | t/s]
    int* corrector;                          // [mp_capacity] lowest walk position of a member that holds the point, preset LOOPFIX_UNSEEN
};
size_t loopfix_set_lds_bytes(int M);
// the walk order and every member's Sim3s and corrected pose (one workgroup); nothing but scratch is written
void loopfix_launch_set(const CovisStores& S, int M, const LcDev& d, hipStream_t s);
// corrector (min-reduction per point), move (a thread per point: position, the two scratch fields, UpdateNormalAndDepth over the mixture of poses), then the poses.
// All three do nothing when the set is larger than d.cap
void loopfix_launch_correct(const CovisStores& S, int M, const LcDev& d, hipStream_t s);

void loopfix_launch_gather(const CovisTree& T, int M, const CovisStores& S, const float* bef, const GbaDev& d, hipStream_t s);
void loopfix_launch_fill(const CovisTree& T, int M, const CovisStores& S, const GbaDev& d, hipStream_t s);
void loopfix_launch_walk(const CovisStores& S, const GbaDev& d, hipStream_t s);
// both do nothing when the walk reported status != 0.  commit: Tcw, mTcwGBA, mnBAGlobalForKF into the records and mTcwBefGBA into the graph, for the slots the walk popped;
// points: one thread per slot of the map-point index
void loopfix_launch_commit(const CovisStores& S, float* bef, const GbaDev& d, hipStream_t s);
void loopfix_launch_points(const CovisStores& S, int mp_first, int mp_n, const GbaDev& d, hipStream_t s);

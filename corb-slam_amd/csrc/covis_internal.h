// covis_internal.h -- the covisibility graph on the device (corb_covis.cpp, covis_kernels.hip): row layout, staging of a batch, launchers
#pragma once
#include "corb_internal.h"
#include "store_internal.h"
#include "device_util.h"
#include "covis_math.h"

#define COVIS_T 256                          // threads of every workgroup here
#define COVIS_MAX_CONNECTIONS 1024           // a row is sorted in the LDS of one workgroup
#define COVIS_DEFAULT_CONNECTIONS 512
#define COVIS_UNSEEN 0x7F7F7F7F              // preset of the first-occurrence arrays (hipMemset 0x7F), as corb_idtab_insert_min's

// The graph: row r belongs to slot r of the keyframe store.  all_* is mConnectedKeyFrameWeights in descending (weight, id), ord_* is
// mvpOrderedConnectedKeyFrames / mvOrderedWeights as it stands (C/include/KeyFrame.h:291-293).
struct CovisRows {
    unsigned long long *all_id, *ord_id;     // [capacity][M]
    int *all_w, *ord_w;                      // [capacity][M]
    int *n_all, *n_ord;                      // [capacity]
    int M;
};
// The spanning tree beside the rows: mpParent / mbFirstConnection / mspChildrens of slot r (C/include/KeyFrame.h).  The set is kept in ascending id.
struct CovisTree {
    unsigned long long* parent;              // [capacity] an id, COVIS_NO_ID = none
    unsigned long long* child_id;            // [capacity][M]
    int *first, *n_child;                    // [capacity]
};
// the two stores as the kernels read them, with the per-call id -> slot table of the keyframes and the map-point store's index
struct CovisStores {
    const char* kf_base; size_t kf_bytes; int F, kf_capacity; CorbIdTable kfid;
    const char* mp_base; size_t mp_bytes; int O, mp_capacity; CorbIdTable mpid;
};
// what UpdateConnections computes from the records alone, per batch member (covis_count_kernel), before anything is committed
struct CovisStageHead { int n_all, n_ord, status, pad; unsigned long long first; };      // status 1: more than M distinct ids; first: front of the ordered list or COVIS_NO_ID
struct CovisStage {
    unsigned long long *all_id, *ord_id;     // [n][M]
    int *all_w, *ord_w, *ord_slot;           // [n][M]
    CovisStageHead* head;                    // [n]
};
struct CovisWindow {                         // device scratch of one corb_covis_local_window call
    int* kf_out; int kf_cap;                 // lLocalKeyFrames then lFixedCameras
    int* mp_out; int mp_cap;                 // lLocalMapPoints
    int* counts;                             // [4]: n_local, n_mp, n_fixed, covisibles met
    int* first_kf;                           // [kf_capacity]: -1 = carries mnBALocalForKF, else the first position an observation of it takes in the walk
    int* first_mp;                           // [mp_capacity]: the first position a feature holding the point takes in the walk
    int *flag, *pos;                         // [n_cand + 1] candidates of the running compaction
    int* scan_scratch;
    int local_bound, mp_bound;               // host-side bounds on n_local and n_mp (launch sizes)
};

size_t covis_lds_bytes(int M);
void covis_launch_count(const CovisStores& S, const int* slots, int n, int th, int M, const CovisStage& st, hipStream_t s);
void covis_launch_apply(const CovisRows& R, const CovisTree& T, const CovisStores& S, const CovisStage& st, int member, int slot, int n_ord, int* overflow, hipStream_t s);
void covis_launch_erase(const CovisRows& R, const CovisStores& S, int slot, hipStream_t s);
// mode 0: the in-store entries of the ordered list, the first N of them if N > 0; mode 1: GetCovisiblesByWeight(min_weight).  out_n[0] = entries written to out_slots / out_w ([M])
void covis_launch_query(const CovisRows& R, const CovisStores& S, int slot, int N, int min_weight, int mode, int* out_slots, int* out_w, int* out_n, hipStream_t s);
void covis_launch_weight(const CovisRows& R, const CovisStores& S, int slot_a, int slot_b, int* out_w, hipStream_t s);
void covis_launch_culling(const CovisStores& S, const int* list, const int* n_list, int max_list, int monocular, float th_depth, int* n_mps, int* n_red, unsigned char* cull, hipStream_t s);
void covis_launch_window(const CovisRows& R, const CovisStores& S, int slot, const CovisWindow& w, hipStream_t s);
// the compaction of the window's points alone (pass 0, 1, scan, 2) over w.kf_out[0 .. counts[0]): corb_track_update_local_map's UpdateLocalPoints has this structure
void covis_launch_window_points(const CovisStores& S, const CovisWindow& w, hipStream_t s);
// ---- the spanning tree (one workgroup each) ----
void covis_launch_tree_init(const CovisTree& T, int capacity, hipStream_t s);
// op 0: AddChild(other), 1: EraseChild(other), 2: ChangeParent(other) on `slot`; overflow[0] is set when a full set refuses an id
void covis_launch_tree_op(const CovisRows& R, const CovisTree& T, const CovisStores& S, int op, int slot, int other, int* overflow, hipStream_t s);
// the tree part of SetBadFlag: out[0] = ChangeParent calls, out[1] = the `if` of :658 was entered, out[2] = a full set refused an id
size_t covis_reparent_lds_bytes(int M);
void covis_launch_reparent(const CovisRows& R, const CovisTree& T, const CovisStores& S, int slot, int* out, hipStream_t s);

// traj_internal.h -- the camera trajectory on records (corb_trajectory.cpp, traj_kernels.hip): the object's device tables as the kernels see them, launchers
#pragma once
#include "corb_internal.h"
#include "store_internal.h"
#include "corb_trajectory.h"

#define TRAJ_T 256                           // threads of every workgroup here

// the front of the export block: what the kernels decide and leave for the one read-back
struct TrajHead {
    int status;                              // 1: no record can be the origin (an empty or out-of-range origin slot, or no held record without CORB_KF_BAD)
    int origin;                              // the origin's slot
    int n_rows;
    CorbTrajStats stats;
    float Two[16];                           // GetPoseInverse(origin)
};

// everything the object holds on the device, and the graph's store and parent field
struct TrajDev {
    const char* kf_base; size_t kf_bytes; int n_slots;                   // the graph's keyframe store
    const unsigned long long* parent;                                    // [n_slots] CovisTree::parent: an id, CORB_NO_ID = none
    CorbTrajEntry* entries; int capacity;                                // the log
    float* Tcp; double* time;                                            // [n_slots][16], [n_slots]
    // the store as plain arrays, gathered at the start of an export (traj_math.h's walk reads these)
    unsigned int* flags; int* held; unsigned long long* id; int* parent_slot; float* Tcw; float* Trw; int* chain;      // [n_slots] each ([n_slots][16] the poses)
    int* valid; int* pos; int* scan_scratch;                             // [capacity + 1] the running compaction of the rows
    TrajHead* head; float* rows; double* times; int* index;              // the export block: head | rows [N][12] | times [N] | index [N] (ids [N] for the keyframes), N = max(capacity, n_slots)
    int* status;                                                         // one int for set_bad_pose
};

// kind 0: the caller's Tcr; 1: Tcr from the records cur and ref; 2: a copy of entry n - 1.  Writes entry n (one workgroup)
void traj_launch_append(const TrajDev& d, int kind, int n, const char* cur, int ref_slot, const float* Tcr, double timestamp, int lost, hipStream_t s);
// Tcp(slot) = Tcw(slot) * GetPoseInverse(parent) (one workgroup); status[0] = 1 and nothing written without a held parent or with an empty slot
void traj_launch_set_bad_pose(const TrajDev& d, int slot, hipStream_t s);
// the whole export of the frames: gather, origin (origin_slot = -1: the min-reduction over ids), walk, validity, scan, rows into the block
void traj_launch_frames(const TrajDev& d, int n_entries, int origin_slot, int format, hipStream_t s);
// the keyframes' rows in ascending id into the block
void traj_launch_keyframes(const TrajDev& d, hipStream_t s);

// localmap_internal.h -- Tracking::UpdateLocalMap on the device (corb_localmap.cpp, localmap_kernels.hip): one call's device scratch and the launchers
#pragma once
#include "covis_internal.h"

#define LOCALMAP_MAX_KFS 80                  // `if(mvpLocalKeyFrames.size()>80) break;` (C/src/Tracking.cc:1313)
#define LOCALMAP_NEIGHBOURS 10               // GetBestCovisibilityKeyFrames(10) (:1318)

// what the vote-and-walk kernel leaves for the host; the first 32 bytes are CorbLocalMap
struct LocalMapHead {
    int n_kf, n_voted, n_mp, ref_slot; unsigned long long ref_id; int counter_empty, n_cleared;
    int status, fail;                        // status 1: more than max_connections distinct voters; fail 1: a list is longer than its cap (set by the finish kernel)
};
struct LocalMapDev {
    char* frame_rec; int F_frame;            // the current frame's record and its store's feature capacity
    const int* prev; int n_prev;             // mvpLocalKeyFrames before the call
    int* votes;                              // [kf_capacity] keyframeCounter by slot, zeroed
    int* mark;                               // [kf_capacity] mnTrackReferenceForFrame == mCurrentFrame.mnId, zeroed
    int* kf_out; int list_cap;               // mvpLocalKeyFrames; list_cap >= max(max_connections, 83, n_prev): no walk can overrun it
    int* mp_out; unsigned long long* mp_ids; // mvpLocalMapPoints as slots and as ids
    int kf_cap, mp_cap;                      // the caller's caps
    int* counts;                             // the CovisWindow's counts: [0] local keyframes, [1] local points
    LocalMapHead* head;
};

size_t localmap_lds_bytes(int M);
void localmap_launch_vote_walk(const CovisRows& R, const CovisTree& T, const CovisStores& S, const LocalMapDev& d, hipStream_t s);
// after the points' compaction: the caps' verdict, the points' ids, and -- only if the call succeeds -- the frame record's bad points cleared (:1278)
void localmap_launch_finish(const CovisStores& S, const LocalMapDev& d, int n_threads, hipStream_t s);

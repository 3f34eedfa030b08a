// tracklocal_internal.h -- Tracking::TrackLocalMap on records (corb_tracklocal.cpp, tracklocal_kernels.hip): what the chain adds to the kernels of
// UpdateLocalMap (localmap_internal.h), SearchLocalPoints / PoseOptimization (track_internal.h) and the matcher (proj_internal.h)
#pragma once
#include "track_internal.h"
#include "localmap_internal.h"
#include "corb_track_local_map.h"

struct TrackLocalMapDev {
    TrackLocalDev v;                         // the frame, the map as read, the camera and the matcher's views; v.ids unused, v.n_local = the launch bound of the list
    char* map;                               // the map's records, written: counters and scratch
    int max_obs;                             // MpLayout(max_obs).scratch
    const int* list;                         // mvpLocalMapPoints as slots (LocalMapDev::mp_out), head->n_mp of them
    const LocalMapHead* head;                // of the chain's UpdateLocalMap; NULL (corb_track_local_map_stats): no earlier step
    unsigned long long frame_id;
    int sensor, only_tracking;
    int* n_inliers;                          // [1] mnMatchesInliers, zeroed
    // the tail also packs the result block of the chain (all optional)
    const int* proj_counts; int* out_counts; // [3] n_in_view | n_matches | status of the matcher -> the block
    int* out_match;                          // [n_cur] <- v.match
    const unsigned char* rejected; unsigned char* out_outlier;       // [n_cur] mvbOutlier of this PoseOptimization -> the block
};
// SearchLocalPoints' two passes (Tracking.cc:1168-1204) with the records' counters and scratch: the frame's features, then the list by slot.  With head->status or
// head->fail set they write the scratch of the matcher only (no claims, no valid query), no record
void tracklocal_launch_prepare(const TrackLocalMapDev& t, hipStream_t s);
// F.mvpMapPoints[f] = vpMapPoints[match[f]] (ORBmatcher.cc:122), the id taken from the record list[match[f]]
void tracklocal_launch_scatter(const TrackLocalMapDev& t, hipStream_t s);
// Tracking.cc:960-978 on the record PoseOptimization left, and the packing of the result block
void tracklocal_launch_tail(const TrackLocalMapDev& t, hipStream_t s);

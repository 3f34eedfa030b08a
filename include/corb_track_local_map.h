/* corb_track_local_map.h -- Tracking::TrackLocalMap on records: search, pose and the points' counters in one call (exported from libcorb_accel.so beside
 * corb_accel.h).
 *
 * bool Tracking::TrackLocalMap() (C/src/Tracking.cc:951-992) runs once per tracked frame: UpdateLocalMap, SearchLocalPoints, Optimizer::PoseOptimization, then the
 * tail that counts the inliers, tells the MapPoints they were found and decides whether tracking goes on.  corb_accel.h has the first three as separate calls
 * (corb_track_update_local_map, corb_track_search_local_points, corb_track_pose_optimization): three synchronisations, the local points read back as ids only to be
 * uploaded again.  Here the list stays on the device as slots, the whole function is one call with one read-back, and the map-point records receive what the
 * reference writes into its MapPoints: mnVisible, mnFound (CorbMapPointCounters) and mnLastFrameSeen, mbTrackInView, mTrackProj*, mnTrackScaleLevel, mTrackViewCos
 * (CorbMapPointScratch).  Every output equals, byte for byte, what the three calls leave when they are made one after the other, with the tail applied.
 * No existing struct changes: CORB_ABI_VERSION stays as corb_accel.h states it. */
#ifndef CORB_TRACK_LOCAL_MAP_H
#define CORB_TRACK_LOCAL_MAP_H
#include "corb_accel.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct CorbTrackLocalMapParams {
    uint64_t frame_id;             /* mCurrentFrame.mnId: what mnLastFrameSeen receives */
    uint64_t last_reloc_frame_id;  /* mnLastRelocFrameId */
    int32_t  max_frames;           /* mMaxFrames */
    int32_t  sensor;               /* 0 MONOCULAR, 1 STEREO, 2 RGBD (System::eSensor) */
    int32_t  only_tracking;        /* mbOnlyTracking */
    float    log_scale_factor;     /* mfLogScaleFactor */
    float    nnratio;              /* 0.8 in the reference */
    float    th;                   /* 0: the reference's rule (:1208-1213): 1, RGBD 3, frame_id < last_reloc_frame_id + 2 -> 5; > 0: this value */
} CorbTrackLocalMapParams;
typedef struct CorbTrackLocalMapResult {
    CorbLocalMap local;            /* exactly what corb_track_update_local_map reports */
    int32_t n_in_view, n_matches;  /* nToMatch, SearchByProjection's return */
    int32_t n_pose_inliers;        /* PoseOptimization's return */
    int32_t n_matches_inliers;     /* mnMatchesInliers */
    int32_t ok;                    /* TrackLocalMap's return */
    float   th_used;
    float   Tcw[16];               /* the pose PoseOptimization left (Tcw_in passed through where it leaves none) */
} CorbTrackLocalMapResult;

/* The frame is record `slot` of `frames` (the graph's keyframe store or another one), the map is the graph's map-point store; cam, Tcw_in as
 * corb_track_pose_optimization takes them (Tcw_in is also the pose SearchLocalPoints projects with).  In the reference's order:
 *   UpdateLocalMap     corb_track_update_local_map in every word of its comment (ascending-id walks, a feature whose point resolves to a bad record loses it, the caps);
 *                      prev_kf_slots / kf_slots / mp_slots / mp_ids / the caps are its arguments, out->local its CorbLocalMap
 *   SearchLocalPoints  corb_track_search_local_points over that list, addressed by slot.  The frame's own points are the ones its features' ids resolve to, the ids that
 *                      discarded features keep included.  Every feature whose point resolves, is not bad and is not discarded: n_visible += 1 (once per feature),
 *                      last_frame_seen = frame_id, track_in_view = 0 (:1182-1184).  Every list point that is neither one of those nor bad goes through
 *                      Frame::isInFrustum(pMP, 0.5): track_in_view = 0 on each early return; on success track_in_view = 1, track_proj_x / _y / _xr, track_scale_level,
 *                      track_view_cos written and n_visible += 1 (Frame.cc:272, :321-326; Tracking.cc:1201).  Then SearchByProjection(frame, list, th) with nnratio;
 *                      match[i] = index into the list of the point feature i received, or -1
 *   PoseOptimization   corb_track_pose_optimization(discard_outliers = 0) from Tcw_in; outlier[i] = mvbOutlier[i]
 *   the tail           every feature that holds a point whose id resolves (:960-978): not an outlier -> n_found += 1, and it counts toward n_matches_inliers when
 *                      only_tracking is set or the record's n_obs > 0; an outlier with sensor == 1 loses its point (the id becomes CORB_NO_MAP_POINT, the outlier flag
 *                      stays, as mvbOutlier does).  ok = !(frame_id < last_reloc_frame_id + max_frames && n_matches_inliers < 50) && n_matches_inliers >= 30 (:983-990)
 * The counters are integer sums on the records, the rest is written by one thread each or with one value: no output depends on the order the device's atomics land in.
 * CORB_ERR_CAPACITY as corb_track_update_local_map.  CORB_ERR_ARG: an empty slot as the frame or among prev_kf_slots, no map-point index, stores on different
 * devices, a bad camera, sensor outside 0..2, log_scale_factor <= 0, mp_cap > 60000, a frame of more than 6000 features (the matcher's limits).  After either, no
 * byte of any record has changed, counters and scratch included, and no caller array is written.  CORB_ERR_OVERFLOW: a search window held more than 256 candidates,
 * as corb_track_search_local_points reports it; the records have been written by then.
 * match and outlier are optional ([n(slot)] each).  mp_cap bounds the search's launches and 12 bytes per point of it are read back whatever the list holds: size it
 * for a local map.  One host synchronisation and one read-back per call.  Locks: the graph, then each store once, as corb_track_update_local_map takes them. */
int corb_track_local_map(CorbCovis* g, CorbKfStore* frames, int slot, const CorbTrackCamera* cam, const float* Tcw_in /* 16 */,
                         const int32_t* prev_kf_slots, int n_prev, const CorbTrackLocalMapParams* params,
                         int32_t* kf_slots, int kf_cap, int32_t* mp_slots, uint64_t* mp_ids, int mp_cap,
                         int32_t* match, uint8_t* outlier,
                         CorbTrackLocalMapResult* out);

/* The tail of TrackLocalMap alone (the same kernel), on a record that corb_track_pose_optimization(discard_outliers = 0) has left: for callers that keep the separate
 * calls, and for the relocalisation path, which runs TrackLocalMap after a pose of its own.  CORB_ERR_ARG with nothing written: an empty slot, no map-point index,
 * stores on different devices, sensor outside 0..2. */
int corb_track_local_map_stats(CorbKfStore* frames, int slot, CorbMpStore* map, int sensor, int only_tracking,
                               uint64_t frame_id, uint64_t last_reloc_frame_id, int max_frames,
                               int32_t* n_matches_inliers, int* ok);

#ifdef __cplusplus
}
#endif
#endif

/* corb_track_frame.h -- the initial pose of a tracked frame on records in one call: Tracking::TrackWithMotionModel and Tracking::TrackReferenceKeyFrame, and the two
 * per-feature loops at the end of Tracking::Track (exported from libcorb_accel.so beside corb_accel.h).
 *
 * bool Tracking::TrackWithMotionModel() (C/src/Tracking.cc:886-949) and bool Tracking::TrackReferenceKeyFrame() (:775-817) are short chains whose branch points are
 * integer counts: "fewer than 20 matches -> search again at twice the window", "fewer than 20 / 15 -> return false".  corb_accel.h has their steps as separate calls
 * (corb_track_search_last_frame, corb_search_by_bow_slots, corb_track_pose_optimization) with a read-back and a host decision between them, and leaves nmatchesMap,
 * UpdateLastFrame's pose and CheckReplacedInLastFrame to the host, which has to fetch what they read.  Here each function is one call with one synchronisation and
 * one read-back: the counts are read and the decisions taken on the device.  With corb_track_local_map (corb_track_local_map.h) a tracked frame is two calls.
 * Every output equals, byte for byte, what the separate calls leave when they are made one after the other with the host steps between them.
 * No existing struct changes: CORB_ABI_VERSION stays as corb_accel.h states it. */
#ifndef CORB_TRACK_FRAME_H
#define CORB_TRACK_FRAME_H
#include "corb_accel.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct CorbTrackFrameParams {
    uint64_t frame_id;             /* mCurrentFrame.mnId: what mnLastFrameSeen of a discarded outlier's point receives (:933, :809) */
    int32_t  sensor;               /* 0 MONOCULAR, 1 STEREO, 2 RGBD (System::eSensor): th's rule, and bMono of SearchByProjection */
    int32_t  only_tracking;        /* mbOnlyTracking (:942-946); TrackReferenceKeyFrame does not read it */
    int32_t  check_replaced;       /* run CheckReplacedInLastFrame first (:754-772, called at :304) */
    int32_t  check_orientation;    /* ORBmatcher's mbCheckOrientation (true in the reference) */
    float    nnratio;              /* 0.9 in TrackWithMotionModel (:888), 0.7 in TrackReferenceKeyFrame (:782) */
    float    th;                   /* TrackWithMotionModel: 0 = the reference's rule (:899-903): 7 for STEREO, 15 otherwise; > 0: this value.  TrackReferenceKeyFrame: unused */
} CorbTrackFrameParams;
typedef struct CorbTrackFrameResult {
    int32_t n_matches_first;       /* SearchByProjection at th (:905); TrackReferenceKeyFrame: SearchByBoW's return (:785) */
    int32_t searched_wide;         /* the search at 2 th ran (:907-911) */
    int32_t n_matches;             /* of the search that counts */
    float   th_used;               /* th, or 2 th when searched_wide */
    int32_t n_pose_inliers;        /* PoseOptimization's return (0 when it did not run) */
    int32_t n_matches_kept;        /* nmatches after the "Discard outliers" loop */
    int32_t n_matches_map;         /* nmatchesMap */
    int32_t vo;                    /* mbVO as :944 sets it (0 unless only_tracking) */
    int32_t ok;                    /* the function's return */
    float   Tlw[16];               /* mLastFrame.mTcw as the call left it */
    float   Tcw_pred[16];          /* the pose the search and the optimisation started from: mVelocity*mLastFrame.mTcw (:894), mLastFrame.mTcw (:791) */
    float   Tcw[16];               /* mCurrentFrame.mTcw as the call left it */
} CorbTrackFrameResult;

/* bool Tracking::TrackWithMotionModel() for the frame in record cur_slot of `frames`, the last frame in record last_slot of the same store, mLastFrame.mpReferenceKF
 * in record ref_slot of `kfs` (that store or another one on the device), the map-point store `map` with a current id index, cam as corb_track_pose_optimization takes
 * it.  In the reference's order:
 *   CheckReplacedInLastFrame  when params->check_replaced: every feature of the last record whose held id (a discarded feature holds none) resolves to a record
 *                      with replaced_by != 0 (CorbMapPointCounters) receives the id replaced_by - 1 -- one step, not followed further, whether or not the new id
 *                      resolves; an id that does not resolve stays
 *   UpdateLastFrame    when Tlr is given (:822-825): Tlw = Tlr * Tcw(ref record) is written into the last record's Tcw.  Tlr = NULL: the last record's pose stands as
 *                      it is.  The creation of the "visual odometry" points (:827-883) stays with corb_kfi_create_stereo_points(mode 2): a caller that needs it runs
 *                      it after this pose is known -- it writes the pose itself from the same product -- and then passes Tlr = NULL
 *   SetPose            Tcw_pred = velocity * Tlw into the current record's Tcw (:894); it stays there whatever the call returns.  Both products are cv::gemm on CV_32F
 *                      as proj_host.h states it: every element a double sum over k ascending, rounded to float once, the bottom row the product's, computed on the
 *                      device from the records (csrc/trackframe_math.h)
 *   fill               every feature of the current record: id CORB_NO_MAP_POINT, CORB_FEATURE_OUTLIER and CORB_FEATURE_DISCARDED cleared (:896)
 *   SearchByProjection corb_track_search_last_frame(Tcw_pred, Tlw, th, mono = sensor == 0, nnratio, check_orientation) on the same kernels; fewer than 20 matches: the
 *                      fill again and the search at 2 th (:907-911), decided on the device; the kernels of the wide search return at once when it is not taken
 *   fewer than 20      ok = 0: the frame keeps the matches the last search left and Tcw_pred; no flag and no map-point byte has changed (:913)
 *   PoseOptimization   corb_track_pose_optimization(discard_outliers = 1) from Tcw_pred
 *   Discard outliers   (:919-940) n_matches_kept = n_matches - the rejected features; every rejected feature's point: track_in_view = 0, last_frame_seen = frame_id
 *                      (CorbMapPointScratch; two features of one point write the same values) -- CORB_FEATURE_DISCARDED is set as corb_track_pose_optimization sets
 *                      it; n_matches_map = the features that hold a point whose id resolves and whose record has n_obs > 0
 *   return             ok = n_matches_map >= 10; with only_tracking: vo = n_matches_map < 10, ok = n_matches_kept > 20 (:942-948)
 * match[i] (optional, n(cur_slot) entries) = the feature of the last frame feature i took its point from, or -1; outlier[i] (optional) = 1 for the features the
 * optimisation rejected.  A current or a last record of no features: CORB_OK with ok = 0, the poses written, nothing else.
 * CORB_ERR_ARG: an empty slot, no map-point index, stores on different devices, a bad camera, sensor outside 0..2, a frame above the matcher's limits (6000
 * features); no byte of any record has changed and no caller array is written.  CORB_ERR_OVERFLOW: a search window held more than 256 candidates, as
 * corb_track_search_last_frame reports it, for the first search and for the wide one when it ran; the records have been written by then.
 * One host synchronisation and one read-back per call.  Locks: each store once, as corb_track_local_map_stats takes them. */
int corb_track_with_motion_model(CorbKfStore* frames, int cur_slot, int last_slot, CorbKfStore* kfs, int ref_slot, CorbMpStore* map, const CorbTrackCamera* cam,
                                 const float* velocity /* 16 */, const float* Tlr /* 16 or NULL */, const CorbTrackFrameParams* params,
                                 int32_t* match, uint8_t* outlier, CorbTrackFrameResult* out);

/* bool Tracking::TrackReferenceKeyFrame() for the same records; pKF = mpReferenceKF is record ref_slot of `kfs`.
 *   ComputeBoW         (:778) voc given and the current record holds no FeatureVector: computed first exactly as corb_kf_store_compute_bow(frames, &cur_slot, 1, voc, 4,
 *                      NULL, NULL) leaves it.  voc = NULL: the record must hold one, else CORB_ERR_ARG.  A keyframe record without one shares no node: no match
 *   SearchByBoW        (:785) corb_search_by_bow_slots variant 0 for the pair (ref_slot, cur_slot) with nnratio and check_orientation; the common vocabulary nodes are
 *                      found on the device.  A keyframe feature takes part iff its id resolves to a record of `map` that is not bad (if(!pMP) continue;
 *                      if(pMP->isBad()) continue, ORBmatcher.cc:195-200), evaluated here: the record's CORB_FEATURE_HAS_MP byte is neither read nor written
 *   fewer than 15      ok = 0: the frame keeps its ids, flags and pose; only the FeatureVector may have been added (:787-788)
 *   otherwise          mvpMapPoints = vpMapPointMatches (:790): every feature is written, matched ones with the keyframe record's id, the rest CORB_NO_MAP_POINT,
 *                      CORB_FEATURE_OUTLIER / _DISCARDED cleared; SetPose(mLastFrame.mTcw) (:791): Tcw of the last record as it stands; PoseOptimization, the
 *                      discard loop and the scratch writes as above (:793-814); ok = n_matches_map >= 10 (:816)
 * match[i] = the keyframe's feature that feature i was matched to, or -1.  n_matches_first = n_matches = SearchByBoW's return; searched_wide = 0, th_used = 0.
 * CORB_ERR_ARG as above, and for a record without a FeatureVector where one is needed, a vocabulary on another device, a record above 8192 features.
 * One host synchronisation and one read-back per call. */
int corb_track_reference_keyframe(CorbKfStore* frames, int cur_slot, int last_slot, CorbKfStore* kfs, int ref_slot, CorbMpStore* map, const CorbTrackCamera* cam,
                                  CorbVoc* voc, const CorbTrackFrameParams* params, int32_t* match, uint8_t* outlier, CorbTrackFrameResult* out);

/* The two per-feature loops at the end of Tracking::Track; NeedNewKeyFrame / CreateNewKeyFrame run between them, so two stages.
 *   stage 0  "Clean VO matches" (:438-447): a feature whose held id resolves to a record with n_obs < 1 loses it: the id becomes CORB_NO_MAP_POINT and
 *            CORB_FEATURE_OUTLIER is cleared.  Ids that do not resolve and discarded features are untouched.  Asynchronous on the frame store's stream; nothing is
 *            read back; Tcr_out is not written (it may be NULL)
 *   stage 1  (:463-467) a feature whose held id resolves and that carries CORB_FEATURE_OUTLIER loses the id; the flag stays, as mvbOutlier does.  (:491) Tcr_out =
 *            Tcw(cur record) * GetPoseInverse(ref record): the entry of mlRelativeFramePoses, which the next frame passes as Tlr.  Twc = [Rcw^T | Ow] with
 *            camera_centre's rule (proj_host.h) and the bottom row 0 0 0 1, the product as above.  One read-back of 64 bytes
 * CORB_ERR_ARG with nothing written: an empty slot, no map-point index, stores on different devices, a stage other than 0 / 1, stage 1 without Tcr_out. */
int corb_track_frame_finish(CorbKfStore* frames, int cur_slot, CorbKfStore* kfs, int ref_slot, CorbMpStore* map, int stage, float* Tcr_out /* 16 */);

#ifdef __cplusplus
}
#endif
#endif

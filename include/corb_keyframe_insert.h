/* corb_keyframe_insert.h -- the moment a tracked frame becomes a keyframe, on device-resident records: the stereo / RGB-D points of Tracking::CreateNewKeyFrame,
 * StereoInitialization and UpdateLastFrame, the per-feature counts of Tracking::NeedNewKeyFrame, the association loop of LocalMapping::ProcessNewKeyFrame and LocalMapping::MapPointCulling.  Exported from libcorb_accel.so
 * beside the drop-in boundary of corb_accel.h (reference paths are relative to corbslam_client/src/).
 *
 * The calls take no workspace lane.  Their temporaries belong to a handle, CorbKfInsert, created once per client: it owns its device scratch, a page-locked staging
 * block and one stream.  Every buffer of the handle is written by a call before that call reads it, so a call's outputs do not depend on what the handle served
 * before (WORKSPACE_AUDIT.md).  A handle serves one call at a time (it locks itself).
 *
 * House rules as for the other calls on records: argument errors are a status with a message in corb_last_error(); the handle, then the keyframe store(s) by
 * address, then the map-point store are locked before a feature count is read; one synchronisation and one read-back per call; the decisions are computed from the
 * records as they stand before the call, so apply == 0 reports exactly what apply != 0 does; on CORB_ERR_CAPACITY nothing is written and the outputs are complete.
 * The definition of every output and every record byte is tests/kfinsert_reference.py. */
#ifndef CORB_KEYFRAME_INSERT_H
#define CORB_KEYFRAME_INSERT_H
#include "corb_accel.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CORB_KFI_MAX_FEATURES 4096      /* the (depth, index) keys of one frame are sorted in the local memory of one workgroup: 32 KiB of keys */

typedef struct CorbKfInsert CorbKfInsert;
/* max_features: the largest feature count of a record the handle is given (1 .. CORB_KFI_MAX_FEATURES; a store with more features per record is refused by the
 * calls); max_recent: the longest recent-point list of corb_kfi_map_point_culling (>= 0). */
int corb_kfi_create(int device, int max_features, int max_recent, CorbKfInsert** out);
void corb_kfi_destroy(CorbKfInsert* h);

/* The stereo-point creation of the tracking thread on record `slot` of `kf` (Tcw and id from its meta; mvKeysUn, mvuRight, mvDepth, descriptors and MapPoint ids
 * from its features).  cam: fx, fy, cx, cy, nlevels and scale (mvScaleFactors).
 *   mode 0  StereoInitialization (Tracking.cc:524-540): every feature with z > 0 in feature order; the ids the features hold are ignored and overwritten
 *   mode 1  CreateNewKeyFrame (:1103-1156): the features with z > 0 ascending in (z, i) -- std::sort on pair<float,int> -- are visited up to and including the first
 *           entry j >= 100 with z_j > th_depth (nPoints counts every visited entry and is tested after the increment: 101 entries at least, all if there is no such j)
 *   mode 2  UpdateLastFrame (:830-883): the same visit rule on the last frame's record; the points are the temporal ones of MapPoint(x3D, cacher, pFrame, idxF)
 * kind[j] of visited entry j (modes 1, 2; mode 0 gives 1 throughout): 1 created, the feature holds CORB_NO_MAP_POINT; 2 created, the held id resolves through the
 * map's id index (corb_mp_store_build_index; needed for modes 1, 2) to a record with n_obs < 1; 0 left alone, the record has observations; 3 left alone, the id
 * resolves to no record (a temporal point the store never saw).
 * The k-th created point in visit order is record first_mp_slot + k with id first_mp_id + k, world_pos = Frame::UnprojectStereo (Frame.cc:670-684) in the arithmetic
 * of corb_create_new_map_points_store.  Modes 0 / 1 (MapPoint(x3D, pKF, cacher) + AddObservation + ComputeDistinctiveDescriptors + UpdateNormalAndDepth, :1137-1141):
 * ref_kf_id = the keyframe's id, the one observation (id, i), flags 0, the feature's descriptor, normal / min_distance / max_distance of that observation in
 * corb_local_ba_store's UpdateNormalAndDepth arithmetic with cam->scale, counters n_visible = n_found = 1, scratch first_kf_id = the keyframe's id, first_frame =
 * frame_id, n_obs_weight = 2 if mvuRight[i] >= 0 else 1.  Mode 2: ref_kf_id 0 (no keyframe), no observation, normal and distances from the frame's own camera centre
 * and the feature's octave (MapPoint.cc:69-80), counters 1 / 1, scratch first_kf_id = -1, first_frame = frame_id, track_in_view = 1.  Everything else in the
 * record is zero.  Feature i of the record gets the new id and its has-a-map-point flag; with `mirror` (optional: a second record, in `kf` or in another store on
 * the same device, with at least as many features) the same feature there gets the same id and flag -- mCurrentFrame.mvpMapPoints[i] = pNewMP.
 * order[j] = feature index and kind[j] per visited entry, x3d[3k ..] per created point (room for n(slot) entries each); *n_visited, *n_created.  Fewer free records
 * than *n_created from first_mp_slot on: CORB_ERR_CAPACITY, no record written.  corb_mp_store_build_index again afterwards. */
int corb_kfi_create_stereo_points(CorbKfInsert* h, CorbKfStore* kf, int slot, CorbMpStore* map, const CorbTrackCamera* cam, float th_depth, int mode, int apply,
                                  int first_mp_slot, uint64_t first_mp_id, int32_t client_id, int64_t frame_id, CorbKfStore* mirror, int mirror_slot,
                                  int32_t* order, uint8_t* kind, float* x3d, int* n_visited, int* n_created);

/* The counts Tracking::NeedNewKeyFrame takes from per-feature data (the scalar decision, :1038-1080, stays with the caller).
 * On record cur_slot of `frames` (:1026-1035): among the features with 0 < z < th_depth, *n_tracked_close = those that hold an id the map's index resolves and whose
 * outlier bit (record flag bit 1) is clear, *n_non_tracked_close = the others.
 * On record ref_slot of `kf` (ref_slot < 0: skipped, *n_ref_matches = 0): *n_ref_matches = pKF->TrackedMapPoints(min_obs) -- features whose point resolves, is not
 * bad and, if min_obs > 0, has Observations() >= min_obs.  Observations() is the reference's weighted nObs, computed from the record's list by corb_local_ba_store's
 * rule: an observation (kf id, idx) counts 2 if that keyframe is among the slots [kf_first, kf_first + kf_n) of `kf` (looked up by id as corb_mp_store_replace does)
 * and its mvuRight[idx] >= 0, else 1.  scratch.n_obs_weight is not read.  No record changes. */
int corb_kfi_need_keyframe_counts(CorbKfInsert* h, CorbKfStore* frames, int cur_slot, CorbMpStore* map, float th_depth, CorbKfStore* kf, int ref_slot, int min_obs,
                                  int kf_first, int kf_n, int* n_tracked_close, int* n_non_tracked_close, int* n_ref_matches);

/* The association loop of LocalMapping::ProcessNewKeyFrame (LocalMapping.cc:132-151) for record `slot` of `kf` (Frame::ComputeBoW is corb_kf_store_compute_bow,
 * UpdateConnections is corb_covis_update).  kind[i] per feature: 0 no id; 1 the point is bad; 2 the id resolves to no record of the map's index (skipped, as a
 * getMapPoint() that returns NULL is); 3 the observation was added; 4 the point observes this keyframe already and enters the recent list (:145-148).  The serial loop
 * in closed form: of several features that hold one point which does not observe the keyframe yet, the LOWEST index is kind 3 and the others are kind 4, because
 * IsInKeyFrame is true by the time the loop reaches them.
 * apply != 0, per kind 3: the observation (keyframe id, i) enters the point's list at its place in ascending keyframe id (as corb_fuse_store action 1);
 * MapPoint::UpdateNormalAndDepth over the observations whose keyframes are among the slots [kf_first, kf_first + kf_n) of `kf` (found by id as corb_mp_store_replace
 * finds them; corb_local_ba_store's arithmetic, mvScaleFactors rebuilt from scale_factor); MapPoint::ComputeDistinctiveDescriptors over the observations in non-bad
 * keyframes of those slots (the rule and selection of corb_mp_store_replace).  mpRefKF, the counters and the scratch are untouched.
 * kind[n(slot)]; recent_slots = the map-point slots of kind 4 in feature order, duplicates included (room for n(slot)); *n_added, *n_recent.  A kind-3 point whose
 * list is full: CORB_ERR_CAPACITY, nothing written.  At most 1024 observations per map point. */
int corb_kfi_process_new_keyframe(CorbKfInsert* h, CorbKfStore* kf, int slot, CorbMpStore* map, int kf_first, int kf_n, float scale_factor, int apply,
                                  uint8_t* kind, int32_t* recent_slots, int* n_added, int* n_recent);

/* LocalMapping::MapPointCulling (LocalMapping.cc:161-188) over mlpRecentAddedMapPoints = recent_slots[n] (slots of `map`).  decision[i], tested in this order as the
 * else-if chain does: 1 dropped, already bad; 2 culled, (float)n_found / n_visible < 0.25f (0 / 0 is NaN and does not cull); 3 culled, (int)cur_kf_id -
 * (int)first_kf_id >= 2 and Observations() <= th_obs (2 monocular, 3 otherwise; Observations() as above); 4 dropped from the list, the difference is >= 3; 0 stays.
 * A slot named more than once: its first occurrence decides; a later one reports 1 if the first culled (2 or 3) and repeats the first's decision otherwise.
 * apply != 0: decisions 2 and 3 do MapPoint::SetBadFlag (MapPoint.cc:255-269) as corb_local_ba_store does on records: CORB_MP_BAD, n_obs = 0, the list cleared, and in
 * every observing keyframe among the named slots feature idx <- CORB_NO_MAP_POINT with its has-a-map-point flag cleared (EraseMapPointMatch).
 * kept_slots = the decision-0 entries in order (room for n); *n_kept; *n_culled = entries with decision 2 or 3. */
int corb_kfi_map_point_culling(CorbKfInsert* h, CorbMpStore* map, const int32_t* recent_slots, int n, uint64_t cur_kf_id, int th_obs, CorbKfStore* kf, int kf_first,
                               int kf_n, int apply, uint8_t* decision, int32_t* kept_slots, int* n_kept, int* n_culled);

#ifdef __cplusplus
}
#endif
#endif

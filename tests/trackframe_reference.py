"""Definition, in plain Python / numpy, of what the calls of include/corb_track_frame.h leave behind: bool Tracking::TrackWithMotionModel()
(corbslam_client/src/Tracking.cc:886-949), bool Tracking::TrackReferenceKeyFrame() (:775-817), CheckReplacedInLastFrame (:754-772), UpdateLastFrame's pose
(:822-825) and the two per-feature loops at the end of Tracking::Track (:438-447, :463-467, :491), as bookkeeping over the outputs of the separate calls.

The searches and the optimisation themselves are not redone here: the matches (corb_track_search_last_frame, corb_search_by_bow_slots) and the rejected set
(corb_track_pose_optimization, discard_outliers = 1) come from those calls.  This module states what lies between and after them: the 4x4 products, the replaced
ids, the retry rule, the tail's counts, flags and scratch writes, setMapPointMatches, and both finish stages."""
import copy

import numpy as np

NO_MAP_POINT = 0xFFFFFFFFFFFFFFFF
MP_BAD = 1                  # CORB_MP_BAD
FEATURE_HAS_MP = 1          # CORB_FEATURE_HAS_MP
FEATURE_OUTLIER = 2         # CORB_FEATURE_OUTLIER
FEATURE_DISCARDED = 4       # CORB_FEATURE_DISCARDED
MONOCULAR, STEREO, RGBD = 0, 1, 2
MIN_MATCHES_MOTION, MIN_MATCHES_REFERENCE, MIN_MATCHES_MAP, MIN_KEPT_ONLY_TRACKING = 20, 15, 10, 20


# ---- poses: cv::gemm on CV_32F = every element a double sum over k ascending, rounded to float once; the bottom row comes out of the product ----
def gemm4(A, B):
    A = np.asarray(A, np.float32).reshape(4, 4); B = np.asarray(B, np.float32).reshape(4, 4)
    C = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            s = np.float64(0.0)
            for k in range(4):
                s = s + np.float64(A[i, k]) * np.float64(B[k, j])
            C[i, j] = np.float32(s)
    return C


def camera_centre(Tcw):
    """Ow = -Rcw^T tcw: the transposed rotation negated exactly, a double sum over k ascending, one rounding (proj_host.h)"""
    T = np.asarray(Tcw, np.float32).reshape(4, 4)
    Ow = np.zeros(3, np.float32)
    for i in range(3):
        s = np.float64(0.0)
        for k in range(3):
            s = s + np.float64(-T[k, i]) * np.float64(T[k, 3])
        Ow[i] = np.float32(s)
    return Ow


def pose_inverse(Tcw):
    """KeyFrame::GetPoseInverse: Twc = [Rcw^T | Ow ; 0 0 0 1]"""
    T = np.asarray(Tcw, np.float32).reshape(4, 4)
    Twc = np.zeros((4, 4), np.float32)
    Twc[:3, :3] = T[:3, :3].T; Twc[:3, 3] = camera_centre(T); Twc[3, 3] = 1
    return Twc


def update_last_frame_pose(Tlr, Tcw_ref):
    """mLastFrame.SetPose(Tlr*pRef->GetPose()) (:825)"""
    return gemm4(Tlr, Tcw_ref)


def predicted_pose(velocity, Tlw):
    """mCurrentFrame.SetPose(mVelocity*mLastFrame.mTcw) (:894)"""
    return gemm4(velocity, Tlw)


def relative_pose(Tcw, Tcw_ref):
    """cv::Mat Tcr = mCurrentFrame.mTcw*mCurrentFrame.mpReferenceKF->GetPoseInverse() (:491)"""
    return gemm4(Tcw, pose_inverse(Tcw_ref))


def th_rule(sensor, th=0.0):
    """Tracking.cc:899-903; th > 0 is the caller's own value"""
    if th > 0:
        return float(th)
    return 7.0 if sensor == STEREO else 15.0


# ---- ids ----
def _slot_of(points):
    slot_of = {int(p["id"]): s for s, p in enumerate(points)}
    assert len(slot_of) == len(points)
    return slot_of


def _resolve(slot_of, i):
    return None if int(i) == NO_MAP_POINT else slot_of.get(int(i))


def check_replaced(last_ids, last_flags, points):
    """CheckReplacedInLastFrame (:754-772).  points: one dict per map slot with id and replaced_by (0 = none, else the new id + 1).  A feature whose held id resolves
    to a record that was replaced receives the new id: one step, whether or not the new id resolves.  A discarded feature holds no point."""
    slot_of = _slot_of(points)
    out = [int(x) for x in last_ids]
    for f, i in enumerate(out):
        if int(last_flags[f]) & FEATURE_DISCARDED:
            continue
        s = _resolve(slot_of, i)
        if s is not None and int(points[s]["replaced_by"]) != 0:
            out[f] = int(points[s]["replaced_by"]) - 1
    return out


def fill(n):
    """fill(mvpMapPoints, NULL) of a fresh Frame (:896): ids and flags"""
    return [NO_MAP_POINT] * n, [0] * n


def retry_rule(n_first, n_wide_fn):
    """:905-911.  n_wide_fn() runs the search at 2 th on an all-NULL frame and returns its count; it is called only when the first count is under 20.
    Returns (searched_wide, n_matches)."""
    if n_first < MIN_MATCHES_MOTION:
        return True, n_wide_fn()
    return False, n_first


def scatter_last(last_ids, match, n):
    """CurrentFrame.mvpMapPoints[f] = LastFrame.mvpMapPoints[match[f]] on an all-NULL frame (ORBmatcher.cc:1582 / 1597)"""
    ids, flags = fill(n)
    for f, m in enumerate(match):
        if m >= 0:
            ids[f] = int(last_ids[int(m)])
    return ids, flags


def set_map_point_matches(kf_ids, match, n):
    """mCurrentFrame.setMapPointMatches(vpMapPointMatches) (:790): every feature is written, flags cleared"""
    ids, flags = fill(n)
    for f, m in enumerate(match):
        if m >= 0:
            ids[f] = int(kf_ids[int(m)])
    return ids, flags


def keyframe_feature_valid(kf_ids, points):
    """if(!pMP) continue; if(pMP->isBad()) continue; (ORBmatcher.cc:195-200): the id resolves to a record that is not bad"""
    slot_of = _slot_of(points)
    out = []
    for i in kf_ids:
        s = _resolve(slot_of, i)
        out.append(1 if s is not None and not int(points[s]["flags"]) & MP_BAD else 0)
    return out


def discard_tail(ids, flags, points, rejected, n_matches, frame_id):
    """The "Discard outliers" loop (:919-940 = :796-814) on the frame after the search.  rejected[f]: this PoseOptimization's mvbOutlier.  points: dicts with id, n_obs,
    last_frame_seen, track_in_view.  Returns (ids, flags, points, n_matches_kept, n_matches_map).  A rejected feature keeps its id in the record behind
    FEATURE_DISCARDED (it names the point whose mnLastFrameSeen is this frame); its outlier flag is clear."""
    slot_of = _slot_of(points)
    ids = [int(x) for x in ids]; flags = [int(x) for x in flags]; pts = copy.deepcopy(points)
    kept, n_map = int(n_matches), 0
    for f in range(len(ids)):
        flags[f] &= ~FEATURE_OUTLIER
        s = None if flags[f] & FEATURE_DISCARDED else _resolve(slot_of, ids[f])
        if rejected[f]:
            assert s is not None                             # an edge exists only for a feature that holds a usable point
            flags[f] |= FEATURE_DISCARDED
            pts[s]["track_in_view"] = 0; pts[s]["last_frame_seen"] = int(frame_id)
            kept -= 1
        elif s is not None and int(pts[s]["n_obs"]) > 0:
            n_map += 1
    return ids, flags, pts, kept, n_map


def motion_model_return(n_matches_kept, n_matches_map, only_tracking):
    """:942-948: (ok, vo)"""
    if only_tracking:
        return n_matches_kept > MIN_KEPT_ONLY_TRACKING, n_matches_map < MIN_MATCHES_MAP
    return n_matches_map >= MIN_MATCHES_MAP, False


def track_with_motion_model(last_ids, points, n_cur, match_first, n_first, wide, rejected, frame_id, only_tracking=False):
    """The whole function from the separate calls' outputs.  last_ids: the last record's ids after check_replaced.  match_first / n_first: the search at th on the
    all-NULL frame.  wide: None, or (match, count) of the search at 2 th -- required iff n_first < 20.  rejected: None when the optimisation did not run, else its
    mvbOutlier.  Returns dict(ids, flags, points, searched_wide, n_matches, n_matches_kept, n_matches_map, ok, vo, ran)."""
    searched_wide, n_matches = retry_rule(n_first, lambda: wide[1])
    match = wide[0] if searched_wide else match_first
    ids, flags = scatter_last(last_ids, match, n_cur)
    if n_matches < MIN_MATCHES_MOTION:                       # return false (:913): the frame keeps the last search's matches
        assert rejected is None
        return dict(ids=ids, flags=flags, points=copy.deepcopy(points), searched_wide=searched_wide, n_matches=n_matches, n_matches_kept=n_matches, n_matches_map=0,
                    ok=False, vo=False, ran=False, match=list(match))
    ids, flags, pts, kept, n_map = discard_tail(ids, flags, points, rejected, n_matches, frame_id)
    ok, vo = motion_model_return(kept, n_map, only_tracking)
    return dict(ids=ids, flags=flags, points=pts, searched_wide=searched_wide, n_matches=n_matches, n_matches_kept=kept, n_matches_map=n_map, ok=ok, vo=vo, ran=True,
                match=list(match))


def track_reference_keyframe(cur_ids, cur_flags, kf_ids, points, match, n_matches, rejected, frame_id):
    """:785-816 from SearchByBoW's output.  Under 15 matches the frame keeps ids and flags.  Returns the dict of track_with_motion_model."""
    if n_matches < MIN_MATCHES_REFERENCE:
        assert rejected is None
        return dict(ids=[int(x) for x in cur_ids], flags=[int(x) for x in cur_flags], points=copy.deepcopy(points), searched_wide=False, n_matches=n_matches,
                    n_matches_kept=n_matches, n_matches_map=0, ok=False, vo=False, ran=False, match=list(match))
    ids, flags = set_map_point_matches(kf_ids, match, len(cur_ids))
    ids, flags, pts, kept, n_map = discard_tail(ids, flags, points, rejected, n_matches, frame_id)
    return dict(ids=ids, flags=flags, points=pts, searched_wide=False, n_matches=n_matches, n_matches_kept=kept, n_matches_map=n_map, ok=n_map >= MIN_MATCHES_MAP, vo=False,
                ran=True, match=list(match))


def finish_stage(ids, flags, points, stage):
    """stage 0: "Clean VO matches" (:438-447): a held point with n_obs < 1 leaves, mvbOutlier cleared.  stage 1 (:463-467): a held point of an outlier feature leaves,
    the flag stays.  Ids that do not resolve and discarded features are untouched."""
    slot_of = _slot_of(points)
    ids = [int(x) for x in ids]; flags = [int(x) for x in flags]
    for f in range(len(ids)):
        s = None if flags[f] & FEATURE_DISCARDED else _resolve(slot_of, ids[f])
        if s is None:
            continue
        if stage == 0:
            if int(points[s]["n_obs"]) < 1:
                flags[f] &= ~FEATURE_OUTLIER; ids[f] = NO_MAP_POINT
        elif flags[f] & FEATURE_OUTLIER:
            ids[f] = NO_MAP_POINT
    return ids, flags

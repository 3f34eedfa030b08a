"""Definition, in plain Python, of what corb_track_local_map leaves behind (include/corb_track_local_map.h): bool Tracking::TrackLocalMap()
(corbslam_client/src/Tracking.cc:951-992) as bookkeeping over the outputs of the three separate calls.

The search and the optimisation themselves are not redone here: the local list (corb_track_update_local_map), the TRACKED array and the matches
(corb_track_search_local_points) and the outlier set (corb_track_pose_optimization, discard_outliers = 0) come from those calls.  From them and the state before the
chain this module derives every write the reference makes beside them: IncreaseVisible / mnLastFrameSeen / mbTrackInView of SearchLocalPoints (:1176-1201),
Frame::isInFrustum's fields (Frame.cc:272, :321-326), mvpMapPoints after the search, mvbOutlier, IncreaseFound, mnMatchesInliers, the stereo outliers' points and
the 30 / 50 decision (:960-991)."""
import copy

NO_MAP_POINT = 0xFFFFFFFFFFFFFFFF
MP_BAD = 1                  # CORB_MP_BAD
FEATURE_OUTLIER = 2         # CORB_FEATURE_OUTLIER
FEATURE_DISCARDED = 4       # CORB_FEATURE_DISCARDED
MONOCULAR, STEREO, RGBD = 0, 1, 2
SCRATCH_FIELDS = ("last_frame_seen", "track_in_view", "track_proj_x", "track_proj_y", "track_proj_xr", "track_scale_level", "track_view_cos")


def th_rule(sensor, frame_id, last_reloc_frame_id, th=0.0):
    """Tracking.cc:1208-1213; th > 0 is the caller's own value"""
    if th > 0:
        return float(th)
    if frame_id < last_reloc_frame_id + 2:
        return 5.0
    return 3.0 if sensor == RGBD else 1.0


def decision(n_matches_inliers, frame_id, last_reloc_frame_id, max_frames):
    """Tracking.cc:983-990"""
    if frame_id < last_reloc_frame_id + max_frames and n_matches_inliers < 50:
        return False
    return n_matches_inliers >= 30


def track_local_map(frame_ids, frame_flags, points, local_slots, tracked, match, outlier, frame_id, last_reloc_frame_id=0, max_frames=30, sensor=STEREO,
                    only_tracking=False, th=0.0):
    """frame_ids / frame_flags: the frame record's per-feature ids and flags BEFORE the chain.  points: one dict per map slot with id, flags, n_obs, n_visible, n_found
    and the seven SCRATCH_FIELDS, before the chain.  local_slots: mvpLocalMapPoints as slots.  tracked: per list entry a dict (valid, proj_x, proj_y, proj_xr, level,
    view_cos) as TrackSearchLocalPoints(want_tracked=True) returns.  match: per feature an index into the list or -1.  outlier: per feature, this PoseOptimization's
    mvbOutlier.  Returns dict(points, frame_ids, frame_flags, n_matches_inliers, ok, th_used); the inputs are left unchanged."""
    ids = [int(x) for x in frame_ids]; flags = [int(x) for x in frame_flags]
    pts = copy.deepcopy(points)
    slot_of = {int(p["id"]): s for s, p in enumerate(pts)}
    assert len(slot_of) == len(pts) and len(tracked) == len(local_slots) and len(match) == len(ids) == len(flags) == len(outlier)

    def resolve(i):
        return None if i == NO_MAP_POINT else slot_of.get(i)

    # UpdateLocalMap (:1278): a feature whose point resolves to a bad record loses it
    for f, i in enumerate(ids):
        s = resolve(i)
        if s is not None and pts[s]["flags"] & MP_BAD:
            ids[f] = NO_MAP_POINT
    # SearchLocalPoints, the frame's own points (:1171-1186)
    seen = set()
    for f, i in enumerate(ids):
        s = resolve(i)
        if s is None:
            continue
        seen.add(i)                                          # a discarded feature's id stays in the record as the point's mnLastFrameSeen == this frame
        if flags[f] & FEATURE_DISCARDED:
            continue
        p = pts[s]
        p["n_visible"] += 1; p["last_frame_seen"] = int(frame_id); p["track_in_view"] = 0
    # the list (:1191-1204) through Frame::isInFrustum
    for q, s in enumerate(local_slots):
        p = pts[int(s)]
        if p["id"] in seen or p["flags"] & MP_BAD:
            continue
        t = tracked[q]
        if t["valid"]:
            p["track_in_view"] = 1
            p["track_proj_x"], p["track_proj_y"], p["track_proj_xr"] = t["proj_x"], t["proj_y"], t["proj_xr"]
            p["track_scale_level"], p["track_view_cos"] = int(t["level"]), t["view_cos"]
            p["n_visible"] += 1
        else:
            p["track_in_view"] = 0
    # SearchByProjection: F.mvpMapPoints[f] = pMP (ORBmatcher.cc:122)
    for f, m in enumerate(match):
        if m >= 0:
            ids[f] = int(pts[int(local_slots[int(m)])]["id"]); flags[f] &= ~(FEATURE_DISCARDED | FEATURE_OUTLIER)
    # PoseOptimization: mvbOutlier
    for f in range(len(ids)):
        flags[f] = (flags[f] & ~FEATURE_OUTLIER) | (FEATURE_OUTLIER if outlier[f] else 0)
    # the tail (:960-978)
    n_inliers = 0
    for f in range(len(ids)):
        s = None if flags[f] & FEATURE_DISCARDED else resolve(ids[f])
        if s is None:
            continue
        if not flags[f] & FEATURE_OUTLIER:
            pts[s]["n_found"] += 1
            if only_tracking or pts[s]["n_obs"] > 0:
                n_inliers += 1
        elif sensor == STEREO:
            ids[f] = NO_MAP_POINT
    return dict(points=pts, frame_ids=ids, frame_flags=flags, n_matches_inliers=n_inliers, ok=decision(n_inliers, frame_id, last_reloc_frame_id, max_frames),
                th_used=th_rule(sensor, frame_id, last_reloc_frame_id, th))

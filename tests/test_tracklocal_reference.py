"""CPU tests of tests/tracklocal_reference.py, the definition the GPU test of corb_track_local_map compares against, on hand-made cases whose answers are worked out
in the comments from corbslam_client/src/Tracking.cc:951-992 and :1168-1216."""
import copy
import pytest
import tracklocal_reference as TR

NONE = TR.NO_MAP_POINT


def point(i, bad=False, n_obs=2, visible=10, found=5):
    p = dict(id=i, flags=TR.MP_BAD if bad else 0, n_obs=n_obs, n_visible=visible, n_found=found)
    p.update(last_frame_seen=0, track_in_view=7, track_proj_x=-1.0, track_proj_y=-1.0, track_proj_xr=-1.0, track_scale_level=-1, track_view_cos=-1.0)
    return p


def seen(valid, x=0.0, level=0):
    return dict(valid=valid, proj_x=x, proj_y=x + 1.0, proj_xr=x - 1.0, level=level, view_cos=0.75)


def scratch(p):
    return tuple(p[k] for k in TR.SCRATCH_FIELDS)


UNTOUCHED = (0, 7, -1.0, -1.0, -1.0, -1, -1.0)


def test_one_frame_by_hand():
    # slots:      0: held by features 0 and 1   1: held by a discarded feature   2: bad, held by feature 3   3: n_obs 0, held by feature 4
    #             4: list point in view, matched by feature 5   5: list point out of the frustum   6: list point in view, unmatched   7: not in the list
    pts = [point(100), point(101), point(102, bad=True), point(103, n_obs=0), point(104), point(105), point(106), point(107)]
    ids = [100, 100, 101, 102, 103, NONE, 555]               # 555 resolves to no record
    flags = [0, 0, TR.FEATURE_DISCARDED, 0, TR.FEATURE_OUTLIER, 0, 0]
    local = [0, 1, 2, 4, 5, 6]
    tracked = [seen(0), seen(0), seen(0), seen(1, 30.0, 2), seen(0), seen(1, 60.0, 3)]
    match = [-1, -1, -1, -1, -1, 3, -1]
    outlier = [0, 1, 0, 0, 0, 0, 0]
    before = copy.deepcopy((pts, ids, flags))
    r = TR.track_local_map(ids, flags, pts, local, tracked, match, outlier, frame_id=40, sensor=TR.STEREO)
    assert (pts, ids, flags) == before                       # the inputs are left alone
    P = r["points"]
    # 100: two features -> visible + 2; feature 0 an inlier (found + 1), feature 1 an outlier (stereo: loses the point)
    assert (P[0]["n_visible"], P[0]["n_found"]) == (12, 6) and scratch(P[0]) == (40, 0) + UNTOUCHED[2:]
    # 101: only a discarded feature keeps its id: seen (the list pass skips it), nothing written
    assert (P[1]["n_visible"], P[1]["n_found"]) == (10, 5) and scratch(P[1]) == UNTOUCHED
    # 102: bad -- the feature loses it, the list pass skips it
    assert (P[2]["n_visible"], P[2]["n_found"]) == (10, 5) and scratch(P[2]) == UNTOUCHED
    # 103: held (the old outlier flag is cleared by this PoseOptimization): visible + 1, found + 1, but n_obs == 0 does not count as an inlier
    assert (P[3]["n_visible"], P[3]["n_found"]) == (11, 6) and scratch(P[3]) == (40, 0) + UNTOUCHED[2:]
    # 104: in view -> visible + 1, the projection written; matched by feature 5 -> found + 1
    assert (P[4]["n_visible"], P[4]["n_found"]) == (11, 6) and scratch(P[4]) == (0, 1, 30.0, 31.0, 29.0, 2, 0.75)
    # 105: isInFrustum returned false: mbTrackInView = false and nothing else
    assert (P[5]["n_visible"], P[5]["n_found"]) == (10, 5) and scratch(P[5]) == (0, 0) + UNTOUCHED[2:]
    # 106: in view, not matched
    assert (P[6]["n_visible"], P[6]["n_found"]) == (11, 5) and scratch(P[6]) == (0, 1, 60.0, 61.0, 59.0, 3, 0.75)
    assert P[7] == pts[7]
    assert r["frame_ids"] == [100, NONE, 101, NONE, 103, 104, 555]
    assert r["frame_flags"] == [0, TR.FEATURE_OUTLIER, TR.FEATURE_DISCARDED, 0, 0, 0, 0]
    assert r["n_matches_inliers"] == 2 and r["ok"] is False and r["th_used"] == 1.0      # features 0 and 5; feature 4's point has no observation


@pytest.mark.parametrize("sensor", [TR.MONOCULAR, TR.STEREO, TR.RGBD])
@pytest.mark.parametrize("only_tracking", [False, True])
def test_sensor_and_only_tracking(sensor, only_tracking):
    pts = [point(1), point(2, n_obs=0)]
    r = TR.track_local_map([1, 2, 1], [0, 0, 0], pts, [], [], [-1, -1, -1], [0, 0, 1], frame_id=9, sensor=sensor, only_tracking=only_tracking)
    assert r["n_matches_inliers"] == (2 if only_tracking else 1)                         # mbOnlyTracking counts a point without observations
    assert r["frame_ids"] == [1, 2, NONE if sensor == TR.STEREO else 1]                  # only STEREO takes the outlier's point away
    assert r["frame_flags"] == [0, 0, TR.FEATURE_OUTLIER]
    assert [p["n_found"] for p in r["points"]] == [6, 6] and [p["n_visible"] for p in r["points"]] == [12, 11]
    assert r["th_used"] == (3.0 if sensor == TR.RGBD else 1.0)


def test_a_matched_feature_loses_its_discarded_and_outlier_flags():
    pts = [point(1), point(2)]
    r = TR.track_local_map([1, NONE], [TR.FEATURE_DISCARDED, TR.FEATURE_OUTLIER], pts, [1], [seen(1)], [0, -1], [0, 0], frame_id=3)
    # feature 0 kept point 1's id as a discarded feature (point 1 is "seen": untouched) and now receives point 2
    assert r["frame_ids"] == [2, NONE] and r["frame_flags"] == [0, 0]
    assert [(p["n_visible"], p["n_found"]) for p in r["points"]] == [(10, 5), (11, 6)]


def test_the_threshold_rule():
    for sensor, base in ((TR.MONOCULAR, 1.0), (TR.STEREO, 1.0), (TR.RGBD, 3.0)):
        assert TR.th_rule(sensor, 101, 100) == 5.0                                       # frame_id = last_reloc + 1 < last_reloc + 2
        assert TR.th_rule(sensor, 102, 100) == base                                      # + 2: no longer
        assert TR.th_rule(sensor, 101, 100, th=2.5) == 2.5


@pytest.mark.parametrize("n,recent,want", [(29, False, False), (30, False, True), (49, False, True), (50, False, True),
                                           (29, True, False), (30, True, False), (49, True, False), (50, True, True)])
def test_the_decision(n, recent, want):
    # recent: mCurrentFrame.mnId < mnLastRelocFrameId + mMaxFrames, here 129 < 100 + 30; not recent: 130
    assert TR.decision(n, 129 if recent else 130, 100, 30) is want
    pts = [point(i) for i in range(1, n + 1)]
    r = TR.track_local_map(list(range(1, n + 1)), [0] * n, pts, [], [], [-1] * n, [0] * n, frame_id=129 if recent else 130, last_reloc_frame_id=100, max_frames=30)
    assert r["n_matches_inliers"] == n and r["ok"] is want

"""CPU tests of tests/trackframe_reference.py, the definition the GPU parity test of include/corb_track_frame.h leans on: hand-made cases of a few features at every
boundary the reference's two functions branch on (19 / 20 matches, 20 / 21 kept in localisation mode, 9 / 10 for nmatchesMap, 14 / 15 for TrackReferenceKeyFrame),
a duplicate id in two rejected features, an unresolvable replaced id, the 4x4 product rule and both finish stages."""
import numpy as np

import trackframe_reference as R

NONE = R.NO_MAP_POINT


def _points(n, n_obs=1):
    return [dict(id=100 + 3 * s, flags=0, n_obs=n_obs, replaced_by=0, last_frame_seen=5, track_in_view=7) for s in range(n)]


def _identity_match(n_cur, n_matched):
    return [f if f < n_matched else -1 for f in range(n_cur)]


def test_gemm4_is_a_double_sum_in_k_order_rounded_once():
    rng = np.random.default_rng(5)
    A = rng.normal(0, 3, (4, 4)).astype(np.float32); B = rng.normal(0, 3, (4, 4)).astype(np.float32)
    C = R.gemm4(A, B)
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += float(A[i, k]) * float(B[k, j])
            assert C[i, j] == np.float32(s)
    # the rule differs from a float accumulation somewhere on such data, and the bottom row is the product's own
    Cf = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            s = np.float32(0)
            for k in range(4):
                s = np.float32(s + np.float32(A[i, k] * B[k, j]))
            Cf[i, j] = s
    assert (C != Cf).any()
    T = np.eye(4, dtype=np.float32); T[3] = [0.5, 0, 0, 2]
    assert R.gemm4(T, T)[3].tolist() == [1.5, 0, 0, 4]


def test_pose_inverse_and_relative_pose():
    c, s = np.float32(0.6), np.float32(0.8)
    T = np.array([[c, 0, s, 1], [0, 1, 0, 2], [-s, 0, c, 3], [0, 0, 0, 1]], np.float32)
    Twc = R.pose_inverse(T)
    assert Twc[3].tolist() == [0, 0, 0, 1] and np.array_equal(Twc[:3, :3], T[:3, :3].T) and np.array_equal(Twc[:3, 3], R.camera_centre(T))
    assert np.allclose(R.relative_pose(T, T), np.eye(4), atol=1e-6)
    assert np.array_equal(R.update_last_frame_pose(np.eye(4, dtype=np.float32), T), T) and np.array_equal(R.predicted_pose(T, np.eye(4, dtype=np.float32)), T)


def test_th_rule():
    assert (R.th_rule(R.STEREO), R.th_rule(R.MONOCULAR), R.th_rule(R.RGBD), R.th_rule(R.STEREO, 9.0)) == (7.0, 15.0, 15.0, 9.0)


def test_replaced_ids_one_step_dangling_and_unresolvable():
    pts = _points(5)
    pts[0]["replaced_by"] = pts[1]["id"] + 1               # to a resolving id
    pts[1]["replaced_by"] = pts[2]["id"] + 1               # ... which is itself replaced: not followed
    pts[3]["replaced_by"] = 9999 + 1                       # to an id no record has
    last = [pts[0]["id"], pts[3]["id"], 777, NONE, pts[4]["id"], pts[0]["id"]]
    flags = [0, 0, 0, 0, 0, R.FEATURE_DISCARDED]
    out = R.check_replaced(last, flags, pts)
    assert out == [pts[1]["id"], 9999, 777, NONE, pts[4]["id"], pts[0]["id"]]       # 777 does not resolve and stays; the discarded feature holds no point


def test_nineteen_and_twenty_matches():
    pts = _points(30)
    last = [p["id"] for p in pts]
    calls = []

    def wide():
        calls.append(1)
        return 19

    assert R.retry_rule(20, wide) == (False, 20) and calls == []
    assert R.retry_rule(19, wide) == (True, 19) and calls == [1]
    # 19 then 19: return false, the frame keeps the wide search's matches, nothing else moves
    r = R.track_with_motion_model(last, pts, 25, _identity_match(25, 19), 19, (_identity_match(25, 19)[::-1], 19), None, 700)
    assert (r["ok"], r["ran"], r["searched_wide"], r["n_matches"]) == (False, False, True, 19)
    assert r["ids"][:6] == [NONE] * 6 and r["ids"][6:] == last[18::-1][:19] and r["flags"] == [0] * 25 and r["points"] == pts
    # 19 then 20: goes on with the wide search's matches
    r = R.track_with_motion_model(last, pts, 25, _identity_match(25, 19), 19, (_identity_match(25, 20), 20), [0] * 25, 700)
    assert (r["ok"], r["ran"], r["searched_wide"], r["n_matches"], r["n_matches_map"]) == (True, True, True, 20, 20)
    # exactly 20 at once: no wide search is consulted
    r = R.track_with_motion_model(last, pts, 25, _identity_match(25, 20), 20, None, [0] * 25, 700)
    assert (r["ok"], r["searched_wide"], r["n_matches_kept"]) == (True, False, 20)


def test_twenty_and_twentyone_kept_in_localisation_mode():
    pts = _points(30)
    last = [p["id"] for p in pts]
    for n, ok in ((20, False), (21, True)):
        r = R.track_with_motion_model(last, pts, 25, _identity_match(25, n), n, None, [0] * 25, 700, only_tracking=True)
        assert (r["n_matches_kept"], r["ok"], r["vo"]) == (n, ok, False)
    # 22 matched, one rejected -> 21 kept; two rejected -> 20 kept
    for rejected, ok in ((1, True), (2, False)):
        rej = [1] * rejected + [0] * (25 - rejected)
        r = R.track_with_motion_model(last, pts, 25, _identity_match(25, 22), 22, None, rej, 700, only_tracking=True)
        assert (r["n_matches_kept"], r["ok"]) == (22 - rejected, ok)


def test_nine_and_ten_observed_points():
    for observed, ok in ((9, False), (10, True)):
        pts = _points(30, n_obs=0)
        for s in range(observed):
            pts[s]["n_obs"] = 2
        last = [p["id"] for p in pts]
        r = R.track_with_motion_model(last, pts, 25, _identity_match(25, 20), 20, None, [0] * 25, 700)
        assert (r["n_matches_map"], r["ok"], r["vo"]) == (observed, ok, False)
        r = R.track_with_motion_model(last, pts, 25, _identity_match(25, 20), 20, None, [0] * 25, 700, only_tracking=True)
        assert (r["ok"], r["vo"]) == (False, not ok)           # 20 kept is not > 20; mbVO = nmatchesMap < 10
        k = R.track_reference_keyframe([NONE] * 25, [0] * 25, last, pts, _identity_match(25, 20), 20, [0] * 25, 700)
        assert (k["n_matches_map"], k["ok"]) == (observed, ok)


def test_fourteen_and_fifteen_for_the_reference_keyframe():
    pts = _points(30)
    kf = [p["id"] for p in pts]
    before_ids = [NONE, 5, 6] + [NONE] * 22; before_flags = [0, R.FEATURE_OUTLIER, R.FEATURE_DISCARDED] + [0] * 22
    r = R.track_reference_keyframe(before_ids, before_flags, kf, pts, _identity_match(25, 14), 14, None, 700)
    assert (r["ok"], r["ran"]) == (False, False) and r["ids"] == before_ids and r["flags"] == before_flags and r["points"] == pts
    r = R.track_reference_keyframe(before_ids, before_flags, kf, pts, _identity_match(25, 15), 15, [0] * 25, 700)
    assert (r["ok"], r["ran"], r["n_matches_map"]) == (True, True, 15)
    assert r["ids"] == kf[:15] + [NONE] * 10 and r["flags"] == [0] * 25           # every feature written, both flags cleared


def test_a_duplicate_id_in_two_rejected_features_and_the_scratch_writes():
    pts = _points(30)
    last = [p["id"] for p in pts]
    last[1] = last[0]                                         # two features of the last frame hold one point
    rej = [1, 1, 0, 1] + [0] * 21
    r = R.track_with_motion_model(last, pts, 25, _identity_match(25, 22), 22, None, rej, 700)
    assert r["n_matches_kept"] == 19 and r["n_matches_map"] == 19
    assert r["flags"][:4] == [R.FEATURE_DISCARDED, R.FEATURE_DISCARDED, 0, R.FEATURE_DISCARDED] and r["ids"][:4] == [last[0], last[0], last[2], last[3]]
    for s, p in enumerate(r["points"]):
        touched = s in (0, 3)
        assert (p["last_frame_seen"], p["track_in_view"]) == ((700, 0) if touched else (5, 7))
    # a feature that holds an id no record has is neither an edge nor counted
    last[5] = 4242
    r = R.track_with_motion_model(last, pts, 25, _identity_match(25, 22), 22, None, [0] * 25, 700)
    assert r["n_matches_map"] == 21 and r["ids"][5] == 4242


def test_keyframe_feature_validity_comes_from_the_map():
    pts = _points(4); pts[1]["flags"] = R.MP_BAD
    assert R.keyframe_feature_valid([pts[0]["id"], pts[1]["id"], 4242, NONE, pts[3]["id"]], pts) == [1, 0, 0, 0, 1]


def test_finish_stages():
    pts = _points(4); pts[1]["n_obs"] = 0
    ids = [pts[0]["id"], pts[1]["id"], 4242, pts[1]["id"], pts[2]["id"], NONE]
    flags = [R.FEATURE_OUTLIER, R.FEATURE_OUTLIER, R.FEATURE_OUTLIER, R.FEATURE_DISCARDED, 0, 0]
    i0, f0 = R.finish_stage(ids, flags, pts, 0)
    assert i0 == [pts[0]["id"], NONE, 4242, pts[1]["id"], pts[2]["id"], NONE] and f0 == [R.FEATURE_OUTLIER, 0, R.FEATURE_OUTLIER, R.FEATURE_DISCARDED, 0, 0]
    i1, f1 = R.finish_stage(i0, f0, pts, 1)
    assert i1 == [NONE, NONE, 4242, pts[1]["id"], pts[2]["id"], NONE] and f1 == f0

"""GPU parity, byte for byte, of the initial pose of a tracked frame on records in one call (include/corb_track_frame.h: corb_track_with_motion_model,
corb_track_reference_keyframe, corb_track_frame_finish).

Every comparison is against the separate existing calls -- TrackSearchLastFrame, SearchByBoW on slots, compute_bow, TrackPoseOptimization(discard_outliers=True) --
run on an identical second copy of the stores with the host steps between them that make the route equivalent (the replaced ids, the poses, the fill, the retry
decision, setMapPointMatches), every one of them tests/trackframe_reference.py's.  From the calls' outputs the definition derives what the chain must leave in the
map points' scratch.  Nothing is compared against the new code, and there is no tolerance anywhere.

The scene is tools/replay_client.World(seed, 12): the reference keyframe observe(4), the last frame observe(5), the current frame observe(6); map-point ids that are
not slots, every 17th point bad, every 23rd with n_obs = 0, ids in the frames that no record has, outlier flags in the last frame, a current record that arrives
with ids and flags of an earlier use, dirty counters and a dirty scratch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import trackframe_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NONE = np.uint64(R.NO_MAP_POINT)
SEED, T_REF, T_LAST, T_CUR = 83, 4, 5, 6
FRAME_ID = 700
PATTERN_A, PATTERN_B = 0xA5A5A5A5, 0x5A5A5A5A
RETRY_ANGLE = 0.014            # rotation of the prediction about y: with the last frame's points at octaves 0 and 1 the oracle's search_by_projection_frame finds 5 matches
                               # at th = 7 and 470 at th = 14 (chosen on the CPU; the test asserts n(th) < 20 <= n(2 th) with the existing GPU call)
_world = {}


def _base():
    if not _world:
        import replay_client as rc
        w = rc.World(SEED, 12)
        _world["w"] = (w, {t: w.observe(t) for t in (T_REF, T_LAST, T_CUR)})
    return _world["w"]


def _inv(T):
    return np.linalg.inv(T.astype(np.float64))


def velocity(angle=0.0):
    """mVelocity as the previous frame would have left it (any float matrix serves: both routes receive the same one)"""
    import replay_client as rc
    w, _ = _base()
    Rm = np.eye(4); Rm[:3, :3] = rc._rot_y(angle)
    return (Rm @ w.pose(T_CUR) @ _inv(w.pose(T_LAST))).astype(np.float32)


def relative_last():
    w, _ = _base()
    return (w.pose(T_LAST) @ _inv(w.pose(T_REF))).astype(np.float32)


class Scene:
    """one copy of the stores.  same_store: the reference keyframe lives in the frames' store.  last_keep: None, or the features of the last frame that hold a point.
    last_ids: None, or a function (ids per feature) -> ids that edits them.  unobserved: map slots whose n_obs is 0 beside every 23rd.  ref_moved: the keyframe's pose
    has changed since the last frame was tracked.  replaced: three of the last frame's points were replaced.  kf_keep: None, or the keyframe's features that hold a
    point.  voc: a device vocabulary -> the keyframe's FeatureVector is computed.  plain: no dirt at all (the mirror program builds the same scene from a file).
    moved: None, or {map slot: world position} of points that are not where the frames saw them."""

    def __init__(self, corb, same_store=False, last_keep=None, last_ids=None, unobserved=(), ref_moved=False, replaced=False, kf_keep=None, voc=None, plain=False, moved=None):
        import replay_client as rc
        self.corb = corb
        w, obs = _base()
        CAM = rc.CAM
        f32 = lambda x: float(np.float32(x))
        self.cam = cam = corb.TrackCamera.make(f32(CAM["fx"]), f32(CAM["fy"]), f32(CAM["cx"]), f32(CAM["cy"]), f32(CAM["bf"]), f32(np.float32(CAM["bf"]) / np.float32(CAM["fx"])),
                                               0.0, float(CAM["w"]), 0.0, float(CAM["h"]), w.scale)
        nL = self.nL = len(w.X)
        ids = self.ids = np.arange(nL, dtype=np.uint64) * np.uint64(3) + np.uint64(1000)
        rec = np.zeros(nL, corb.MP_RECORD_DTYPE)
        rec["id"] = ids; rec["world_pos"] = w.Xest; rec["descriptor"] = w.desc; rec["n_obs"] = 1
        if not plain:
            rec["flags"][::17] = 1; rec["n_obs"][::23] = 0
        rec["n_obs"][list(unobserved)] = 0
        for slot, X in (moved or {}).items():
            rec["world_pos"][slot] = X
        self.rec = rec
        self.MP = MP = corb.MapPointStore(nL, 4)
        off = np.concatenate([[0], np.cumsum(rec["n_obs"])]).astype(np.int32)
        MP.put(0, rec, off, np.full(off[-1], 10, np.uint64), np.zeros(off[-1], np.uint32)); MP.build_index(0, nL)
        keys4, ur4, desc4, lm4 = obs[T_REF]; keys5, ur5, desc5, lm5 = obs[T_LAST]; keys6, ur6, desc6, lm6 = obs[T_CUR]
        self.lm = {T_REF: lm4, T_LAST: lm5, T_CUR: lm6}
        rep = np.zeros(nL, np.uint64)
        held5 = lm5[(np.arange(len(lm5)) % 5 != 0) & (rec["flags"][lm5] == 0)]
        if replaced:                                            # to a resolving good point, to an id no record has, to a bad point
            self.replaced = [int(held5[3]), int(held5[40]), int(held5[77])]
            rep[self.replaced[0]] = ids[held5[4]] + np.uint64(1); rep[self.replaced[1]] = 5; rep[self.replaced[2]] = ids[17 * 3] + np.uint64(1)
        if not plain:
            MP.set_counters(0, 10 + np.arange(nL) % 5, 3 + np.arange(nL) % 2, rep)
            sc = np.zeros(nL, corb.MP_SCRATCH_DTYPE)
            sc["first_kf_id"] = np.arange(nL) % 6 + 10; sc["last_frame_seen"] = 5; sc["track_in_view"] = 7; sc["track_proj_x"] = -1; sc["track_scale_level"] = -2; sc["n_obs_weight"] = 9
            sc["ba_local_for_kf"] = np.arange(nL)
            MP.set_scratch(0, sc)
        inv_s2 = np.zeros(16, np.float32); inv_s2[:8] = (1.0 / (w.scale * w.scale)).astype(np.float32)
        self.KF = KF = corb.KeyFrameStore(3, 2048)
        self.FR = FR = KF if same_store else corb.KeyFrameStore(2, 2048)
        self.ref = 0; self.last, self.cur = (1, 2) if same_store else (0, 1)
        meta = lambda S, slot, kid, T: S.set_meta(slot, id=kid, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, bf=cam.bf, nlevels=8, inv_level_sigma2=inv_s2, Tcw=np.asarray(T, np.float32))
        # the reference keyframe
        KF.put(self.ref, keys4, desc4, ur4, None, keyframe_id=10)
        Tref = w.pose(T_REF).astype(np.float32)
        if ref_moved:
            Tref = Tref.copy(); Tref[0, 3] += np.float32(0.01); Tref[2, 3] -= np.float32(0.004)
        meta(KF, self.ref, 10, Tref)
        kf_ids = ids[lm4].copy()
        if not plain:
            kf_ids[::41] = 7                                    # ids no record has
            kf_ids[::13] = NONE
        if kf_keep is not None:
            keep = np.zeros(len(lm4), bool); keep[list(kf_keep)] = True; kf_ids[~keep] = NONE
        KF.set_map_points(self.ref, kf_ids)
        if voc is not None:
            KF.compute_bow([self.ref], voc, 4)
        # the last frame
        FR.put(self.last, keys5, desc5, ur5, None, keyframe_id=FRAME_ID - 1)
        meta(FR, self.last, FRAME_ID - 1, w.pose(T_LAST).astype(np.float32))
        l_ids = ids[lm5].copy()
        if last_keep is None:
            l_ids[::5] = NONE
            if not plain:
                l_ids[1::41] = 7
        else:
            keep = np.zeros(len(lm5), bool); keep[list(last_keep)] = True; l_ids[~keep] = NONE
        if last_ids is not None:
            l_ids = last_ids(l_ids)
        FR.set_map_points(self.last, l_ids)
        if not plain:
            fl = np.zeros(len(lm5), np.uint8); fl[2::29] = R.FEATURE_OUTLIER; fl[3::97] = R.FEATURE_DISCARDED
            FR.set_flags(self.last, fl)
        # the current frame: the record of an earlier frame, used again
        self.n = len(lm6)
        FR.put(self.cur, keys6, desc6, ur6, None, keyframe_id=FRAME_ID)
        T_old = w.pose(T_CUR).astype(np.float32).copy(); T_old[1, 3] += np.float32(0.5)
        meta(FR, self.cur, FRAME_ID, T_old)
        if not plain:
            c_ids = np.full(self.n, NONE, np.uint64); c_ids[::3] = ids[lm6][::3]
            FR.set_map_points(self.cur, c_ids)
            fl = np.zeros(self.n, np.uint8); fl[::6] = R.FEATURE_OUTLIER; fl[3::6] = R.FEATURE_DISCARDED; fl[1::6] = R.FEATURE_HAS_MP
            FR.set_flags(self.cur, fl)
        else:
            FR.set_map_points(self.cur, np.full(self.n, NONE, np.uint64))

    def stores(self):
        return [self.KF] + ([self.FR] if self.FR is not self.KF else [])

    def snapshot(self, scratch=True, flag_mask=0xFF):
        """every byte the calls could reach: all filled records of the stores, the whole map with counters (and scratch)"""
        out = []
        for S in self.stores():
            for s in range(S.capacity):
                if self.corb.load().corb_kf_store_count(S.h, s) < 0:
                    continue
                d = S.get(s)
                out += [d["kp"].tobytes(), d["desc"].tobytes(), d["u_right"].tobytes(), (d["flags"] & np.uint8(flag_mask)).tobytes(), S.get_meta(s).tobytes(), S.get_map_points(s).tobytes(),
                        d["fv"][0].tobytes(), d["fv"][1].tobytes(), d["fv"][2].tobytes()]
        r, okf, oi = self.MP.get(0, self.nL)
        out += [r.tobytes(), okf.tobytes(), oi.tobytes(), self.MP.get_counters(0, self.nL).tobytes()]
        if scratch:
            out.append(self.MP.get_scratch(0, self.nL).tobytes())
        return out

    def close(self):
        for S in self.stores():
            S.close()
        self.MP.close()


def _points(S):
    ct = S.MP.get_counters(0, S.nL); sc = S.MP.get_scratch(0, S.nL)
    pts = [dict(id=int(S.rec["id"][s]), flags=int(S.rec["flags"][s]), n_obs=int(S.rec["n_obs"][s]), replaced_by=int(ct["replaced_by"][s]),
                last_frame_seen=int(sc["last_frame_seen"][s]), track_in_view=int(sc["track_in_view"][s])) for s in range(S.nL)]
    return pts, sc


def _expected_scratch(sc, pts):
    out = sc.copy()
    for s, p in enumerate(pts):
        out["last_frame_seen"][s] = p["last_frame_seen"]; out["track_in_view"][s] = p["track_in_view"]
    return out


def _fill(S):
    S.FR.set_map_points(S.cur, np.full(S.n, NONE, np.uint64))
    S.FR.set_flags(S.cur, S.FR.get(S.cur)["flags"] & np.uint8(0xFF & ~(R.FEATURE_OUTLIER | R.FEATURE_DISCARDED)))


PAR = dict(frame_id=FRAME_ID, sensor=R.STEREO, only_tracking=False, check_replaced=True, th=0.0)


def _separate_motion(A, par, vel, Tlr, ref_slot=None, kf_store=None):
    """the existing calls with the host steps between them: what corb_track_with_motion_model must give and leave"""
    FR, MP = A.FR, A.MP
    KFS = A.KF if kf_store is None else kf_store
    ref_slot = A.ref if ref_slot is None else ref_slot
    pts, sc = _points(A)
    last_ids = FR.get_map_points(A.last)
    if par["check_replaced"]:
        last_ids = np.array(R.check_replaced(last_ids, FR.get(A.last)["flags"], pts), np.uint64)
        FR.set_map_points(A.last, last_ids)
    if Tlr is not None:
        Tlw = R.update_last_frame_pose(Tlr, KFS.get_meta(ref_slot)["Tcw"])            # a fetch of the reference keyframe's pose
        FR.set_meta(A.last, Tcw=Tlw)
    else:
        Tlw = np.array(FR.get_meta(A.last)["Tcw"], np.float32).reshape(4, 4)
    Tpred = R.predicted_pose(vel, Tlw)
    FR.set_meta(A.cur, Tcw=Tpred)
    th = R.th_rule(par["sensor"], par["th"]); mono = par["sensor"] == R.MONOCULAR
    n = FR._n_features(A.cur)
    search = lambda t: FR.TrackSearchLastFrame(A.cur, A.last, MP, Tpred, Tlw, A.cam, t, mono=mono, nnratio=0.9, check_orientation=True)
    _fill(A)
    m1, n1 = search(th)
    wide = None
    if n1 < R.MIN_MATCHES_MOTION:
        _fill(A)
        wide = search(2 * th)
    n_matches = wide[1] if wide else n1
    T, outl, inl = Tpred, None, 0
    if n_matches >= R.MIN_MATCHES_MOTION:
        T, outl, inl = FR.TrackPoseOptimization(A.cur, MP, A.cam, Tpred, discard_outliers=True)
    want = R.track_with_motion_model(last_ids, pts, n, m1, n1, wide, outl, par["frame_id"], par["only_tracking"])
    # the definition agrees with what the existing calls left in the frame
    assert [int(x) for x in FR.get_map_points(A.cur)] == want["ids"] and [int(x) for x in FR.get(A.cur)["flags"] & np.uint8(6)] == want["flags"]
    return dict(want=want, n_first=n1, wide=wide is not None, n_matches=n_matches, th_used=2 * th if wide else th, inl=inl, T=np.asarray(T, np.float32).reshape(4, 4),
                outl=np.zeros(n, bool) if outl is None else outl, Tlw=Tlw, Tpred=Tpred, scratch=_expected_scratch(sc, want["points"]))


def _chain_motion(B, par, vel, Tlr, ref_slot=None, kf_store=None, **kw):
    return B.FR.TrackWithMotionModel(B.cur, B.last, B.KF if kf_store is None else kf_store, B.ref if ref_slot is None else ref_slot, B.MP, B.cam, vel, par["frame_id"], Tlr=Tlr,
                                     sensor=par["sensor"], only_tracking=par["only_tracking"], check_replaced=par["check_replaced"], th=par["th"], **kw)


def _compare_result(r, ref):
    want = ref["want"]
    assert (r["n_matches_first"], r["searched_wide"], r["n_matches"], r["th_used"]) == (ref["n_first"], ref["wide"], ref["n_matches"], ref["th_used"])
    assert (r["n_pose_inliers"], r["n_matches_kept"], r["n_matches_map"], r["vo"], r["ok"]) == (ref["inl"], want["n_matches_kept"], want["n_matches_map"], want["vo"], want["ok"])
    assert np.array_equal(r["match"], np.asarray(want["match"], np.int32)) and np.array_equal(r["outlier"], ref["outl"])
    assert r["Tlw"].tobytes() == ref["Tlw"].tobytes() and r["Tcw_pred"].tobytes() == ref["Tpred"].tobytes() and r["Tcw"].tobytes() == ref["T"].tobytes()


def _compare(A, B, r, ref, flag_mask=0xFF):
    _compare_result(r, ref)
    assert A.snapshot(scratch=False, flag_mask=flag_mask) == B.snapshot(scratch=False, flag_mask=flag_mask)      # whole records, the map, the counters
    assert B.MP.get_scratch(0, B.nL).tobytes() == ref["scratch"].tobytes()


# ---------------------------------------------------------------- TrackWithMotionModel ----------------------------------------------------------------
@pytest.mark.parametrize("sensor", [R.MONOCULAR, R.STEREO, R.RGBD])
@pytest.mark.parametrize("with_Tlr", [True, False])
def test_no_retry(corb, sensor, with_Tlr):
    par = dict(PAR, sensor=sensor)
    same = sensor == R.RGBD                                   # (one of the cases keeps the reference keyframe in the frames' store)
    A = Scene(corb, same_store=same); B = Scene(corb, same_store=same)
    assert A.snapshot() == B.snapshot()
    Tlr = relative_last() if with_Tlr else None
    ref = _separate_motion(A, par, velocity(), Tlr)
    want = ref["want"]
    assert not ref["wide"] and ref["n_first"] >= 300 and ref["th_used"] == (7.0 if sensor == R.STEREO else 15.0) and want["ok"] and ref["inl"] >= 30
    assert 0 < want["n_matches_map"] < want["n_matches_kept"]           # points with n_obs = 0 are among the matches
    print("sensor %d: matches %d, rejected %d, kept %d, in the map %d" % (sensor, ref["n_matches"], ref["outl"].sum(), want["n_matches_kept"], want["n_matches_map"]))
    _compare(A, B, _chain_motion(B, par, velocity(), Tlr), ref)
    A.close(); B.close()


def test_the_reference_pose_moved_after_the_last_frame_was_tracked(corb):
    A = Scene(corb, ref_moved=True); B = Scene(corb, ref_moved=True)
    stale = np.array(B.FR.get_meta(B.last)["Tcw"], np.float32).reshape(4, 4)
    ref = _separate_motion(A, PAR, velocity(), relative_last())
    assert ref["Tlw"].tobytes() != stale.tobytes() and ref["Tlw"].tobytes() == R.gemm4(relative_last(), B.KF.get_meta(B.ref)["Tcw"]).tobytes()
    r = _chain_motion(B, PAR, velocity(), relative_last())
    _compare(A, B, r, ref)
    assert np.array(B.FR.get_meta(B.last)["Tcw"], np.float32).tobytes() == ref["Tlw"].tobytes()       # Tlw follows the record
    A.close(); B.close()


def test_replaced_points_in_the_last_frame(corb):
    A = Scene(corb, replaced=True); B = Scene(corb, replaced=True)
    before = A.FR.get_map_points(A.last)
    ref = _separate_motion(A, PAR, velocity(), None)
    after = A.FR.get_map_points(A.last)
    changed = np.nonzero(before != after)[0]
    to = {int(before[f]): int(after[f]) for f in changed}
    a, b, c = (int(A.ids[s]) for s in A.replaced)
    assert len(changed) == 3 and to[b] == 4 and int(A.rec["flags"][np.nonzero(A.ids == to[c])[0][0]]) == 1 and to[a] in set(int(x) for x in A.ids)
    _compare(A, B, _chain_motion(B, PAR, velocity(), None), ref)
    # without check_replaced the last record keeps its ids
    C = Scene(corb, replaced=True); D = Scene(corb, replaced=True)
    par = dict(PAR, check_replaced=False)
    ref = _separate_motion(C, par, velocity(), None)
    _compare(C, D, _chain_motion(D, par, velocity(), None), ref)
    assert np.array_equal(D.FR.get_map_points(D.last), before)
    for S in (A, B, C, D):
        S.close()


def _low_octaves():
    w, obs = _base()
    return np.nonzero(obs[T_LAST][0]["octave"] <= 1)[0]


def test_the_retry_is_taken(corb):
    keep = _low_octaves()
    A = Scene(corb, last_keep=keep); B = Scene(corb, last_keep=keep)
    vel = velocity(RETRY_ANGLE)
    ref = _separate_motion(A, PAR, vel, relative_last())
    print("retry: %d matches at th, %d at 2 th" % (ref["n_first"], ref["n_matches"]))
    assert ref["wide"] and ref["n_first"] < 20 <= ref["n_matches"] and ref["th_used"] == 14.0 and ref["want"]["ran"]       # the precondition, from the existing calls
    _compare(A, B, _chain_motion(B, PAR, vel, relative_last()), ref)
    A.close(); B.close()


def _preliminary(corb):
    """Matched and not rejected features of the full scene, from the existing calls, as (feature of the last frame, map slot), the surest first: the point is
    observed and good, the match sits in the rotation histogram's bin 0 away from its edges (the three-maxima filter keeps it whatever else is matched) and the
    reprojection error under the optimised pose is small (the optimisation of a subset keeps it too)"""
    import replay_client as rc
    P = Scene(corb)
    ref = _separate_motion(P, PAR, velocity(), None)
    m = np.asarray(ref["want"]["match"])
    w, obs = _base()
    k5, lm5 = obs[T_LAST][0], obs[T_LAST][3]; k6, ur6 = obs[T_CUR][0], obs[T_CUR][1]
    T = ref["T"].astype(np.float64)
    out = []
    for f in range(P.n):
        if m[f] < 0 or ref["outl"][f]:
            continue
        j = int(m[f]); s = int(lm5[j])
        rot = float(k5["angle"][j]) - float(k6["angle"][f])
        if P.rec["n_obs"][s] < 1 or P.rec["flags"][s] or not 1.0 < rot < 14.0:
            continue
        Xc = T[:3, :3] @ P.rec["world_pos"][s].astype(np.float64) + T[:3, 3]
        e = [k6["x"][f] - (rc.CAM["fx"] * Xc[0] / Xc[2] + rc.CAM["cx"]), k6["y"][f] - (rc.CAM["fy"] * Xc[1] / Xc[2] + rc.CAM["cy"])]
        if ur6[f] >= 0:
            e.append(ur6[f] - (rc.CAM["fx"] * Xc[0] / Xc[2] + rc.CAM["cx"] - rc.CAM["bf"] / Xc[2]))
        out.append((float(np.dot(e, e)) / float(w.scale[k6["octave"][f]]) ** 2, j, s, f))
    P.close()
    out.sort()
    return [(j, s) for _, j, s, _ in out]


def test_both_searches_under_twenty(corb):
    good = _preliminary(corb)[:19]
    keep = [f for f, _ in good]
    A = Scene(corb, last_keep=keep); B = Scene(corb, last_keep=keep)
    before = B.snapshot()
    ref = _separate_motion(A, PAR, velocity(), None)
    assert ref["wide"] and 0 < ref["n_first"] <= 19 and 0 < ref["n_matches"] <= 19 and not ref["want"]["ok"] and not ref["want"]["ran"]
    r = _chain_motion(B, PAR, velocity(), None)
    _compare(A, B, r, ref)
    after = B.snapshot()
    f = B.FR.get(B.cur)
    assert (B.FR.get_map_points(B.cur) != NONE).sum() == ref["n_matches"] and not (f["flags"] & 6).any() and r["Tcw"].tobytes() == r["Tcw_pred"].tobytes()
    assert np.array(B.FR.get_meta(B.cur)["Tcw"], np.float32).tobytes() == r["Tcw_pred"].tobytes()
    assert after[-1] == before[-1] and after[-2] == before[-2]             # no scratch byte, no counter has moved
    A.close(); B.close()


@pytest.mark.parametrize("observed", [9, 10])
def test_exactly_twenty_matches_and_none_rejected(corb, observed):
    good = _preliminary(corb)[:20]
    keep = [f for f, _ in good]
    unobserved = [s for _, s in good[observed:]]
    for only_tracking in (False, True):
        par = dict(PAR, only_tracking=only_tracking)
        A = Scene(corb, last_keep=keep, unobserved=unobserved); B = Scene(corb, last_keep=keep, unobserved=unobserved)
        ref = _separate_motion(A, par, velocity(), None)
        want = ref["want"]
        assert not ref["wide"] and ref["n_matches"] == 20 and not ref["outl"].any() and want["n_matches_kept"] == 20 and want["n_matches_map"] == observed
        assert want["ok"] == ((observed >= 10) if not only_tracking else False) and want["vo"] == (only_tracking and observed < 10)
        _compare(A, B, _chain_motion(B, par, velocity(), None), ref)
        A.close(); B.close()


def test_a_gross_outlier_and_an_id_held_twice(corb):
    """One id sits in two features of the last frame, and one matched point lies nearer on its ray than the frames saw it: its projection stays, its disparity is
    5 px off -- inside the search window, far outside the optimiser's stereo gate -- so its feature is a gross outlier, rejected and discarded.  (The two holders of
    one id project to one place and look for one descriptor: SearchByProjection gives the point to one feature, the other holder finds the feature claimed.)"""
    import replay_client as rc
    w, obs = _base()
    lm5 = obs[T_LAST][3]
    good = _preliminary(corb)
    (a, sa), (b, _) = good[10], good[50]
    near = next((j, s) for j, s in good[60:] if obs[T_LAST][0]["octave"][j] == 0 and obs[T_LAST][1][j] >= 0)
    C = -w.pose(T_CUR)[:3, :3].T @ w.pose(T_CUR)[:3, 3]
    z = (w.pose(T_CUR)[:3, :3] @ w.X[near[1]] + w.pose(T_CUR)[:3, 3])[2]
    k = (rc.CAM["bf"] / (rc.CAM["bf"] / z + 5.0)) / z
    moved = {near[1]: (C + (w.Xest[near[1]].astype(np.float64) - C) * k).astype(np.float32)}

    def twice(l_ids):
        l_ids = l_ids.copy(); l_ids[b] = l_ids[a]
        return l_ids

    A = Scene(corb, last_ids=twice, moved=moved); B = Scene(corb, last_ids=twice, moved=moved)
    ref = _separate_motion(A, PAR, velocity(), None)
    want = ref["want"]
    m = np.asarray(want["match"])
    fa, fb, fn = np.nonzero(m == a)[0], np.nonzero(m == b)[0], np.nonzero(m == near[0])[0]
    assert len(fa) + len(fb) == 1                                        # one point, one feature
    assert len(fn) == 1 and ref["outl"][fn[0]]                           # the precondition: the displaced point's feature is rejected
    slot = near[1]
    assert want["points"][slot]["last_frame_seen"] == FRAME_ID and want["points"][slot]["track_in_view"] == 0
    assert want["flags"][fn[0]] == R.FEATURE_DISCARDED and want["ids"][fn[0]] == int(A.ids[slot])
    _compare(A, B, _chain_motion(B, PAR, velocity(), None), ref)
    sc = B.MP.get_scratch(0, B.nL); fl = B.FR.get(B.cur)["flags"]
    assert sc["last_frame_seen"][slot] == FRAME_ID and sc["track_in_view"][slot] == 0 and fl[fn[0]] & R.FEATURE_DISCARDED
    assert (sc["last_frame_seen"] == FRAME_ID).sum() == len(set(want["ids"][f] for f in np.nonzero(ref["outl"])[0])) and (sc["track_in_view"] == 0).sum() == (sc["last_frame_seen"] == FRAME_ID).sum()
    A.close(); B.close()


# ---------------------------------------------------------------- TrackReferenceKeyFrame ----------------------------------------------------------------
@pytest.fixture(scope="module")
def voc(corb):
    import bow_cases as G
    f = G.vocab("k3L6irr").flat()
    v = corb.Vocabulary(f["k"], f["L"], f["parent"], f["is_leaf"], f["descriptor"], f["weight"])
    yield v
    v.close()


def _kf_has_good_point(S):
    pts, _ = _points(S)
    return np.array(R.keyframe_feature_valid(S.KF.get_map_points(S.ref), pts), np.uint8)


def _separate_reference(A, par, voc, compute_bow, stale_flags=False):
    FR, MP, KF = A.FR, A.MP, A.KF
    pts, sc = _points(A)
    if par["check_replaced"]:
        FR.set_map_points(A.last, np.array(R.check_replaced(FR.get_map_points(A.last), FR.get(A.last)["flags"], pts), np.uint64))
    if compute_bow:
        FR.compute_bow([A.cur], voc, 4)
    if not stale_flags:
        KF.set_flags(A.ref, _kf_has_good_point(A))            # the host's upkeep of "vpMapPoints[i] && !isBad()"
    cur_ids = FR.get_map_points(A.cur); cur_flags = FR.get(A.cur)["flags"]
    kf_ids = KF.get_map_points(A.ref)
    before = np.array(FR.get_meta(A.cur)["Tcw"], np.float32).reshape(4, 4)
    Tlw = np.array(FR.get_meta(A.last)["Tcw"], np.float32).reshape(4, 4)
    m, n = KF.SearchByBoW(A.ref, FR, A.cur, nnratio=0.7, checkOri=True, variant=0)
    T, outl, inl = before, None, 0
    if n >= R.MIN_MATCHES_REFERENCE:
        ids, flags = R.set_map_point_matches(kf_ids, m, len(cur_ids))              # the id gather and its upload
        FR.set_map_points(A.cur, np.array(ids, np.uint64))
        FR.set_flags(A.cur, cur_flags & np.uint8(0xFF & ~(R.FEATURE_OUTLIER | R.FEATURE_DISCARDED)))
        FR.set_meta(A.cur, Tcw=Tlw)
        T, outl, inl = FR.TrackPoseOptimization(A.cur, MP, A.cam, Tlw, discard_outliers=True)
    want = R.track_reference_keyframe(cur_ids, cur_flags & np.uint8(6), kf_ids, pts, m, n, outl, par["frame_id"])
    assert [int(x) for x in FR.get_map_points(A.cur)] == want["ids"] and [int(x) for x in FR.get(A.cur)["flags"] & np.uint8(6)] == want["flags"]
    return dict(want=want, n_first=n, wide=False, n_matches=n, th_used=0.0, inl=inl, T=np.asarray(T, np.float32).reshape(4, 4), outl=np.zeros(len(cur_ids), bool) if outl is None else outl,
                Tlw=Tlw, Tpred=Tlw, scratch=_expected_scratch(sc, want["points"]))


def _chain_reference(B, par, voc):
    return B.FR.TrackReferenceKeyFrame(B.cur, B.last, B.KF, B.ref, B.MP, B.cam, par["frame_id"], voc=voc, sensor=par["sensor"], check_replaced=par["check_replaced"])


@pytest.mark.parametrize("bow_in_call", [True, False])
def test_reference_keyframe_basic(corb, voc, bow_in_call):
    A = Scene(corb, voc=voc, same_store=not bow_in_call); B = Scene(corb, voc=voc, same_store=not bow_in_call)
    if not bow_in_call:
        B.FR.compute_bow([B.cur], voc, 4)
    B.KF.set_flags(B.ref, _kf_has_good_point(B))              # (both copies carry correct HAS_MP bytes here; the chain does not read them)
    ref = _separate_reference(A, PAR, voc, True)
    want = ref["want"]
    n_nodes = len(A.FR.get(A.cur)["fv"][0])
    print("TrackReferenceKeyFrame: %d nodes, %d matches, %d rejected, %d in the map" % (n_nodes, ref["n_matches"], ref["outl"].sum(), want["n_matches_map"]))
    assert n_nodes >= 3 and ref["n_matches"] >= 100 and want["ok"] and ref["inl"] >= 30 and 0 < want["n_matches_map"] < want["n_matches_kept"]
    r = _chain_reference(B, PAR, voc if bow_in_call else None)
    _compare(A, B, r, ref)
    # the pose the optimisation started from is the last record's
    assert r["Tcw_pred"].tobytes() == np.array(B.FR.get_meta(B.last)["Tcw"], np.float32).tobytes()
    # the host mirror of the FeatureVector is current: a matcher on slots that reads it gives the same on both copies
    ma, na = A.KF.SearchByBoW(A.ref, A.FR, A.cur, nnratio=0.7); mb, nb = B.KF.SearchByBoW(B.ref, B.FR, B.cur, nnratio=0.7)
    assert na == nb and np.array_equal(ma, mb)
    A.close(); B.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_reference_keyframe_from_a_pose_whose_rotation_has_a_negative_trace(corb, voc, axis):
    """SetPose(mLastFrame.mTcw) with a last pose turned by 179 degrees about x, y or z: Converter::toSE3Quat takes its other branch, with the largest diagonal element
    at each of the three places; the chain converts the pose on the device, the separate call on the host"""
    a = np.deg2rad(179.0); c, s_ = np.cos(a), np.sin(a)
    Rm = np.eye(4)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    Rm[i, i] = c; Rm[j, j] = c; Rm[i, j] = -s_; Rm[j, i] = s_
    A = Scene(corb, voc=voc); B = Scene(corb, voc=voc)
    T = (Rm @ _base()[0].pose(T_LAST)).astype(np.float32)
    assert T[0, 0] + T[1, 1] + T[2, 2] < 0 and int(np.argmax([T[0, 0], T[1, 1], T[2, 2]])) == axis
    for S in (A, B):
        S.FR.set_meta(S.last, Tcw=T)
    ref = _separate_reference(A, PAR, voc, True)
    assert ref["want"]["ran"] and ref["Tpred"].tobytes() == T.tobytes()
    _compare(A, B, _chain_reference(B, PAR, voc), ref, flag_mask=0xFF & ~R.FEATURE_HAS_MP)
    A.close(); B.close()


def test_reference_keyframe_needs_a_feature_vector_or_a_vocabulary(corb, voc):
    B = Scene(corb, voc=voc)
    before = B.snapshot()
    with pytest.raises(corb.CorbError, match=r"\(-1\)"):
        _chain_reference(B, PAR, None)
    assert B.snapshot() == before
    B.close()


def test_reference_keyframe_with_stale_has_mp_bytes(corb, voc):
    A = Scene(corb, voc=voc); B = Scene(corb, voc=voc)
    valid = _kf_has_good_point(A)
    ids = A.KF.get_map_points(A.ref)
    assert ((ids != NONE) & (valid == 0)).sum() >= 20                     # features whose point is bad or whose id dangles
    ref = _separate_reference(A, PAR, voc, True)                          # correct bytes on this copy
    assert not B.KF.get(B.ref)["flags"].any()                             # stale (all zero) on the copy under test
    _compare(A, B, _chain_reference(B, PAR, voc), ref, flag_mask=0xFF & ~R.FEATURE_HAS_MP)
    assert not B.KF.get(B.ref)["flags"].any()                             # neither read nor written
    A.close(); B.close()


def test_reference_keyframe_under_fifteen(corb, voc):
    P = Scene(corb, voc=voc)
    ref = _separate_reference(P, PAR, voc, True)
    m = np.asarray(ref["want"]["match"])
    keep = sorted(set(int(x) for x in m[m >= 0]))[:14]                   # 14 usable points in the keyframe
    P.close()
    A = Scene(corb, voc=voc, kf_keep=keep); B = Scene(corb, voc=voc, kf_keep=keep)
    B.FR.compute_bow([B.cur], voc, 4)
    before = B.snapshot()
    ref = _separate_reference(A, PAR, voc, True)
    assert 0 < ref["n_matches"] < 15 and not ref["want"]["ok"]
    r = _chain_reference(B, dict(PAR, check_replaced=False), None)
    _compare_result(r, ref)
    assert B.snapshot() == before                                         # the frame is untouched, and so is everything else
    assert r["Tcw"].tobytes() == np.array(B.FR.get_meta(B.cur)["Tcw"], np.float32).tobytes()
    # one more usable point: 15
    keep15 = keep + [next(int(x) for x in m[m >= 0] if int(x) not in keep)]
    A.close(); B.close()
    A = Scene(corb, voc=voc, kf_keep=keep15); B = Scene(corb, voc=voc, kf_keep=keep15)
    ref = _separate_reference(A, PAR, voc, True)
    if ref["n_matches"] >= 15:
        assert ref["want"]["ran"]
    _compare(A, B, _chain_reference(B, PAR, voc), ref, flag_mask=0xFF & ~R.FEATURE_HAS_MP)       # (the HAS_MP bytes are the separate route's upkeep)
    A.close(); B.close()


# ---------------------------------------------------------------- the end of Track, and the chain ----------------------------------------------------------------
def _host_finish(A, kf_store, ref_slot, stage):
    pts, _ = _points(A)
    ids, flags = R.finish_stage(A.FR.get_map_points(A.cur), A.FR.get(A.cur)["flags"], pts, stage)
    full = A.FR.get(A.cur)["flags"]
    A.FR.set_map_points(A.cur, np.array(ids, np.uint64))
    A.FR.set_flags(A.cur, (full & np.uint8(0xFF & ~6)) | np.array(flags, np.uint8) & np.uint8(6))
    return R.relative_pose(A.FR.get_meta(A.cur)["Tcw"], kf_store.get_meta(ref_slot)["Tcw"]) if stage else None


def test_motion_model_then_track_local_map_then_finish(corb):
    """the whole tracked frame on one copy: corb_track_with_motion_model, corb_track_local_map, both finish stages; on the other the separate calls and the definition"""
    import test_gpu_tracklocal as TL
    import tracklocal_reference as TR
    A = TL.Scene(corb, True); B = TL.Scene(corb, True)
    ref_slot = TL.N_KF - 1
    for S in (A, B):
        S.ref = ref_slot
    w = _base()[0]
    vel = velocity()
    Tlr = (w.pose(T_LAST) @ _inv(w.pose(ref_slot))).astype(np.float32)
    par = dict(PAR, check_replaced=False)
    ref = _separate_motion(A, par, vel, Tlr, ref_slot=ref_slot, kf_store=A.KF)
    r = _chain_motion(B, par, vel, Tlr, ref_slot=ref_slot, kf_store=B.KF)
    _compare_result(r, ref)
    assert ref["want"]["ok"] and B.MP.get_scratch(0, B.nL).tobytes() == ref["scratch"].tobytes()
    A.MP.set_scratch(0, ref["scratch"])                                   # the separate calls do not write the scratch: the definition's writes, by hand
    assert A.snapshot() == B.snapshot()
    for S in (A, B):                                                      # a free feature receives a held point: TrackLocalMap's optimisation will call it an outlier
        ids = S.FR.get_map_points(S.cur); fl = S.FR.get(S.cur)["flags"]
        held = [f for f in range(S.n) if ids[f] != NONE and not fl[f] and S.rec["n_obs"][(int(ids[f]) - 1000) // 3] > 0 and not S.rec["flags"][(int(ids[f]) - 1000) // 3]]
        free = [f for f in range(S.n) if ids[f] == NONE and not fl[f]]
        ids[free[0]] = ids[held[0]]
        S.FR.set_map_points(S.cur, ids)
    # TrackLocalMap: the three calls and the tail on A, the one call on B
    A.T0 = ref["T"]; B.T0 = r["Tcw"]
    LPAR = dict(TL.PAR, sensor=TR.RGBD)                                   # (not STEREO: TrackLocalMap's outliers keep their points, which the second finish stage then takes)
    seq = TL._sequence(A, LPAR, {})
    A.FR.TrackLocalMapStats(A.cur, A.MP, LPAR["frame_id"], LPAR["last_reloc_frame_id"], LPAR["max_frames"], LPAR["sensor"], LPAR["only_tracking"])
    A.MP.set_scratch(0, seq["scratch"]); ct = seq["counters"]; A.MP.set_counters(0, ct["n_visible"], ct["n_found"], ct["replaced_by"])
    rl = TL._chain(B, LPAR, {})
    TL._compare(B, rl, seq)
    assert seq["outl"].sum() >= 1 and A.snapshot() == B.snapshot()
    outliers = (A.FR.get(A.cur)["flags"] & R.FEATURE_OUTLIER) != 0
    assert outliers.any() and (A.FR.get_map_points(A.cur)[outliers] != NONE).all()
    # the finish stages
    for stage in (0, 1):
        want_Tcr = _host_finish(A, A.KF, ref_slot, stage)
        got = B.FR.TrackFrameFinish(B.cur, B.KF, ref_slot, B.MP, stage)
        assert A.snapshot() == B.snapshot(), stage
        if stage:
            assert got.tobytes() == want_Tcr.tobytes() and (B.FR.get_map_points(B.cur)[outliers] == NONE).all()
        else:
            assert got is None
    A.close(); B.close()


def test_finish_stages_on_a_frame_with_outliers_and_unobserved_points(corb):
    A = Scene(corb); B = Scene(corb)
    ref = _separate_motion(A, PAR, velocity(), None)
    _chain_motion(B, PAR, velocity(), None)
    for S in (A, B):                                                     # a feature receives another feature's point, then a PoseOptimization that keeps its outliers, as TrackLocalMap's does
        ids = S.FR.get_map_points(S.cur); fl = S.FR.get(S.cur)["flags"]
        held = [f for f in range(S.n) if ids[f] != NONE and ids[f] != 7 and not fl[f] & R.FEATURE_DISCARDED and S.rec["n_obs"][(int(ids[f]) - 1000) // 3] > 0]
        ids[held[5]] = ids[held[200]]
        S.FR.set_map_points(S.cur, ids)
        S.FR.TrackPoseOptimization(S.cur, S.MP, S.cam, ref["T"], discard_outliers=False)
    A.MP.set_scratch(0, ref["scratch"])                                   # the separate calls do not write the scratch: the definition's writes, by hand
    fl = A.FR.get(A.cur)["flags"]; ids = A.FR.get_map_points(A.cur)
    unobserved = [f for f in range(A.n) if ids[f] != NONE and ids[f] != 7 and not fl[f] & R.FEATURE_DISCARDED and A.rec["n_obs"][(int(ids[f]) - 1000) // 3] == 0]
    assert fl[held[5]] & R.FEATURE_OUTLIER and len(unobserved) >= 1 and (fl & R.FEATURE_DISCARDED).any()
    assert A.snapshot() == B.snapshot()
    for stage in (0, 1):
        before = A.FR.get_map_points(A.cur)
        want_Tcr = _host_finish(A, A.KF, A.ref, stage)
        assert (A.FR.get_map_points(A.cur) != before).any()              # the stage does something here
        got = B.FR.TrackFrameFinish(B.cur, B.KF, B.ref, B.MP, stage)
        assert A.snapshot() == B.snapshot(), stage
        if stage:
            assert got.tobytes() == want_Tcr.tobytes()
    A.close(); B.close()


# ---------------------------------------------------------------- arena states, errors, the mirror ----------------------------------------------------------------
def test_workspace_states(corb, voc):
    """a fresh, a warm and two pattern-filled arenas give equal bytes (the corb_scratch_fill rule of tests/test_gpu_workspace_states.py)"""
    keep = _low_octaves()

    def run():
        out = []
        for retry in (False, True):
            B = Scene(corb, last_keep=keep if retry else None)
            r = _chain_motion(B, PAR, velocity(RETRY_ANGLE if retry else 0.0), relative_last())
            assert r["searched_wide"] == retry
            out += [r["match"], r["outlier"], r["Tcw"], r["Tlw"], r["Tcw_pred"], np.array([r["n_matches_first"], r["n_matches"], r["n_pose_inliers"], r["n_matches_kept"], r["n_matches_map"], int(r["ok"])])]
            B.FR.TrackFrameFinish(B.cur, B.KF, B.ref, B.MP, 0)
            out.append(B.FR.TrackFrameFinish(B.cur, B.KF, B.ref, B.MP, 1))
            out += [np.frombuffer(b, np.uint8) for b in B.snapshot()]
            B.close()
        B = Scene(corb, voc=voc)
        r = _chain_reference(B, PAR, voc)
        out += [r["match"], r["outlier"], r["Tcw"], np.array([r["n_matches"], r["n_pose_inliers"], r["n_matches_kept"], r["n_matches_map"], int(r["ok"])])]
        out += [np.frombuffer(b, np.uint8) for b in B.snapshot()]
        B.close()
        return out

    corb.release_scratch(0)
    outs = [run(), run()]
    size = max(corb.scratch_report(0)[0], 1 << 20)
    for word in (PATTERN_A, PATTERN_B):
        filled = corb.scratch_fill(0, word, size)
        outs.append(run())
        assert corb.scratch_report(0)[:2] == (filled, 1), "the call took memory outside the filled chunk"
    for k, o in enumerate(outs[1:]):
        assert [x.tobytes() for x in o] == [x.tobytes() for x in outs[0]], ("fresh", "warm", "pattern A", "pattern B")[k + 1]
    corb.release_scratch(0)


def test_refused_arguments_write_nothing(corb, voc):
    B = Scene(corb, voc=voc)
    before = B.snapshot()

    def refused(fn, *a, **k):
        with pytest.raises(corb.CorbError, match=r"\(-1\)"):
            fn(*a, **k)
        assert B.snapshot() == before

    vel = velocity()
    refused(_chain_motion, B, dict(PAR, sensor=3), vel, None)
    refused(_chain_motion, B, dict(PAR, sensor=-1), vel, None)
    refused(_chain_reference, B, dict(PAR, sensor=3), voc)
    bad_cam = type(B.cam).from_buffer_copy(B.cam); bad_cam.nlevels = 0
    refused(B.FR.TrackWithMotionModel, B.cur, B.last, B.KF, B.ref, B.MP, bad_cam, vel, FRAME_ID)
    refused(B.FR.TrackReferenceKeyFrame, B.cur, B.last, B.KF, B.ref, B.MP, bad_cam, FRAME_ID, voc=voc)
    refused(B.FR.TrackWithMotionModel, B.cur, B.last, B.KF, 1, B.MP, B.cam, vel, FRAME_ID)                # an empty slot as the reference keyframe
    refused(B.FR.TrackReferenceKeyFrame, B.cur, B.last, B.KF, 1, B.MP, B.cam, FRAME_ID, voc=voc)
    refused(B.FR.TrackFrameFinish, B.cur, B.KF, 1, B.MP, 1)
    refused(B.FR.TrackFrameFinish, B.cur, B.KF, B.ref, B.MP, 2)                                         # no such stage
    empty = corb.KeyFrameStore(2, 64)
    refused(empty.TrackWithMotionModel, 1, 0, B.KF, B.ref, B.MP, B.cam, vel, FRAME_ID)                  # empty slots as the frames
    refused(empty.TrackReferenceKeyFrame, 1, 0, B.KF, B.ref, B.MP, B.cam, FRAME_ID, voc=voc)
    refused(empty.TrackFrameFinish, 1, B.KF, B.ref, B.MP, 0)
    refused(B.FR.TrackWithMotionModel, B.cur, B.cur, B.KF, B.ref, B.MP, B.cam, vel, FRAME_ID)             # the last frame is the current one
    big = corb.KeyFrameStore(2, 6016)                                                                   # a frame above the matcher's limit
    for s in (0, 1):
        big.put(s, np.zeros(6001, corb.KP_DTYPE), np.zeros((6001, 32), np.uint8), np.zeros(6001, np.float32), None, keyframe_id=FRAME_ID + 1 + s)
    refused(big.TrackWithMotionModel, 1, 0, B.KF, B.ref, B.MP, B.cam, vel, FRAME_ID)
    import torch
    if torch.cuda.device_count() > 1:                                                                   # stores on different devices (needs a second device to exist)
        other = corb.KeyFrameStore(2, 64, device=1)
        for s in (0, 1):
            other.put(s, np.zeros(4, corb.KP_DTYPE), np.zeros((4, 32), np.uint8), np.zeros(4, np.float32), None, keyframe_id=FRAME_ID + 3 + s)
        refused(other.TrackWithMotionModel, 1, 0, B.KF, B.ref, B.MP, B.cam, vel, FRAME_ID)
        other.close()
    # no map-point index: a put makes it stale (the same record again, so the bytes stay)
    r, okf, oi = B.MP.get(0, 1)
    n0 = int(r["n_obs"][0])
    B.MP.put(0, r, np.array([0, n0], np.int32), okf[0, :n0], oi[0, :n0])
    B.MP.set_counters(0, [10], [3]); sc = np.zeros(1, corb.MP_SCRATCH_DTYPE)
    sc["first_kf_id"] = 10; sc["last_frame_seen"] = 5; sc["track_in_view"] = 7; sc["track_proj_x"] = -1; sc["track_scale_level"] = -2; sc["n_obs_weight"] = 9
    B.MP.set_scratch(0, sc)
    assert B.snapshot() == before
    refused(_chain_motion, B, PAR, vel, None)
    refused(_chain_reference, B, PAR, voc)
    refused(B.FR.TrackFrameFinish, B.cur, B.KF, B.ref, B.MP, 0)
    B.MP.build_index(0, B.nL)
    assert _chain_motion(B, PAR, vel, None)["ok"]
    empty.close(); big.close(); B.close()


def test_frames_without_features(corb):
    B = Scene(corb)
    none = corb.KeyFrameStore(2, 64)
    inv_s2 = np.zeros(16, np.float32)
    for s in (0, 1):
        none.put(s, np.zeros(0, corb.KP_DTYPE), np.zeros((0, 32), np.uint8), np.zeros(0, np.float32), None, keyframe_id=FRAME_ID + s)
        none.set_meta(s, id=FRAME_ID + s, nlevels=8, inv_level_sigma2=inv_s2, Tcw=np.eye(4, dtype=np.float32) * np.float32(1 + s))
    before = B.snapshot()
    r = none.TrackWithMotionModel(1, 0, B.KF, B.ref, B.MP, B.cam, velocity(), FRAME_ID, Tlr=relative_last())
    Tlw = R.gemm4(relative_last(), B.KF.get_meta(B.ref)["Tcw"])
    assert not r["ok"] and r["n_matches"] == 0 and r["Tlw"].tobytes() == Tlw.tobytes() and r["Tcw"].tobytes() == R.gemm4(velocity(), Tlw).tobytes()
    assert np.array(none.get_meta(0)["Tcw"], np.float32).tobytes() == Tlw.tobytes() and np.array(none.get_meta(1)["Tcw"], np.float32).tobytes() == r["Tcw"].tobytes()
    assert B.snapshot() == before
    none.close(); B.close()


def test_the_mirror_program_agrees_with_the_python_route(corb, tmp_path):
    """tests/host/trackframe_main.cpp: corb::TrackInitialPose (TrackWithMotionModel; TrackReferenceKeyFrame is not reached), CleanVOMatches and TrackFrameFinish in a
    child process on a scene handed over in a file"""
    exe = tmp_path / "trackframe_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "trackframe_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    B = Scene(corb, plain=True)
    rec, okf, oi = B.MP.get(0, B.nL)
    n_obs = rec["n_obs"].astype(np.int64); keep = np.arange(B.MP.O)[None, :] < n_obs[:, None]
    recs = []
    for S, slot in ((B.KF, B.ref), (B.FR, B.last), (B.FR, B.cur)):
        d = S.get(slot)
        recs += [S.get_meta(slot).reshape(1), d["kp"], d["desc"], d["u_right"].astype(np.float32), S.get_map_points(slot)]
    cam = B.cam
    vel, Tlr = velocity(), relative_last()
    blob = [np.array([2048, B.nL, B.MP.O, R.STEREO, len(B.lm[T_REF]), len(B.lm[T_LAST]), B.n, 1], np.int32), np.array([FRAME_ID, 0], np.uint64),
            rec, np.concatenate([[0], np.cumsum(n_obs)]).astype(np.int32), okf[keep], oi[keep]] + recs + [
            vel.reshape(16), Tlr.reshape(16), np.array([cam.fx, cam.fy, cam.cx, cam.cy, cam.bf, cam.mb, cam.min_x, cam.max_x, cam.min_y, cam.max_y] + [cam.scale[l] for l in range(8)], np.float32)]
    path = tmp_path / "scene.bin"
    path.write_bytes(b"".join(np.ascontiguousarray(b).tobytes() for b in blob))
    r = _chain_motion(B, PAR, vel, Tlr)
    B.FR.TrackFrameFinish(B.cur, B.KF, B.ref, B.MP, 0)
    Tcr = B.FR.TrackFrameFinish(B.cur, B.KF, B.ref, B.MP, 1)
    p = subprocess.run([str(exe), str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    lines = p.stdout.decode().splitlines()
    assert p.returncode == (0 if r["ok"] else 1) and len(lines) == 4, (p.returncode, p.stderr.decode()[-2000:])
    assert r["ok"] and lines[0] == "R 1 1 %d %d %d %d %d %d %d %d" % (r["n_matches_first"], r["searched_wide"], r["n_matches"], r["n_pose_inliers"], r["n_matches_kept"], r["n_matches_map"],
                                                                  r["vo"], r["outlier"].sum())
    assert lines[1] == "T" + "".join(" %08x" % x for x in r["Tcw"].reshape(16).view(np.uint32))
    assert lines[2] == "I" + "".join(" %d" % x for x in B.FR.get_map_points(B.cur))
    assert lines[3] == "C" + "".join(" %08x" % x for x in Tcr.reshape(16).view(np.uint32))
    B.close()

"""GPU parity, byte for byte, of Tracking::TrackLocalMap on records in one call (corb_track_local_map, include/corb_track_local_map.h).

Every comparison is against the three existing calls -- TrackUpdateLocalMap, TrackSearchLocalPoints, TrackPoseOptimization(discard_outliers=False) -- run on an
identical second copy of the stores, with tests/tracklocal_reference.py deriving from their outputs what the chain must leave in the records.  Nothing is compared
against the new code, and there is no tolerance anywhere.

The scene is tools/replay_client.World(seed, 12): keyframes observe(0..5) with real observation lists in a map-point store whose ids are not slots, a covisibility
graph over the six, the frame observe(6) after TrackSearchLastFrame + TrackPoseOptimization(discard_outliers=True) so that it holds discarded features; every 17th
point is bad, every 23rd has n_obs = 0, every 31st has a distance range its true distance misses, every 37th a normal that looks away, and one id sits in two
features (twice: one pair ends as a discarded feature, the other as an outlier of the chain's own optimisation)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tracklocal_reference as TR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NONE = np.uint64(TR.NO_MAP_POINT)
SEED, N_KF, T_LAST, T_CUR = 83, 6, 5, 6
FRAME_ID = 700
PATTERN_A, PATTERN_B = 0xA5A5A5A5, 0x5A5A5A5A
_world = {}


def _observations(seed):
    if seed not in _world:
        import replay_client as rc
        w = rc.World(seed, 12)
        _world[seed] = (w, [w.observe(t) for t in range(T_CUR + 1)])
    return _world[seed]


class Scene:
    """one copy of the stores.  variant: None the full scene; ("list", L) the keyframes' records hold exactly L good points between them; "no_obs" no map point has
    an observation (an empty vote counter); "two" no observation and the frame holds two points"""

    def __init__(self, corb, own_store, variant=None, seed=SEED):
        import replay_client as rc
        self.corb = corb
        w, obs_t = _observations(seed)
        CAM = rc.CAM
        f32 = lambda x: float(np.float32(x))
        self.cam = cam = corb.TrackCamera.make(f32(CAM["fx"]), f32(CAM["fy"]), f32(CAM["cx"]), f32(CAM["cy"]), f32(CAM["bf"]), f32(np.float32(CAM["bf"]) / np.float32(CAM["fx"])),
                                               0.0, float(CAM["w"]), 0.0, float(CAM["h"]), w.scale)
        self.logs = float(np.float32(np.log(np.float32(1.2))))
        nL = self.nL = len(w.X)
        ids = self.ids = np.arange(nL, dtype=np.uint64) * np.uint64(3) + np.uint64(1000)
        rec = np.zeros(nL, corb.MP_RECORD_DTYPE)
        rec["id"] = ids; rec["world_pos"] = w.Xest; rec["descriptor"] = w.desc; rec["flags"][::17] = 1
        PO = w.Xest - np.array([0.0, 0.0, 4.0], np.float32); dist = np.linalg.norm(PO, axis=1).astype(np.float32)
        rec["normal"] = (PO / dist[:, None]).astype(np.float32)
        rec["normal"][::37] *= np.float32(-1)
        rec["max_distance"] = (dist * w.scale[w.octave] * np.float32(1.3)).astype(np.float32); rec["min_distance"] = (rec["max_distance"] / w.scale[7] / np.float32(1.5)).astype(np.float32)
        rec["max_distance"][::31] = 0.5; rec["min_distance"][::31] = 0.1
        inv_s2 = np.zeros(16, np.float32); inv_s2[:8] = (1.0 / (w.scale * w.scale)).astype(np.float32)
        self.KF = KF = corb.KeyFrameStore(N_KF + 2, 2048); self.MP = MP = corb.MapPointStore(nL, 8)
        self.FR = corb.KeyFrameStore(2, 2048) if own_store else KF
        self.last, self.cur = (0, 1) if own_store else (N_KF, N_KF + 1)
        obs = [dict() for _ in range(nL)]
        budget = variant[1] if isinstance(variant, tuple) else None
        for t in range(N_KF):
            keys, ur, desc, lm = obs_t[t]
            KF.put(t, keys, desc, ur, None, keyframe_id=10 + t)
            KF.set_meta(t, id=10 + t, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, bf=cam.bf, nlevels=8, inv_level_sigma2=inv_s2, Tcw=w.pose(t).astype(np.float32))
            held = ids[lm].copy()
            if budget is not None:                             # the first features of keyframe 0 up to `budget` good points, nothing in the others
                good = np.cumsum(rec["flags"][lm] == 0)
                held[(good > budget) | ((good == budget) & (rec["flags"][lm] != 0))] = NONE
                budget = 0
            KF.set_map_points(t, held)
            for i, j in enumerate(lm):
                obs[int(j)].setdefault(10 + t, i)
        if variant in ("no_obs", "two"):
            obs = [dict() for _ in range(nL)]
        for j in range(0, nL, 23):
            obs[j] = dict()
        rec["n_obs"] = [len(o) for o in obs]
        off = np.concatenate([[0], np.cumsum(rec["n_obs"])]).astype(np.int32)
        MP.put(0, rec, off, np.array([k for o in obs for k in sorted(o)], np.uint64), np.array([o[k] for o in obs for k in sorted(o)], np.uint32)); MP.build_index(0, nL)
        MP.set_counters(0, 10 + np.arange(nL) % 5, 3 + np.arange(nL) % 2)
        sc = np.zeros(nL, corb.MP_SCRATCH_DTYPE)
        sc["first_kf_id"] = np.arange(nL) % 6 + 10; sc["last_frame_seen"] = 5; sc["track_in_view"] = 7; sc["track_proj_x"] = -1; sc["track_scale_level"] = -2; sc["n_obs_weight"] = 9
        sc["ba_local_for_kf"] = np.arange(nL)
        MP.set_scratch(0, sc)
        self.rec = rec
        self.g = corb.Covisibility(KF, MP, 16)
        self.g.UpdateConnections(np.arange(N_KF))
        # the frame: TrackWithMotionModel up to its "Discard outliers"
        FR = self.FR
        keys, ur, desc, lm5 = obs_t[T_LAST]
        FR.put(self.last, keys, desc, ur, None, keyframe_id=FRAME_ID - 1)
        FR.set_meta(self.last, id=FRAME_ID - 1, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, bf=cam.bf, nlevels=8, inv_level_sigma2=inv_s2, Tcw=w.pose(T_LAST).astype(np.float32))
        has = np.zeros(len(lm5), bool); has[::2] = True
        FR.set_map_points(self.last, np.where(has, ids[lm5], NONE))
        keys, ur, desc, lm6 = obs_t[T_CUR]
        self.n = len(lm6)
        FR.put(self.cur, keys, desc, ur, None, keyframe_id=FRAME_ID)
        T_pred = w.pose(T_CUR).astype(np.float32)
        FR.set_meta(self.cur, id=FRAME_ID, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, bf=cam.bf, nlevels=8, inv_level_sigma2=inv_s2, Tcw=T_pred)
        FR.set_map_points(self.cur, np.full(self.n, NONE, np.uint64))
        FR.TrackSearchLastFrame(self.cur, self.last, MP, T_pred, w.pose(T_LAST).astype(np.float32), cam, 7.0, mono=False)
        held = FR.get_map_points(self.cur)
        hi = np.nonzero(held != NONE)[0]; free = np.nonzero(held == NONE)[0]
        assert len(hi) > 300 and len(free) > 300
        held[free[0]] = held[hi[0]]                            # one id in two features: the second is a gross outlier and ends discarded
        if variant == "two":
            held[:] = NONE; held[hi[3]] = ids[lm6[hi[3]]]; held[hi[9]] = ids[lm6[hi[9]]]
        FR.set_map_points(self.cur, held)
        T, out, inl = FR.TrackPoseOptimization(self.cur, MP, cam, T_pred, discard_outliers=True)
        if variant != "two":
            assert out[free[0]] and inl >= 30
            held = FR.get_map_points(self.cur)
            good = [i for i in hi[1:] if not out[i] and rec["flags"][lm6[i]] == 0 and (rec["n_obs"][lm6[i]] > 0 or variant == "no_obs")]
            held[free[1]] = held[good[0]]                      # and again: this pair reaches the chain, whose own optimisation rejects the second
            FR.set_map_points(self.cur, held)
            fl = FR.get(self.cur)["flags"]; fl[free[1]] = 0; FR.set_flags(self.cur, fl)
            self.twice = (good[0], free[1])
        self.T0 = np.asarray(T, np.float32).reshape(4, 4).copy()

    def frame(self):
        return dict(ids=self.FR.get_map_points(self.cur), flags=self.FR.get(self.cur)["flags"].copy(), meta=self.FR.get_meta(self.cur).copy())

    def snapshot(self):
        """every byte the calls could reach: all keyframe records, the whole map with counters and scratch, the graph's rows"""
        out = []
        stores = [self.KF] + ([self.FR] if self.FR is not self.KF else [])
        for S in stores:
            for s in range(S.capacity):
                if self.corb.load().corb_kf_store_count(S.h, s) < 0:
                    continue
                d = S.get(s)
                out += [d["kp"].tobytes(), d["desc"].tobytes(), d["u_right"].tobytes(), d["flags"].tobytes(), S.get_meta(s).tobytes(), S.get_map_points(s).tobytes()]
        r, okf, oi = self.MP.get(0, self.nL)
        out += [r.tobytes(), okf.tobytes(), oi.tobytes(), self.MP.get_counters(0, self.nL).tobytes(), self.MP.get_scratch(0, self.nL).tobytes()]
        for s in range(N_KF):
            (ai, aw), (oi2, ow) = self.g.get(s)
            out += [np.asarray(ai).tobytes(), np.asarray(aw).tobytes(), np.asarray(oi2).tobytes(), np.asarray(ow).tobytes()]
        return out

    def points(self):
        ct = self.MP.get_counters(0, self.nL); sc = self.MP.get_scratch(0, self.nL)
        pts = []
        for s in range(self.nL):
            p = dict(id=int(self.rec["id"][s]), flags=int(self.rec["flags"][s]), n_obs=int(self.rec["n_obs"][s]), n_visible=int(ct["n_visible"][s]), n_found=int(ct["n_found"][s]))
            for k in TR.SCRATCH_FIELDS:
                p[k] = sc[k][s]
            pts.append(p)
        return pts, ct, sc

    def close(self):
        self.g.close(); self.KF.close(); self.MP.close()
        if self.FR is not self.KF:
            self.FR.close()


def _frustum_classes(A, local_slots, tracked, seen_ids):
    """which of isInFrustum's four tests turned each rejected list point away (plain float64 arithmetic: a census of the scene, not a comparison)"""
    T = A.T0.astype(np.float64); C = -T[:3, :3].T @ T[:3, 3]
    counts = [0, 0, 0, 0]
    for q, s in enumerate(local_slots):
        r = A.rec[s]
        if r["flags"] or int(r["id"]) in seen_ids or tracked["valid"][q]:
            continue
        P = r["world_pos"].astype(np.float64); Pc = T[:3, :3] @ P + T[:3, 3]
        if Pc[2] <= 0:
            counts[0] += 1; continue
        u = A.cam.fx * Pc[0] / Pc[2] + A.cam.cx; v = A.cam.fy * Pc[1] / Pc[2] + A.cam.cy
        if u < A.cam.min_x or u > A.cam.max_x or v < A.cam.min_y or v > A.cam.max_y:
            counts[1] += 1; continue
        d = np.linalg.norm(P - C)
        if d < 0.8 * r["min_distance"] or d > 1.2 * r["max_distance"]:
            counts[2] += 1; continue
        counts[3] += (P - C) @ r["normal"].astype(np.float64) / d < 0.5
    return counts


def _sequence(A, par, caps, prev=()):
    """the three existing calls on copy A, then the definition's tail: what the chain must give and leave"""
    pre = A.frame(); pts, ct, sc = A.points()
    ks, ms, mids, info = A.FR.TrackUpdateLocalMap(A.cur, A.g, prev, **caps)
    th = TR.th_rule(par["sensor"], par["frame_id"], par["last_reloc_frame_id"], par.get("th", 0.0))
    m, n_matches, n_in_view, tr = A.FR.TrackSearchLocalPoints(A.cur, A.MP, mids, A.cam, A.T0, A.logs, th=th, nnratio=0.8, want_tracked=True)
    T, outl, inl = A.FR.TrackPoseOptimization(A.cur, A.MP, A.cam, A.T0, discard_outliers=False)
    want = TR.track_local_map(pre["ids"], pre["flags"], pts, ms, tr, m, outl, par["frame_id"], par["last_reloc_frame_id"], par["max_frames"], par["sensor"], par["only_tracking"], par.get("th", 0.0))
    ect = ct.copy(); esc = sc.copy()
    for s, p in enumerate(want["points"]):
        ect["n_visible"][s] = p["n_visible"]; ect["n_found"][s] = p["n_found"]
        for k in TR.SCRATCH_FIELDS:
            esc[k][s] = p[k]
    seen_ids = set(int(i) for i, f in zip(pre["ids"], pre["flags"]) if i != NONE)
    return dict(ks=ks, ms=ms, mids=mids, info=info, m=m, n_matches=n_matches, n_in_view=n_in_view, tr=tr, T=np.asarray(T, np.float32), outl=outl, inl=inl, want=want,
                counters=ect, scratch=esc, pose=A.FR.get_meta(A.cur)["Tcw"].copy(), pre=pre, seen_ids=seen_ids)


def _compare(B, r, ref):
    info, L = ref["info"], r["local"]
    assert bytes(L) == bytes(info)
    assert np.array_equal(r["kf_slots"], ref["ks"]) and np.array_equal(r["mp_slots"], ref["ms"]) and np.array_equal(r["mp_ids"], ref["mids"])
    assert np.array_equal(r["match"], ref["m"]) and np.array_equal(r["outlier"], ref["outl"])
    assert (r["n_in_view"], r["n_matches"], r["n_pose_inliers"]) == (ref["n_in_view"], ref["n_matches"], ref["inl"])
    assert r["Tcw"].tobytes() == ref["T"].reshape(4, 4).tobytes()
    want = ref["want"]
    assert (r["n_matches_inliers"], r["ok"], r["th_used"]) == (want["n_matches_inliers"], want["ok"], want["th_used"])
    f = B.frame()
    assert [int(x) for x in f["ids"]] == want["frame_ids"] and [int(x) for x in f["flags"]] == want["frame_flags"]
    assert f["meta"]["Tcw"].tobytes() == ref["pose"].tobytes()
    assert B.MP.get_counters(0, B.nL).tobytes() == ref["counters"].tobytes()
    assert B.MP.get_scratch(0, B.nL).tobytes() == ref["scratch"].tobytes()


PAR = dict(frame_id=FRAME_ID, last_reloc_frame_id=0, max_frames=30, sensor=TR.STEREO, only_tracking=False)


def _chain(B, par, caps, prev=(), **kw):
    return B.FR.TrackLocalMap(B.cur, B.g, B.cam, B.T0, par["frame_id"], B.logs, prev_kf_slots=prev, last_reloc_frame_id=par["last_reloc_frame_id"], max_frames=par["max_frames"],
                              sensor=par["sensor"], only_tracking=par["only_tracking"], th=par.get("th", 0.0), **dict(caps, **kw))


def _untouched_elsewhere(B, before, after):
    """of the snapshot's pieces only the frame's flags / header / ids and the map's counters / scratch may differ"""
    stores = 1 + (B.FR is not B.KF)
    n_rec = sum(1 for S in ([B.KF] + ([B.FR] if stores == 2 else [])) for s in range(S.capacity) if B.corb.load().corb_kf_store_count(S.h, s) >= 0)
    frame_at = (n_rec - 1) * 6                                # the frame is the last filled slot of the last store
    allowed = {frame_at + 3, frame_at + 4, frame_at + 5, n_rec * 6 + 3, n_rec * 6 + 4}
    assert len(before) == len(after)
    assert [i for i, (a, b) in enumerate(zip(before, after)) if a != b and i not in allowed] == []


@pytest.mark.parametrize("own_store", [True, False])
def test_the_chain_equals_the_three_calls_and_the_definition(corb, own_store):
    A = Scene(corb, own_store); B = Scene(corb, own_store)
    before = B.snapshot()
    assert A.snapshot() == before                             # the two copies are identical
    ref = _sequence(A, PAR, {})
    # the reference side shows the case is not empty
    want = ref["want"]
    assert ref["n_in_view"] >= 200 and ref["n_matches"] >= 100 and ref["outl"].sum() >= 1 and ref["inl"] >= 30 and want["n_matches_inliers"] >= 30 and want["ok"]
    assert (ref["pre"]["flags"] & TR.FEATURE_DISCARDED).any()
    classes = _frustum_classes(A, ref["ms"], ref["tr"], ref["seen_ids"])
    print("list %d, in view %d, matches %d, outliers %d, inliers %d, rejected by depth / image / distance / cosine %s" % (len(ref["ms"]), ref["n_in_view"], ref["n_matches"], ref["outl"].sum(), ref["inl"], classes))
    assert min(classes) >= 1
    a, b = A.twice                                            # one id in two features: visible + 2, the second an outlier that (stereo) loses the point
    slot = int(np.nonzero(A.ids == ref["pre"]["ids"][a])[0][0])
    assert ref["pre"]["ids"][a] == ref["pre"]["ids"][b] and ref["outl"][b] and not ref["outl"][a] and want["frame_ids"][b] == TR.NO_MAP_POINT
    assert want["points"][slot]["n_visible"] == 10 + slot % 5 + 2 and want["points"][slot]["n_found"] == 3 + slot % 2 + 1
    r = _chain(B, PAR, {})
    _compare(B, r, ref)
    _untouched_elsewhere(B, before, B.snapshot())
    # corb_track_local_map_stats after the separate calls is the chain's tail
    got = A.FR.TrackLocalMapStats(A.cur, A.MP, PAR["frame_id"], PAR["last_reloc_frame_id"], PAR["max_frames"], PAR["sensor"], PAR["only_tracking"])
    assert got == (want["n_matches_inliers"], want["ok"])
    fa, fb = A.frame(), B.frame()
    assert fa["ids"].tobytes() == fb["ids"].tobytes() and fa["flags"].tobytes() == fb["flags"].tobytes() and fa["meta"].tobytes() == fb["meta"].tobytes()
    assert np.array_equal(A.MP.get_counters(0, A.nL)["n_found"], ref["counters"]["n_found"])
    A.close(); B.close()


@pytest.mark.parametrize("sensor,only_tracking,reloc", [(TR.MONOCULAR, False, 0), (TR.MONOCULAR, True, FRAME_ID - 1), (TR.STEREO, True, 0), (TR.RGBD, False, 0), (TR.RGBD, True, FRAME_ID - 1)])
def test_sensors_only_tracking_and_the_threshold_rule(corb, sensor, only_tracking, reloc):
    par = dict(PAR, sensor=sensor, only_tracking=only_tracking, last_reloc_frame_id=reloc)
    A = Scene(corb, True); B = Scene(corb, True)
    ref = _sequence(A, par, dict(mp_cap=16384))
    assert ref["want"]["th_used"] == (5.0 if reloc else 3.0 if sensor == TR.RGBD else 1.0) and ref["outl"].sum() >= 1
    _compare(B, _chain(B, par, dict(mp_cap=16384)), ref)
    A.close(); B.close()


@pytest.mark.parametrize("length", [1, 63, 64, 65, 257])
def test_short_lists_with_exact_caps(corb, length):
    A = Scene(corb, True, ("list", length)); B = Scene(corb, True, ("list", length))
    ref = _sequence(A, PAR, {})
    assert len(ref["ms"]) == length
    caps = dict(kf_cap=len(ref["ks"]), mp_cap=length)
    before = B.snapshot()
    _compare(B, _chain(B, PAR, caps), ref)
    _untouched_elsewhere(B, before, B.snapshot())
    A.close(); B.close()


def test_exact_caps_on_the_full_scene_and_one_short(corb):
    A = Scene(corb, False); B = Scene(corb, False)
    ref = _sequence(A, PAR, {})
    caps = dict(kf_cap=len(ref["ks"]), mp_cap=len(ref["ms"]))
    before = B.snapshot()
    for short in (dict(caps, mp_cap=caps["mp_cap"] - 1), dict(caps, kf_cap=caps["kf_cap"] - 1)):
        with pytest.raises(corb.CorbError, match=r"\(-2\)"):
            _chain(B, PAR, short)
        assert B.snapshot() == before                         # CORB_ERR_CAPACITY: no byte of any record has changed
    _compare(B, _chain(B, PAR, caps), ref)
    A.close(); B.close()


def test_an_empty_vote_counter_and_fewer_than_three_correspondences(corb):
    for variant in ("no_obs", "two"):
        A = Scene(corb, True, variant); B = Scene(corb, True, variant)
        par = dict(PAR, only_tracking=variant == "no_obs")
        ref = _sequence(A, par, {})
        assert ref["info"].counter_empty and len(ref["ms"]) == 0 and ref["n_matches"] == 0
        if variant == "no_obs":                               # no list, but the frame's own points are counted and (only tracking) are inliers
            assert ref["want"]["n_matches_inliers"] >= 30 and ref["want"]["ok"]
            assert (ref["counters"]["n_visible"] > 10 + np.arange(A.nL) % 5).sum() >= 30
        else:                                                 # `if(nInitialCorrespondences<3) return 0;`: the pose passes through
            assert ref["inl"] == 0 and ref["T"].tobytes() == A.T0.tobytes() and not ref["want"]["ok"]
        _compare(B, _chain(B, par, {}), ref)
        A.close(); B.close()


def test_refused_arguments_write_nothing(corb):
    B = Scene(corb, True)
    before = B.snapshot()

    def refused(code, fn, *a, **k):
        with pytest.raises(corb.CorbError, match=r"\(%d\)" % code):
            fn(*a, **k)
        assert B.snapshot() == before

    refused(-1, _chain, B, dict(PAR, sensor=3), {})
    refused(-1, _chain, B, dict(PAR, sensor=-1), {})
    refused(-1, B.FR.TrackLocalMap, B.cur, B.g, B.cam, B.T0, FRAME_ID, 0.0)                      # log_scale_factor <= 0
    refused(-1, _chain, B, PAR, dict(mp_cap=60001))                                             # beyond the search's PROJ_MAX_QUERIES
    empty = corb.KeyFrameStore(2, 64)
    refused(-1, empty.TrackLocalMap, 0, B.g, B.cam, B.T0, FRAME_ID, B.logs)                     # an empty slot
    refused(-1, B.FR.TrackLocalMapStats, B.cur, B.MP, FRAME_ID, sensor=3)
    refused(-1, empty.TrackLocalMapStats, 0, B.MP, FRAME_ID)
    big = corb.KeyFrameStore(1, 6016)                                                           # a frame above PROJ_MAX_FEATURES
    big.put(0, np.zeros(6001, corb.KP_DTYPE), np.zeros((6001, 32), np.uint8), np.zeros(6001, np.float32), None, keyframe_id=FRAME_ID + 1)
    refused(-1, big.TrackLocalMap, 0, B.g, B.cam, B.T0, FRAME_ID, B.logs)
    import torch
    if torch.cuda.device_count() > 1:                                                           # stores on different devices (needs a second device to exist)
        other = corb.KeyFrameStore(2, 64, device=1)
        other.put(0, np.zeros(4, corb.KP_DTYPE), np.zeros((4, 32), np.uint8), np.zeros(4, np.float32), None, keyframe_id=FRAME_ID + 2)
        refused(-1, other.TrackLocalMap, 0, B.g, B.cam, B.T0, FRAME_ID, B.logs)
        other.close()
    # no map-point index: a put makes it stale (the same record again, so the bytes stay)
    r, okf, oi = B.MP.get(0, 1)
    n0 = int(r["n_obs"][0])
    B.MP.put(0, r, np.array([0, n0], np.int32), okf[0, :n0], oi[0, :n0])
    B.MP.set_counters(0, [10], [3]); sc = np.zeros(1, corb.MP_SCRATCH_DTYPE)
    sc["first_kf_id"] = 10; sc["last_frame_seen"] = 5; sc["track_in_view"] = 7; sc["track_proj_x"] = -1; sc["track_scale_level"] = -2; sc["n_obs_weight"] = 9
    B.MP.set_scratch(0, sc)
    assert B.snapshot() == before
    refused(-1, _chain, B, PAR, {})
    refused(-1, B.FR.TrackLocalMapStats, B.cur, B.MP, FRAME_ID)
    B.MP.build_index(0, B.nL)
    assert _chain(B, PAR, {})["ok"]
    empty.close(); big.close(); B.close()


def test_workspace_states(corb):
    """a fresh, a warm and two pattern-filled arenas give equal bytes (the corb_scratch_fill rule of tests/test_gpu_workspace_states.py)"""
    def run():
        B = Scene(corb, True)
        r = _chain(B, PAR, {})
        f = B.frame()
        out = [r["kf_slots"], r["mp_slots"], r["mp_ids"], r["match"], r["outlier"], r["Tcw"], np.array([r["n_in_view"], r["n_matches"], r["n_pose_inliers"], r["n_matches_inliers"], int(r["ok"])]),
               f["ids"], f["flags"], B.MP.get_counters(0, B.nL), B.MP.get_scratch(0, B.nL)]
        n, ok = B.FR.TrackLocalMapStats(B.cur, B.MP, FRAME_ID)
        out.append(np.array([n, int(ok)]))
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


def test_the_adapter_runs_one_stereo_frame_and_returns_the_references_bool(corb, tmp_path):
    """tests/host/tracklocal_adapter_main.cpp: FrameStoreT::TrackLocalMap on the test doubles, the scene handed over in a file, against the three calls and the definition"""
    exe = tmp_path / "tracklocal_adapter_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           "-I", os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "tests", "host", "tracklocal_adapter_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    A = Scene(corb, True)
    kfs = [A.KF.get(s) for s in range(N_KF)]
    off = np.concatenate([[0], np.cumsum([len(k["kp"]) for k in kfs])]).astype(np.int32)
    rec, okf, oi = A.MP.get(0, A.nL)
    n_obs = rec["n_obs"].astype(np.int64); keep = np.arange(A.MP.O)[None, :] < n_obs[:, None]
    fr = A.FR.get(A.cur); f = A.frame()
    meta = f["meta"].copy(); meta["Tcw"] = A.T0.reshape(meta["Tcw"].shape)               # mCurrentFrame.mTcw: the pose the frame enters TrackLocalMap with
    cam = A.cam
    blob = [np.array([N_KF, 2048, A.nL, A.MP.O, 16, A.n, TR.STEREO, 0, 30], np.int32), np.array([FRAME_ID, 0], np.uint64),
            np.concatenate([A.KF.get_meta(s).reshape(1) for s in range(N_KF)]), off,
            np.concatenate([k["kp"] for k in kfs]), np.concatenate([k["desc"] for k in kfs]), np.concatenate([k["u_right"] for k in kfs]).astype(np.float32),
            np.concatenate([A.KF.get_map_points(s) for s in range(N_KF)]),
            rec, np.concatenate([[0], np.cumsum(n_obs)]).astype(np.int32), okf[keep], oi[keep],
            meta.reshape(1), fr["kp"], fr["desc"], fr["u_right"].astype(np.float32), f["ids"], f["flags"],
            np.array([cam.mb, cam.min_x, cam.max_x, cam.min_y, cam.max_y, A.logs] + [cam.scale[l] for l in range(8)], np.float32)]
    path = tmp_path / "scene.bin"
    path.write_bytes(b"".join(np.ascontiguousarray(b).tobytes() for b in blob))
    ref = _sequence(A, PAR, {})
    want = ref["want"]
    p = subprocess.run([str(exe), str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    lines = p.stdout.decode().splitlines()
    assert p.returncode == (0 if want["ok"] else 1) and len(lines) == 4, (p.returncode, p.stderr.decode()[-2000:])
    assert lines[0] == "R %d %d %d %d %d %d %d %d" % (want["ok"], want["n_matches_inliers"], ref["n_in_view"], ref["n_matches"], ref["inl"], ref["outl"].sum(), len(ref["ks"]), len(ref["ms"]))
    assert lines[1] == "T" + "".join(" %08x" % x for x in ref["T"].reshape(16).view(np.uint32))
    assert lines[2] == "I" + "".join(" %d" % x for x in want["frame_ids"])
    assert lines[3] == "S %d %d" % (want["ok"], want["n_matches_inliers"])
    A.close()

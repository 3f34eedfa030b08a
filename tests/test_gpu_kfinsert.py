"""Keyframe insertion on records (include/corb_keyframe_insert.h) against its definition (tests/kfinsert_reference.py) on the seeded cases of tests/kfinsert_cases.py:
every output array and every record -- keyframe features, flags, ids and meta; map-point headers, observation lists, counters and scratch -- byte-equal to the
definition applied to the same scene, untouched records included; apply == 0 and every capacity error leave the records alone and return the same outputs; each call
on a fresh handle and on a handle that has just served the largest scene of that call."""
import numpy as np
import pytest

import kfinsert_reference as R
import kfinsert_cases as G
import newpoints_reference as NP
from kfinsert_stores import to_stores, expected_state, state

pytestmark = pytest.mark.gpu


def same(a, b):
    return all(np.array_equal(a[k], b[k]) if isinstance(b[k], np.ndarray) and b[k].dtype != np.float32 else
               (np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) if isinstance(b[k], np.ndarray) else a[k] == b[k]) for k in b)


def cam_of(corb):
    c = G.CAM
    return corb.TrackCamera.make(c["fx"], c["fy"], c["cx"], c["cy"], c["bf"], c["mb"], 0.0, 1241.0, 0.0, 376.0, c["scale"])


# ---------------------------------------------------------------- the handle that has just served the largest scene of a call
class Dirty:
    def __init__(self, corb):
        self.corb = corb; self.h = corb.KeyframeInserter(G.F, 400); self.cam = cam_of(corb)
        self.points = (*to_stores(corb, G.points_case("full_far150")[0]), G.points_case("full_far150")[1])
        self.assoc = (*to_stores(corb, G.assoc_case("full")[0]), G.assoc_case("full")[1])
        self.cull = (*to_stores(corb, G.cull_case("n300")[0]), G.cull_case("n300")[1])

    def serve(self, call):
        if call == 1:
            KF, MP, a = self.points
            self.h.CreateStereoPoints(KF, a["slot"], MP, self.cam, a["th_depth"], 1)
        elif call == 3:
            KF, MP, a = self.assoc
            self.h.ProcessNewKeyFrame(KF, a["slot"], MP, a["kf_first"], a["kf_n"], a["scale_factor"])
        else:
            KF, MP, a = self.cull
            self.h.MapPointCulling(MP, a["recent_slots"], a["cur_kf_id"], a["th_obs"], KF, a["kf_first"], a["kf_n"])
        return self.h


@pytest.fixture(scope="module")
def dirty(corb):
    d = Dirty(corb)
    yield d
    d.h.close()
    for KF, MP, _ in (d.points, d.assoc, d.cull):
        KF.close(); MP.close()


def handles(corb, dirty, call):
    """(name, handle factory): a fresh handle, and the module's handle right after the largest scene of the call"""
    return [("fresh", lambda: corb.KeyframeInserter(G.F, 400)), ("dirty", lambda: dirty.serve(call))]


# ---------------------------------------------------------------- call 1
@pytest.mark.parametrize("name", sorted(G.POINTS))
def test_create_stereo_points(corb, dirty, name):
    sc, a = G.points_case(name)
    cam = cam_of(corb)
    dry, _ = R.create_stereo_points(sc, apply=False, **a)
    want, after = R.create_stereo_points(sc, apply=True, **a)
    assert same(dry, want)
    for which, make in handles(corb, dirty, 1):
        KF, MP = to_stores(corb, sc); h = make()
        before, rest = state(KF, MP)
        assert before == expected_state(corb, sc)
        kw = dict(first_mp_slot=a["first_mp_slot"], first_mp_id=a["first_mp_id"], client_id=a["client_id"], frame_id=a["frame_id"], mirror=KF, mirror_slot=a["mirror"])
        got = h.CreateStereoPoints(KF, a["slot"], MP, cam, a["th_depth"], a["mode"], apply=False, **kw)
        assert same(got, dry), (which, got["n_visited"], dry["n_visited"])
        assert state(KF, MP) == (before, rest)
        if want["n_created"] > 1:                                   # too few free records: the outputs are complete, nothing is written
            short = dict(kw, first_mp_slot=MP.capacity - want["n_created"] + 1)
            got = h.CreateStereoPoints(KF, a["slot"], MP, cam, a["th_depth"], a["mode"], apply=True, **short)
            assert got["capacity_error"] and same(dict(got, capacity_error=False), dry) and state(KF, MP) == (before, rest)
        got = h.CreateStereoPoints(KF, a["slot"], MP, cam, a["th_depth"], a["mode"], apply=True, **kw)
        assert same(got, want), which
        now, rest_now = state(KF, MP)
        exp = expected_state(corb, after)
        for k in range(len(exp)):
            assert now[k] == exp[k], (which, k)
        assert rest_now == rest
        assert np.array_equal(KF.get_map_points(a["mirror"]), KF.get_map_points(a["slot"]))      # the mirror ends with the keyframe's ids
        if which == "fresh":
            h.close()
        KF.close(); MP.close()


def test_create_stereo_points_arguments(corb):
    sc, a = G.points_case("n64")
    KF, MP = to_stores(corb, sc); cam = cam_of(corb); h = corb.KeyframeInserter(G.F, 8)
    with pytest.raises(corb.CorbError):
        h.CreateStereoPoints(KF, 0, MP, cam, 35.0, 3)                                            # no such mode
    with pytest.raises(corb.CorbError):
        h.CreateStereoPoints(KF, 0, MP, cam, 35.0, 1, mirror=KF, mirror_slot=0)                  # the mirror is the keyframe
    small = corb.KeyframeInserter(G.F - 1, 8)
    with pytest.raises(corb.CorbError):
        small.CreateStereoPoints(KF, 0, MP, cam, 35.0, 1)                                        # the store's records are larger than the handle's
    with pytest.raises(corb.CorbError):
        corb.KeyframeInserter(0, 8)
    MP.put(0, np.zeros(1, corb.MP_RECORD_DTYPE), np.zeros(2, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    with pytest.raises(corb.CorbError):
        h.CreateStereoPoints(KF, 0, MP, cam, 35.0, 1)                                            # no current id index
    assert h.CreateStereoPoints(KF, 0, MP, cam, 35.0, 0)["n_visited"] == 64                      # StereoInitialization needs none
    with pytest.raises(corb.CorbError):
        h.MapPointCulling(MP, np.zeros(9, np.int32), 1, 3, KF, 0, 1)                             # a list longer than the handle's
    h.close(); small.close(); KF.close(); MP.close()


# ---------------------------------------------------------------- call 2
@pytest.mark.parametrize("name", ["n0", "n1", "n63", "n64", "n65", "n257", "full"])
def test_need_keyframe_counts(corb, name):
    sc, a = G.assoc_case(name)
    KF, MP = to_stores(corb, sc); h = corb.KeyframeInserter(G.F, 8)
    before = state(KF, MP)
    for th_depth, min_obs, first, n in ((15.0, 0, 1, 5), (15.0, 1, 1, 5), (25.0, 3, 1, 5), (15.0, 3, 0, 6), (15.0, 4, 2, 2), (np.nan, 2, 0, 0)):
        want = R.need_keyframe_counts(sc, 5, th_depth, 5, min_obs, first, n)
        assert h.NeedKeyFrameCounts(KF, 5, MP, th_depth, KF, 5, min_obs, first, n) == want, (th_depth, min_obs, first, n)
    assert h.NeedKeyFrameCounts(KF, 5, MP, 15.0, KF, -1, 0, 1, 5) == R.need_keyframe_counts(sc, 5, 15.0, -1, 0, 1, 5)
    assert state(KF, MP) == before
    h.close(); KF.close(); MP.close()


# ---------------------------------------------------------------- call 3
@pytest.mark.parametrize("name", sorted(G.ASSOC))
def test_process_new_keyframe(corb, dirty, name):
    sc, a = G.assoc_case(name)
    dry, _ = R.process_new_keyframe(sc, apply=False, **a)
    want, after = R.process_new_keyframe(sc, apply=True, **a)
    assert same(dry, want) and want["capacity_error"] == (name == "list_full")
    for which, make in handles(corb, dirty, 3):
        KF, MP = to_stores(corb, sc); h = make()
        before = state(KF, MP)
        assert before[0] == expected_state(corb, sc)
        got = h.ProcessNewKeyFrame(KF, a["slot"], MP, a["kf_first"], a["kf_n"], a["scale_factor"], apply=False)
        assert same(got, dry), which
        assert state(KF, MP) == before
        got = h.ProcessNewKeyFrame(KF, a["slot"], MP, a["kf_first"], a["kf_n"], a["scale_factor"], apply=True)
        assert same(got, want), which
        now, rest = state(KF, MP)
        exp = expected_state(corb, after)                           # (a full list: `after` is the scene as it was)
        for k in range(len(exp)):
            assert now[k] == exp[k], (which, k)
        assert rest == before[1]
        if which == "fresh":
            h.close()
        KF.close(); MP.close()


# ---------------------------------------------------------------- call 4
@pytest.mark.parametrize("name", sorted(G.CULL))
def test_map_point_culling(corb, dirty, name):
    sc, a = G.cull_case(name)
    for first, n in ((a["kf_first"], a["kf_n"]), (0, 5), (2, 1)):                                # observing keyframes inside and outside the named range
        b = dict(a, kf_first=first, kf_n=n)
        dry, _ = R.map_point_culling(sc, apply=False, **b)
        want, after = R.map_point_culling(sc, apply=True, **b)
        assert same(dry, want)
        for which, make in handles(corb, dirty, 4):
            KF, MP = to_stores(corb, sc); h = make()
            before = state(KF, MP)
            got = h.MapPointCulling(MP, b["recent_slots"], b["cur_kf_id"], b["th_obs"], KF, first, n, apply=False)
            assert same(got, dry), which
            assert state(KF, MP) == before
            got = h.MapPointCulling(MP, b["recent_slots"], b["cur_kf_id"], b["th_obs"], KF, first, n, apply=True)
            assert same(got, want), which
            now, rest = state(KF, MP)
            exp = expected_state(corb, after)
            for k in range(len(exp)):
                assert now[k] == exp[k], (which, k)
            assert rest == before[1]
            if which == "fresh":
                h.close()
            KF.close(); MP.close()


# ---------------------------------------------------------------- one keyframe, stage by stage
def test_the_sequence_of_one_keyframe(corb, pyorc):
    """corb_kfi_create_stereo_points, the index, corb_kfi_process_new_keyframe, corb_kfi_map_point_culling, corb_create_new_map_points_store on one map"""
    cur, nbs, truth, W = NP.scene(33, 200, 2)
    rng = np.random.default_rng(33)
    kfs = []
    for k in [cur] + list(nbs):
        n = len(k["kp"])
        kfs.append(dict(id=int(k["id"]), Tcw=k["Tcw"], nlevels=8, kf_flags=0, kp=k["kp"], desc=k["desc"], u_right=k["u_right"], depth=k["depth"], fv=k["fv"],
                        flags=np.zeros(n, np.uint8), mp_id=np.full(n, R.NO_MAP_POINT, np.uint64)))
    # thirty tracked points: seen by the neighbours, held by the current frame, not yet observing it; a few of them old and poorly found
    olds = []
    for q in range(30):
        i = 5 * q; obs = [(int(nbs[j]["id"]), int(truth[j][i])) for j in range(2)]
        p = G.point(rng, 500 + q, obs, found=1 if q % 6 else 0, visible=3, first_kf=int(cur["id"]) - (q % 5))
        olds.append(p)
        kfs[0]["mp_id"][i] = p["id"]; kfs[0]["flags"][i] = R.HAS_MP
        for j in range(2):
            kfs[j + 1]["mp_id"][truth[j][i]] = p["id"]; kfs[j + 1]["flags"][truth[j][i]] = R.HAS_MP
    cam = dict(G.CAM); cam.update({f: float(cur[f]) for f in ("fx", "fy", "cx", "cy", "bf")}); cam["scale"] = cur["scale"]
    sc = dict(kfs=kfs, mps=olds + [None] * 400, cam=cam, F=256, O=8, index={})
    R.build_index(sc, 0, 30)
    KF, MP = to_stores(corb, sc)
    tc = corb.TrackCamera.make(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["bf"], float(cur["mb"]), 0.0, 1241.0, 0.0, 376.0, cam["scale"])
    h = corb.KeyframeInserter(256, 400)

    def check(stage):
        now = state(KF, MP)[0]; exp = expected_state(corb, sc)
        for k in range(len(exp)):
            assert now[k] == exp[k], (stage, k)

    # 1: the stereo points of the new keyframe
    want, sc = R.create_stereo_points(sc, 0, 20.0, 1, True, first_mp_slot=30, first_mp_id=70000, client_id=1, frame_id=9)
    got = h.CreateStereoPoints(KF, 0, MP, tc, 20.0, 1, apply=True, first_mp_slot=30, first_mp_id=70000, client_id=1, frame_id=9)
    assert same(got, want) and 0 < want["n_created"] < want["n_visited"]
    check(1)
    # 2: the index over the old and the new records
    n_mp = 30 + want["n_created"]
    R.build_index(sc, 0, n_mp); MP.build_index(0, n_mp)
    # 3: the association loop
    want3, sc = R.process_new_keyframe(sc, 0, 0, 3, 1.2, True)
    got3 = h.ProcessNewKeyFrame(KF, 0, MP, 0, 3, 1.2, apply=True)
    assert same(got3, want3) and want3["n_added"] == 30 and len(want3["recent_slots"]) == want["n_created"]
    check(3)
    # 4: culling over the earlier keyframes' recent points and this keyframe's
    recent = np.concatenate([np.arange(30, dtype=np.int32), want3["recent_slots"]])
    want4, sc = R.map_point_culling(sc, recent, int(cur["id"]), 3, 0, 3, True)
    got4 = h.MapPointCulling(MP, recent, int(cur["id"]), 3, KF, 0, 3, apply=True)
    assert same(got4, want4) and want4["n_culled"] > 0 and len(want4["kept_slots"]) > want["n_created"]
    check(4)
    # 5: CreateNewMapPoints on what the calls left
    FE = [NP.compute_F12(cur, nb) for nb in nbs]; F12 = [f for f, _ in FE]; ep = [e for _, e in FE]
    probe = KF.CreateNewMapPoints(0, [1, 2], F12, ep, tc)
    dev = {}
    for j in range(2):
        for p in range(probe["pair_offset"][j], probe["pair_offset"][j + 1]):
            if probe["source"][p] == 0:
                dev[(j, int(probe["pairs"][p, 0]), int(probe["pairs"][p, 1]))] = probe["x3d"][p]
    views = [dict(k, has_mp=(s["flags"] & 1).astype(np.uint8), mp_id=s["mp_id"]) for k, s in zip([cur] + list(nbs), sc["kfs"])]
    ref = NP.create_new_map_points(pyorc, views[0], views[1:], F12, ep, x3d_svd=dev, first_mp_id=80000, client_id=1)
    out = KF.CreateNewMapPoints(0, [1, 2], F12, ep, tc, mp_store=MP, first_mp_slot=n_mp, first_mp_id=80000, client_id=1, apply=True)
    assert np.array_equal(out["pairs"], ref["pairs"]) and np.array_equal(out["status"], ref["status"]) and out["n_new"] == ref["n_new"] > 0
    assert np.array_equal(out["x3d"].view(np.uint32), ref["x3d"].view(np.uint32))
    assert not np.isin(out["pairs"][:, 0], want["order"][np.isin(want["kind"], (1, 2))]).any()       # no feature that got a stereo point is triangulated again
    for s in range(3):
        assert np.array_equal(KF.get(s)["flags"], ref["flags"][s]) and np.array_equal(KF.get_map_points(s), ref["mp_ids"][s])
    h.close(); KF.close(); MP.close()

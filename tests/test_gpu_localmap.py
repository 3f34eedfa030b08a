"""GPU parity, bit for bit: Tracking::UpdateLocalMap and the spanning tree on store records (corb_track_update_local_map, corb_covis_*_tree / _child / _parent /
reparent_children) against tests/localmap_reference.py.  Every case builds both stores from the seeded cases of tests/localmap_cases.py, runs the calls on the device
and in Python, and compares every list, count and the frame record's ids, and after every operation the tree state and the row of EVERY slot."""
import os
import sys

import numpy as np
import pytest

import covis_reference as R
import covis_cases as G
import localmap_cases as C
import localmap_reference as LR
import records_reference as RR

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
NO_ID = LR.NO_ID
NONE = np.uint64(NO_ID)


class Dev:
    """a map in the two stores (keyframe k of kf_order in slot k, map point p of mp_order in slot p) with a graph over them.  The current frame goes into the slot
    behind the keyframes (own_store = False: `frames` is the keyframe store itself) or into slot 1 of a store of its own."""

    def __init__(self, corb, m, M=0, F=None, O=12, own_store=False, F_frame=320):
        self.corb = corb; self.m = m
        a = self.a = G.arrays(m)
        self.kf_order = [int(i) for i in a["kf_ids"]]; self.mp_order = [int(i) for i in a["mp_ids"]]
        self.slot = {k: s for s, k in enumerate(self.kf_order)}; self.mp_slot = {p: s for s, p in enumerate(self.mp_order)}
        K = len(self.kf_order); n_mp = len(self.mp_order)
        F = int(np.diff(a["feat_off"]).max()) if F is None else F
        self.KF = corb.KeyFrameStore(K + 1, F if own_store else max(F, F_frame)); self.MP = corb.MapPointStore(max(n_mp, 1), O)
        self.FR = corb.KeyFrameStore(2, F_frame) if own_store else self.KF
        self.frame_slot = 1 if own_store else K
        meta = np.zeros(K, corb.KF_META_DTYPE); meta["id"] = a["kf_ids"]; meta["flags"] = a["kf_bad"].astype(np.uint32); meta["nlevels"] = 8
        kp = np.zeros(len(a["mp_id"]), corb.KP_DTYPE); kp["octave"] = a["octave"]
        self.KF.put_batch(0, meta, a["feat_off"], kp, None, a["u_right"], a["depth"], a["mp_id"])
        rec = np.zeros(n_mp, corb.MP_RECORD_DTYPE); rec["id"] = a["mp_ids"]; rec["n_obs"] = np.diff(a["obs_off"]); rec["flags"] = a["mp_bad"].astype(np.uint32)
        self.MP.put(0, rec, a["obs_off"], a["obs_kf"], a["obs_idx"]); self.MP.build_index(0, n_mp)
        self.g = corb.Covisibility(self.KF, self.MP, M)

    def put_frame(self, frame):
        n = len(frame.mp_ids)
        meta = np.zeros(1, self.corb.KF_META_DTYPE); meta["id"] = C.FRAME_ID; meta["nlevels"] = 8
        self.FR.put_batch(self.frame_slot, meta, np.array([0, n], np.int32), np.zeros(n, self.corb.KP_DTYPE), mp_id=np.array(frame.mp_ids, np.uint64))

    def frame_ids(self):
        return [int(x) for x in self.FR.get_map_points(self.frame_slot)]

    def update(self, kids):
        fp = self.g.UpdateConnections([self.slot[k] for k in kids])
        want = [LR.update_connections(self.m, k) for k in kids]
        assert [None if int(f) == NO_ID else int(f) for f in fp] == want
        return fp

    def set_trees(self):
        """the Python tree into the device (what an archive delivers)"""
        for s, (p, f, c) in enumerate(C.trees(self.m, self.kf_order)):
            self.g.SetTree(s, p, f, c[::-1])                     # any order: the set sorts

    def trees(self):
        return [(p, f, [int(x) for x in c]) for p, f, c in (self.g.GetTree(s) for s in range(len(self.kf_order)))]

    def rows(self):
        out = []
        for s in range(len(self.kf_order)):
            (ai, aw), (oi, ow) = self.g.get(s)
            out.append((([int(i) for i in ai], [int(w) for w in aw]), ([int(i) for i in oi], [int(w) for w in ow])))
        return out

    def check(self):
        assert self.rows() == G.rows(self.m, self.kf_order)
        got = self.trees(); want = C.trees(self.m, self.kf_order)
        for s, (a, b) in enumerate(zip(got, want)):
            assert a == b, (s, self.kf_order[s], a, b)

    def local_map(self, frame, prev_ids, exact_caps=False):
        """one call on the device and in Python, everything compared; returns the definition's answer"""
        self.put_frame(frame)
        want = LR.update_local_map(self.m, frame, prev_ids)
        prev = [self.slot[k] for k in prev_ids]
        kw = dict(kf_cap=len(want["kfs"]), mp_cap=len(want["mps"])) if exact_caps else {}
        ks, ms, ids, info = self.FR.TrackUpdateLocalMap(self.frame_slot, self.g, prev, **kw)
        assert [self.kf_order[s] for s in ks] == want["kfs"]
        assert [int(x) for x in ids] == want["mps"] and [int(s) for s in ms] == [self.mp_slot[p] for p in want["mps"]]
        assert (info.n_kf, info.n_voted, info.n_mp, bool(info.counter_empty), info.n_cleared) == (len(want["kfs"]), want["n_voted"], len(want["mps"]), want["counter_empty"], want["n_cleared"])
        assert (info.ref_slot, info.ref_id) == ((-1, NO_ID) if want["ref"] is None else (self.slot[want["ref"]], want["ref"]))
        assert self.frame_ids() == frame.mp_ids
        return want

    def close(self):
        self.g.close(); self.KF.close(); self.MP.close()
        if self.FR is not self.KF:
            self.FR.close()


def fails_with(corb, code, fn, *args, **kw):
    with pytest.raises(corb.CorbError) as e:
        fn(*args, **kw)
    assert "(%d)" % code in str(e.value), str(e.value)


def tiny(kfs, points, bad_kfs=(), bad_points=()):
    m = R.Map()
    for k, ids in kfs.items():
        m.kfs[k] = R.KeyFrame(k, ids, bad=k in bad_kfs)
    for p, obs in points.items():
        m.mps[p] = R.MapPoint(p, {o: (kfs[o].index(p) if o in kfs and p in kfs[o] else 0) for o in obs}, bad=p in bad_points)
    return m


def test_tree_calls_follow_the_reference_literally(corb):
    m = tiny({k: [100 + k] for k in (1, 2, 3, 4, 5)}, {100 + k: [k] for k in (1, 2, 3, 4, 5)})
    d = Dev(corb, m, M=3)
    d.check()                                                    # a fresh graph: no parent, first connection, no children
    assert d.trees()[0] == (NO_ID, True, [])
    s = d.slot
    for kid, other in ((1, 4), (1, 2), (1, 4), (1, 3)):
        d.g.AddChild(s[kid], s[other]); LR.add_child(m, kid, other); d.check()
    assert d.trees()[s[1]][2] == [2, 3, 4]
    fails_with(corb, -5, d.g.AddChild, s[1], s[5])               # a full set: CORB_ERR_OVERFLOW, nothing changes
    d.check()
    d.g.AddChild(s[1], s[3]); d.check()                          # present already: no overflow
    for kid, other in ((1, 3), (1, 3), (1, 5), (2, 1)):
        d.g.EraseChild(s[kid], s[other]); LR.erase_child(m, kid, other); d.check()
    d.g.ChangeParent(s[5], s[1]); LR.change_parent(m, 5, 1); d.check()
    d.g.ChangeParent(s[5], s[2]); LR.change_parent(m, 5, 2); d.check()      # the old parent keeps the child
    assert d.trees()[s[1]][2] == [2, 4, 5] and d.trees()[s[2]][2] == [5] and d.trees()[s[5]][0] == 2
    LR.set_tree(m, 3, 9000001, False, [5, 1, 9000002]); d.g.SetTree(s[3], 9000001, False, [5, 1, 9000002]); d.check()
    fails_with(corb, -5, d.g.SetTree, s[3], NO_ID, True, [1, 2, 3, 4])
    fails_with(corb, -1, d.g.SetTree, s[3], NO_ID, True, [1, 1])
    d.check()
    d.close()


@pytest.mark.parametrize("name", sorted(G.RANDOM_MAPS))
def test_update_connections_grows_the_tree_batch_and_one_by_one(corb, name):
    kw = G.RANDOM_MAPS[name]
    a = Dev(corb, G.random_map(**kw)); b = Dev(corb, G.random_map(**kw))
    kids = sorted(a.m.kfs)
    first = kids[2::3] + kids[0:5]                               # several first-connection keyframes in one batch, then the whole map over what they left
    first = list(dict.fromkeys(first))
    a.update(first); a.check()
    for k in first:
        b.update([k])
    b.check()
    assert a.trees() == b.trees() and a.rows() == b.rows()
    a.update(kids[::-1]); a.check()
    assert all(f is False for k, (p, f, c) in zip(a.kf_order, a.trees()) if k != 0 and a.m.kfs[k].ordered)
    if 0 in a.m.kfs:
        assert a.trees()[a.slot[0]][:2] == (NO_ID, True)         # mnId 0 takes no parent
    a.close(); b.close()


@pytest.mark.parametrize("own_store", [False, True])
@pytest.mark.parametrize("name", sorted(C.LOCALMAP_CASES))
def test_update_local_map_equals_the_definition(corb, name, own_store):
    kw, frames = C.LOCALMAP_CASES[name]
    kw = dict(kw); tree = kw.pop("tree", None)
    m = G.random_map(**kw)
    d = Dev(corb, m, own_store=own_store)
    d.update(sorted(m.kfs)); d.check()
    if tree:
        C.retree(m, tree); d.set_trees(); d.check()
    prev = sorted(m.kfs)[:3]
    for i, (seed, n, first, width, extra) in enumerate(frames):
        f = C.frame_for(m, seed, n, first, width, **extra)
        before = list(f.mp_ids)
        want = d.local_map(f, prev)
        # the caps exactly enough, then one short each: CORB_ERR_CAPACITY and nothing written, the frame's bad points included
        f2 = LR.Frame(before)
        d.local_map(f2, prev, exact_caps=True)
        d.put_frame(LR.Frame(before))
        ps = [d.slot[k] for k in prev]
        if want["kfs"]:
            fails_with(corb, -2, d.FR.TrackUpdateLocalMap, d.frame_slot, d.g, ps, kf_cap=len(want["kfs"]) - 1, mp_cap=len(want["mps"]))
            assert d.frame_ids() == before
        if want["mps"]:
            fails_with(corb, -2, d.FR.TrackUpdateLocalMap, d.frame_slot, d.g, ps, kf_cap=len(want["kfs"]), mp_cap=len(want["mps"]) - 1)
            assert d.frame_ids() == before
        prev = want["kfs"][:5] if want["kfs"] else prev
    d.check()                                                    # no record but the frame's and no row is written
    d.close()


def test_seventeen_voters_with_sixteen_connections_is_a_capacity_error(corb):
    kfs = {10 + k: [500] for k in range(17)}
    kfs[10] = [500, 501]
    m = tiny(kfs, {500: list(kfs), 501: [10]}, bad_points={501})
    d = Dev(corb, m, M=16, O=20)
    f = LR.Frame([501, 500, 424242])
    d.put_frame(f)
    fails_with(corb, -2, d.FR.TrackUpdateLocalMap, d.frame_slot, d.g, [])
    assert d.frame_ids() == [501, 500, 424242]                   # the bad point is still there
    del m.mps[500].obs[26]                                       # sixteen voters pass
    d2 = Dev(corb, m, M=16, O=20)
    want = d2.local_map(f, [])
    assert want["n_voted"] == 16 and want["n_cleared"] == 1
    d.close(); d2.close()


def test_without_a_map_point_index_the_call_is_refused(corb):
    m = tiny({1: [100]}, {100: [1]})
    d = Dev(corb, m)
    d.put_frame(LR.Frame([100]))
    rec = np.zeros(1, corb.MP_RECORD_DTYPE); rec["id"] = 100; rec["n_obs"] = 1
    d.MP.put(0, rec, np.array([0, 1], np.int32), np.array([1], np.uint64), np.array([0], np.uint32))      # a put invalidates the index
    fails_with(corb, -1, d.FR.TrackUpdateLocalMap, d.frame_slot, d.g, [])
    d.close()


def test_an_empty_frame_slot_or_previous_keyframe_slot_is_refused(corb):
    m = tiny({1: [100]}, {100: [1]})
    d = Dev(corb, m, own_store=True)
    d.put_frame(LR.Frame([100]))
    fails_with(corb, -1, d.FR.TrackUpdateLocalMap, 0, d.g, [])                     # slot 0 of the frames' store was never filled
    fails_with(corb, -1, d.FR.TrackUpdateLocalMap, d.frame_slot, d.g, [1])         # nor was slot 1 of the keyframe store
    assert d.frame_ids() == [100]
    d.local_map(LR.Frame([100]), [1])                                              # (prev is given as ids: keyframe 1 is slot 0)
    d.close()


def test_ids_spread_over_64_bits_collide_in_both_id_tables(corb):
    rng = np.random.default_rng(6)
    kw = dict(seed=41, n_kf=24, F=48, span=5, p_bad_kf=0.1)
    kf_ids = np.sort(RR.colliding_ids(kw["n_kf"], RR.id_table_cells(kw["n_kf"] + 1), rng))
    n_points = len(G.random_map(ids=kf_ids, **kw).mps)
    mp_ids = RR.colliding_ids(n_points, RR.id_table_cells(n_points), rng)
    assert RR.probe_chain(kf_ids, RR.id_table_cells(len(kf_ids) + 1))[1] > 0 and RR.probe_chain(mp_ids, RR.id_table_cells(n_points))[1] > 0
    m = G.random_map(ids=kf_ids, point_ids=mp_ids, **kw)
    d = Dev(corb, m)
    d.update(sorted(m.kfs)); d.check()
    for seed, first, width in ((51, 0, 8), (52, 10, 14)):
        d.local_map(C.frame_for(m, seed, 64, first, width), [])
    for k in C.culling_sequence(m, 7, 4):
        cull(d, k)
    d.local_map(C.frame_for(m, 53, 64, 0, 24), [])
    d.close()


def cull(d, kid):
    """KeyFrame::SetBadFlag on the device as the reference orders it, against the definition"""
    d.g.EraseConnections(d.slot[kid])
    got = d.g.ReparentChildren(d.slot[kid])
    d.KF.set_meta(d.slot[kid], flags=1)                          # CORB_KF_BAD is the caller's to set
    assert got == C.set_bad_flag(d.m, kid)
    d.check()
    return got


@pytest.mark.parametrize("name", ["k8", "k20", "k20_star", "k40_id0"])
def test_culling_reparents_the_children_and_the_local_map_follows(corb, name):
    kw, frames = C.LOCALMAP_CASES[name]
    kw = dict(kw); tree = kw.pop("tree", None)
    m = G.random_map(**kw)
    d = Dev(corb, m)
    d.update(sorted(m.kfs))
    if tree:
        C.retree(m, tree); d.set_trees()
    d.check()
    seq = C.culling_sequence(m, 5, 6)
    if tree == "star":
        seq = [sorted(m.kfs)[0]] + seq                            # the root of the star: many children, no parent
    answers = set()
    for kid in seq:
        answers.add(cull(d, kid)[1])
        seed, n, first, width, extra = frames[0]
        d.local_map(C.frame_for(m, seed, n, first, width, **extra), [])
    if tree is None:
        assert answers == {False, True}                          # the quirk of :658 both ways
    d.close()


def test_the_child_set_of_a_new_parent_overflows_as_a_row_does(corb):
    """max_connections = 2: keyframe 10 (parent 2) is culled; its children 20, 30, 40 have no links, so the fallback hands all three to 2, whose set holds two"""
    m = tiny({k: [100 + k] for k in (2, 10, 20, 30, 40)}, {100 + k: [k] for k in (2, 10, 20, 30, 40)})
    d = Dev(corb, m, M=2)
    LR.set_tree(m, 2, None, False, [10]); d.g.SetTree(d.slot[2], NO_ID, False, [10])
    fails_with(corb, -5, d.g.SetTree, d.slot[10], 2, False, [20, 30, 40])
    LR.set_tree(m, 10, 2, False, [20, 30]); d.g.SetTree(d.slot[10], 2, False, [20, 30])
    d.check()
    fails_with(corb, -5, d.g.ReparentChildren, d.slot[10])       # 2 holds {10, 20}; 30 finds it full, then 10 leaves
    t = d.trees()
    assert t[d.slot[2]] == (NO_ID, False, [20]) and t[d.slot[20]][0] == 2 and t[d.slot[30]][0] == 2
    d.close()


def test_a_keyframe_that_is_its_own_parent_edits_the_set_it_walks(corb):
    """two keyframes that took each other as parents, one of them culled, leave the other as its own parent and child: the fallback's AddChild / EraseChild then work
    on the culled keyframe's own set"""
    m = tiny({k: [100 + k] for k in (2, 10, 20)}, {100 + k: [k] for k in (2, 10, 20)})
    d = Dev(corb, m)
    LR.set_tree(m, 10, 10, False, [10, 20]); LR.set_tree(m, 20, 10, False, [])
    d.set_trees(); d.check()
    assert d.g.ReparentChildren(d.slot[10]) == LR.reparent_children(m, 10) == (2, True)
    d.check()
    assert d.trees()[d.slot[10]] == (10, False, [20])
    d.close()


def test_the_chain_update_local_map_search_local_points_and_culling(corb):
    """TrackLocalMap on records: the device's mp_ids feed corb_track_search_local_points and give what the definition's list gives; then KeyFrameCulling's pick is
    erased and re-parented and the next update of the local map equals the definition's sequence"""
    import replay_client as rc
    w = rc.World(83, 12)
    CAM = rc.CAM
    f32 = lambda x: float(np.float32(x))
    cam = corb.TrackCamera.make(f32(CAM["fx"]), f32(CAM["fy"]), f32(CAM["cx"]), f32(CAM["cy"]), f32(CAM["bf"]), f32(np.float32(CAM["bf"]) / np.float32(CAM["fx"])),
                                0.0, float(CAM["w"]), 0.0, float(CAM["h"]), w.scale)
    nL = len(w.X)
    ids = np.arange(nL, dtype=np.uint64) * np.uint64(3) + np.uint64(1000)
    rec = np.zeros(nL, corb.MP_RECORD_DTYPE)
    rec["id"] = ids; rec["world_pos"] = w.Xest; rec["descriptor"] = w.desc; rec["flags"][::17] = 1
    PO = w.Xest - np.array([0.0, 0.0, 4.0], np.float32); dist = np.linalg.norm(PO, axis=1).astype(np.float32)
    rec["normal"] = (PO / dist[:, None]).astype(np.float32)
    rec["max_distance"] = (dist * w.scale[w.octave] * np.float32(1.3)).astype(np.float32); rec["min_distance"] = (rec["max_distance"] / w.scale[7] / np.float32(1.5)).astype(np.float32)
    n_kf, t_cur = 6, 6
    KF = corb.KeyFrameStore(n_kf + 2, 2048); MP = corb.MapPointStore(nL, 8)
    inv_s2 = np.zeros(16, np.float32); inv_s2[:8] = (1.0 / (w.scale * w.scale)).astype(np.float32)
    m = R.Map(); obs = [dict() for _ in range(nL)]
    for t in range(n_kf):
        keys, ur, desc, lm = w.observe(t)
        KF.put(t, keys, desc, ur, None, keyframe_id=10 + t)
        KF.set_meta(t, id=10 + t, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, bf=cam.bf, nlevels=8, inv_level_sigma2=inv_s2, Tcw=w.pose(t).astype(np.float32))
        KF.set_map_points(t, ids[lm])
        m.kfs[10 + t] = R.KeyFrame(10 + t, [int(x) for x in ids[lm]], octave=keys["octave"].tolist(), u_right=ur.tolist())
        for i, j in enumerate(lm):
            obs[int(j)].setdefault(10 + t, i)
    for j in range(nL):
        m.mps[int(ids[j])] = R.MapPoint(int(ids[j]), obs[j], bad=bool(rec["flags"][j]))
    rec["n_obs"] = [len(o) for o in obs]
    off = np.concatenate([[0], np.cumsum(rec["n_obs"])]).astype(np.int32)
    MP.put(0, rec, off, np.array([k for o in obs for k in sorted(o)], np.uint64), np.array([o[k] for o in obs for k in sorted(o)], np.uint32)); MP.build_index(0, nL)
    keys, ur, desc, lm = w.observe(t_cur)
    held = np.zeros(len(lm), bool); held[::3] = True
    T = w.pose(t_cur).astype(np.float32)
    for s in (n_kf, n_kf + 1):                                   # the current frame twice: one for the device's list, one for the definition's
        KF.put(s, keys, desc, ur, None, keyframe_id=C.FRAME_ID + s)
        KF.set_meta(s, id=C.FRAME_ID + s, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, bf=cam.bf, nlevels=8, inv_level_sigma2=inv_s2, Tcw=T)
        KF.set_map_points(s, np.where(held, ids[lm], NONE))
    g = corb.Covisibility(KF, MP, 16)
    slot = {10 + t: t for t in range(n_kf)}
    fp = g.UpdateConnections(np.arange(n_kf))
    assert [int(x) for x in fp] == [LR.update_connections(m, 10 + t) for t in range(n_kf)]
    frame = LR.Frame([int(x) for x in np.where(held, ids[lm], NONE)])
    want = LR.update_local_map(m, frame, [])
    ks, ms, mids, info = KF.TrackUpdateLocalMap(n_kf, g)
    assert [10 + int(s) for s in ks] == want["kfs"] and [int(x) for x in mids] == want["mps"] and info.ref_id == want["ref"] and len(mids) > 500
    logs = float(np.float32(np.log(np.float32(1.2))))
    a = KF.TrackSearchLocalPoints(n_kf, MP, mids, cam, T, logs)
    b = KF.TrackSearchLocalPoints(n_kf + 1, MP, np.array(want["mps"], np.uint64), cam, T, logs)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] and a[1] > 100
    # (the second frame's record was not cleaned by an update: SearchLocalPoints drops the bad points itself, so the records agree where a point is held)
    got = KF.get_map_points(n_kf); frame.mp_ids = [int(x) for x in got]
    assert np.array_equal(got, KF.get_map_points(n_kf + 1))
    # LocalMapping on the newest keyframe: culling's answers, then SetBadFlag of one listed keyframe through erase -> reparent
    cs, nm, nr, cu = g.KeyFrameCulling(slot[15], True, 35.0)
    assert [(10 + int(s), int(x), int(y), bool(z)) for s, x, y, z in zip(cs, nm, nr, cu)] == R.keyframe_culling(m, 15, True, 35.0)
    pick = next((10 + int(s) for s, z in zip(cs, cu) if z), 10 + int(cs[0]))
    g.EraseConnections(slot[pick]); got = g.ReparentChildren(slot[pick]); KF.set_meta(slot[pick], flags=1)
    assert got == C.set_bad_flag(m, pick)
    for t in range(n_kf):
        p, f, c = g.GetTree(t)
        assert (None if p == NO_ID else p, f, [int(x) for x in c]) == LR.get_tree(m, 10 + t)
    want2 = LR.update_local_map(m, frame, want["kfs"])
    ks2, ms2, mids2, info2 = KF.TrackUpdateLocalMap(n_kf, g, [slot[k] for k in want["kfs"]])
    assert [10 + int(s) for s in ks2] == want2["kfs"] and [int(x) for x in mids2] == want2["mps"]
    assert [int(x) for x in KF.get_map_points(n_kf)] == frame.mp_ids
    g.close(); KF.close(); MP.close()

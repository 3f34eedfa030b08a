"""GPU parity of the loop-correction calls on store records against tests/loopfix_reference.py.  First, bit for bit, the map update after a global bundle adjustment
(corb_gba_propagate_store, corb_covis_set / get_pose_before_gba); below it CorrectLoop's propagation (corb_loop_correct_store).  Its FP64 Sim3 parts were allowed
1e-12 relative on the doubles and one last place (2^-23 x the vector's largest magnitude) on the floats; the build turned out bit-equal to the numpy definition on every
case -- the operations are IEEE +, -, x, / and sqrt in one order on both sides, nothing is contracted -- so the poses, the positions and the two n x 8 arrays are
asserted EQUAL.  Normal and distances keep the project's bar (2e-7 absolute, 2e-6 relative).  Every case builds both stores and the graph's tree from the seeded cases of tests/loopfix_cases.py, runs the call on the device and in
Python, and compares Tcw, mTcwGBA, the mark and mTcwBefGBA of EVERY slot, every point's position and all seven counts.  The whole path is the float convention of
csrc/loopfix_internal.h, so every comparison is an equality."""
import numpy as np
import pytest

import covis_cases as G
import loopfix_cases as C
import loopfix_reference as XR

pytestmark = pytest.mark.gpu
NO_ID = XR.NO_ID
L = C.LOOP_KF
COUNTS = ("n_popped", "n_reached", "n_propagated", "n_revisited", "n_points_set", "n_points_moved", "n_points_skipped")


class Dev:
    """a map in the two stores (keyframe k of `order` in slot k, map point p of sorted(m.mps) in slot p, one empty keyframe slot behind them) with a graph over them"""

    def __init__(self, corb, m, order, M=0):
        self.corb = corb; self.m = m; self.order = list(order); self.mp_order = sorted(m.mps)
        self.slot = {k: s for s, k in enumerate(self.order)}
        a = G.arrays(m, self.order, self.mp_order)
        K = len(self.order); n_mp = len(self.mp_order)
        self.KF = corb.KeyFrameStore(K + 1, 2); self.MP = corb.MapPointStore(max(n_mp, 1), 4)
        meta = np.zeros(K, corb.KF_META_DTYPE); meta["id"] = a["kf_ids"]; meta["nlevels"] = 8
        for s, k in enumerate(self.order):
            kf = m.kfs[k]
            meta["Tcw"][s] = kf.Tcw.reshape(16); meta["TcwGBA"][s] = kf.TcwGBA.reshape(16); meta["ba_global_for_kf"][s] = kf.ba_global
        self.KF.put_batch(0, meta, a["feat_off"], np.zeros(len(a["mp_id"]), corb.KP_DTYPE), None, a["u_right"], a["depth"], a["mp_id"])
        rec = np.zeros(n_mp, corb.MP_RECORD_DTYPE); rec["id"] = a["mp_ids"]; rec["flags"] = a["mp_bad"].astype(np.uint32)
        for s, p in enumerate(self.mp_order):
            mp = m.mps[p]
            rec["world_pos"][s] = mp.pos; rec["pos_gba"][s] = mp.pos_gba; rec["ba_global_for_kf"][s] = mp.ba_global
            rec["ref_kf_id"][s] = NO_ID if mp.ref_kf is None else mp.ref_kf
        if n_mp:
            self.MP.put(0, rec, a["obs_off"], a["obs_kf"], a["obs_idx"])
        self.MP.build_index(0, n_mp)
        self.g = corb.Covisibility(self.KF, self.MP, M)
        eye = np.eye(4, dtype=np.float32)
        for s, k in enumerate(self.order):
            kf = m.kfs[k]
            if kf.children or kf.parent is not None:
                self.g.SetTree(s, NO_ID if kf.parent is None else kf.parent, kf.first, sorted(kf.children))
            if not np.array_equal(kf.TcwBef, eye):
                self.g.SetPoseBeforeGBA(s, kf.TcwBef)

    def state(self):
        """everything the call may write, as bytes: per slot the whole header and mTcwBefGBA, and every map-point record"""
        K = len(self.order)
        kfs = [(self.KF.get_meta(s).tobytes(), self.g.GetPoseBeforeGBA(s).tobytes()) for s in range(K + 1)]
        rec, okf, oidx = self.MP.get(0, max(len(self.mp_order), 1))
        return kfs, rec.tobytes(), okf.tobytes(), oidx.tobytes(), [self.g.GetTree(s)[0] for s in range(K)]

    def compare(self):
        for s, k in enumerate(self.order):
            kf = self.m.kfs[k]; meta = self.KF.get_meta(s)
            assert np.array_equal(meta["Tcw"].reshape(4, 4), kf.Tcw), ("Tcw", s, k)
            assert np.array_equal(meta["TcwGBA"].reshape(4, 4), kf.TcwGBA), ("TcwGBA", s, k)
            assert int(meta["ba_global_for_kf"]) == kf.ba_global, ("mark", s, k)
            assert np.array_equal(self.g.GetPoseBeforeGBA(s), kf.TcwBef), ("TcwBef", s, k)
        if self.mp_order:
            rec, _, _ = self.MP.get(0, len(self.mp_order))
            want = np.stack([self.m.mps[p].pos for p in self.mp_order])
            bad = np.nonzero((rec["world_pos"] != want).any(axis=1))[0]
            assert len(bad) == 0, (bad[:8], rec["world_pos"][bad[:8]], want[bad[:8]])

    def close(self):
        self.g.close(); self.KF.close(); self.MP.close()


def fails_with(corb, code, fn, *args, **kw):
    with pytest.raises(corb.CorbError) as e:
        fn(*args, **kw)
    assert "(%d)" % code in str(e.value), str(e.value)


def test_a_fresh_graph_holds_the_identity_and_keeps_what_is_set(corb):
    m, origins, order = C.tree_map(seed=1, shape="chain", n=3)
    d = Dev(corb, m, order)
    g2 = corb.Covisibility(d.KF, d.MP)
    for s in range(4):
        assert np.array_equal(g2.GetPoseBeforeGBA(s), np.eye(4, dtype=np.float32))
    T = np.arange(16, dtype=np.float32).reshape(4, 4) / 8
    g2.SetPoseBeforeGBA(2, T)
    assert np.array_equal(g2.GetPoseBeforeGBA(2), T) and np.array_equal(g2.GetPoseBeforeGBA(1), np.eye(4, dtype=np.float32))
    g2.close()
    fails_with(corb, -1, d.g.GetPoseBeforeGBA, 4)
    fails_with(corb, -1, d.g.PropagateGlobalBA, [3], L)          # an empty slot as an origin
    d.close()


@pytest.mark.parametrize("name", sorted(C.GBA_CASES))
def test_propagate_equals_the_definition_bit_for_bit(corb, name):
    m, origins, order = C.tree_map(**C.GBA_CASES[name])
    d = Dev(corb, m, order)
    cap = 50000
    want = XR.gba_propagate(m, origins, L, cap)
    got = d.g.PropagateGlobalBA([d.slot[k] for k in origins], L, queue_cap=cap)
    assert {k: getattr(got, k) for k in COUNTS} == want
    d.compare()
    d.close()


def test_the_default_queue_cap_and_an_exact_one(corb):
    m, origins, order = C.tree_map(**C.GBA_CASES["chain70"])
    import copy
    m2 = copy.deepcopy(m)
    d = Dev(corb, m, order)
    want = XR.gba_propagate(m, origins, L, XR.default_queue_cap(len(order) + 1))
    got = d.g.PropagateGlobalBA([d.slot[k] for k in origins], L)
    assert got.n_popped == want["n_popped"] == 70
    d.compare(); d.close()
    d = Dev(corb, m2, order)
    before = d.state()
    fails_with(corb, -2, d.g.PropagateGlobalBA, [d.slot[k] for k in origins], L, queue_cap=69)
    assert d.state() == before
    got = d.g.PropagateGlobalBA([d.slot[k] for k in origins], L, queue_cap=70)
    XR.gba_propagate(m2, origins, L, 70)
    d.compare(); d.close()


def test_a_cyclic_child_set_is_a_capacity_error_and_nothing_changes(corb):
    m, origins, order = C.tree_map(**C.CYCLIC_CASE)
    d = Dev(corb, m, order)
    before = d.state()
    with pytest.raises(XR.CapacityError):
        XR.gba_propagate(m, origins, L, XR.default_queue_cap(len(order) + 1))
    fails_with(corb, -2, d.g.PropagateGlobalBA, [d.slot[k] for k in origins], L)
    assert d.state() == before
    d.compare()
    d.close()


def test_without_an_index_or_without_origins(corb):
    m, origins, order = C.tree_map(seed=2, shape="chain", n=4, n_points=10)
    d = Dev(corb, m, order)
    got = d.g.PropagateGlobalBA([], L)                           # no origin: the points still run
    want = XR.gba_propagate(m, [], L, 100)
    assert {k: getattr(got, k) for k in COUNTS} == want and got.n_popped == 0
    d.compare()
    rec, okf, oidx = d.MP.get(0, 1)
    d.MP.put(0, rec, np.array([0, 0], np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint32))      # a put invalidates the index
    fails_with(corb, -1, d.g.PropagateGlobalBA, [0], L)
    d.close()


# ---- CorrectLoop's propagation (corb_loop_correct_store) ---------------------------------------------------------------------------------------------------------
class LoopDev:
    """the maps of loopfix_cases.loop_map in the two stores (slots in a shuffled order), rows as the definition's UpdateConnections left them"""

    def __init__(self, corb, m, seed):
        rng = np.random.default_rng(seed)
        self.corb = corb; self.m = m
        self.order = [sorted(m.kfs)[i] for i in rng.permutation(len(m.kfs))]; self.mp_order = [sorted(m.mps)[i] for i in rng.permutation(len(m.mps))]
        self.slot = {k: s for s, k in enumerate(self.order)}
        a = G.arrays(m, self.order, self.mp_order)
        K = len(self.order); n_mp = len(self.mp_order)
        self.KF = corb.KeyFrameStore(K, 24); self.MP = corb.MapPointStore(n_mp, 8)
        meta = np.zeros(K, corb.KF_META_DTYPE); meta["id"] = a["kf_ids"]; meta["nlevels"] = 8
        for s, k in enumerate(self.order):
            meta["Tcw"][s] = m.kfs[k].Tcw.reshape(16); meta["TcwGBA"][s] = np.eye(4, dtype=np.float32).reshape(16)
        kp = np.zeros(len(a["mp_id"]), corb.KP_DTYPE); kp["octave"] = a["octave"]
        self.KF.put_batch(0, meta, a["feat_off"], kp, None, a["u_right"], a["depth"], a["mp_id"])
        rec = np.zeros(n_mp, corb.MP_RECORD_DTYPE); rec["id"] = a["mp_ids"]; rec["n_obs"] = np.diff(a["obs_off"]); rec["flags"] = a["mp_bad"].astype(np.uint32)
        sc = np.zeros(n_mp, corb.MP_SCRATCH_DTYPE)
        for s, p in enumerate(self.mp_order):
            mp = m.mps[p]
            rec["world_pos"][s] = mp.pos; rec["normal"][s] = mp.normal; rec["min_distance"][s] = mp.min_distance; rec["max_distance"][s] = mp.max_distance
            rec["ref_kf_id"][s] = NO_ID if mp.ref_kf is None else mp.ref_kf
            sc["corrected_by_kf"][s] = mp.corrected_by; sc["corrected_reference"][s] = mp.corrected_ref
        self.MP.put(0, rec, a["obs_off"], a["obs_kf"], a["obs_idx"]); self.MP.set_scratch(0, sc); self.MP.build_index(0, n_mp)
        self.g = corb.Covisibility(self.KF, self.MP, 64)
        self.g.UpdateConnections([self.slot[k] for k in sorted(m.kfs)], th=3)
        assert [list(r[1][0]) for r in self.rows()] == [[i for i, _ in m.kfs[k].ordered] for k in self.order]

    def rows(self):
        return [self.g.get(s) for s in range(len(self.order))]

    def state(self):
        rec, okf, oidx = self.MP.get(0, len(self.mp_order))
        return ([self.KF.get_meta(s).tobytes() for s in range(len(self.order))], rec.tobytes(), okf.tobytes(), oidx.tobytes(), self.MP.get_scratch(0, len(self.mp_order)).tobytes())

    def close(self):
        self.g.close(); self.KF.close(); self.MP.close()


def run_correct_loop(corb, seed, cur, scale, scale_factor, cap_delta=None):
    import copy
    m, cur_id = C.loop_map(seed, cur=cur)
    Scw = C.loop_scw(m, cur_id, seed, scale)
    d = LoopDev(corb, m, seed)
    before = copy.deepcopy(m)
    walk, co, nc, n_points = XR.correct_loop(m, cur_id, Scw, scale_factor)
    if cap_delta is not None and cap_delta < 0:
        state = d.state()
        fails_with(corb, -2, d.g.CorrectLoop, d.slot[cur_id], Scw, scale_factor, cap=len(walk) + cap_delta)
        assert d.state() == state
        d.close()
        return
    ks, gco, gnc, gn = d.g.CorrectLoop(d.slot[cur_id], Scw, scale_factor, cap=None if cap_delta is None else len(walk) + cap_delta)
    assert [d.order[s] for s in ks] == walk and gn == n_points
    for got, want in ((gco, co), (gnc, nc)):
        assert got.shape == want.shape and np.array_equal(got, want), np.abs(got - want).max()
    new_T = {}
    rec, okf, oidx = d.MP.get(0, len(d.mp_order))
    print("correct_loop seed %d scale %g: floats that differ from the definition at all: %d of %d pose entries, %d of %d coordinates; the doubles: %.3g relative"
          % (seed, scale, sum(int((d.KF.get_meta(d.slot[k])["Tcw"].reshape(4, 4) != m.kfs[k].Tcw).sum()) for k in walk), 16 * len(walk),
             sum(int((rec["world_pos"][s] != m.mps[p].pos).sum()) for s, p in enumerate(d.mp_order)), 3 * len(d.mp_order),
             max(np.abs(gco - co).max() / max(1.0, np.abs(co).max()), np.abs(gnc - nc).max() / max(1.0, np.abs(nc).max()))))
    for s, k in enumerate(d.order):
        meta = d.KF.get_meta(s); T = meta["Tcw"].reshape(4, 4); new_T[k] = T.copy()
        want = m.kfs[k].Tcw
        if k in walk:
            assert np.array_equal(T[3], [0, 0, 0, 1])
        assert np.array_equal(T, want), (k, T, want)
        assert int(meta["flags"]) == 0 and int(meta["ba_global_for_kf"]) == 0
    rec, okf, oidx = d.MP.get(0, len(d.mp_order)); sc = d.MP.get_scratch(0, len(d.mp_order))
    for s, p in enumerate(d.mp_order):
        mp = m.mps[p]; old = before.mps[p]
        assert (int(sc["corrected_by_kf"][s]), int(sc["corrected_reference"][s])) == (mp.corrected_by, mp.corrected_ref), p
        assert int(rec["flags"][s]) == int(mp.bad)
        moved = mp.corrected_ref != old.corrected_ref or mp.corrected_by != old.corrected_by
        if not moved:
            assert np.array_equal(rec["world_pos"][s], old.pos) and np.array_equal(rec["normal"][s], old.normal) and rec["max_distance"][s] == old.max_distance
            continue
        assert np.array_equal(rec["world_pos"][s], mp.pos), (p, rec["world_pos"][s], mp.pos)
        if scale_factor > 0:
            # normal and distances from the DEVICE's position and the mixture the rule prescribes: members before the corrector have their corrected pose
            w = walk.index(mp.corrected_ref)
            probe = copy.copy(mp); probe.pos = rec["world_pos"][s].copy(); probe.normal = old.normal; probe.min_distance = old.min_distance; probe.max_distance = old.max_distance
            XR.update_normal_and_depth(m, probe, lambda k: new_T[k] if k in walk and walk.index(k) < w else before.kfs[k].Tcw, scale_factor)
            for got, want in ((rec["normal"][s], probe.normal), (rec["min_distance"][s], probe.min_distance), (rec["max_distance"][s], probe.max_distance)):
                assert np.all(np.abs(np.asarray(got, np.float64) - want) <= 2e-7 + 2e-6 * np.abs(want)), (p, got, want)
        else:
            assert np.array_equal(rec["normal"][s], old.normal) and rec["min_distance"][s] == old.min_distance and rec["max_distance"][s] == old.max_distance
    d.close()


@pytest.mark.parametrize("scale", C.LOOP_SCALES)
@pytest.mark.parametrize("i", range(len(C.LOOP_SEEDS)))
def test_correct_loop_equals_the_definition(corb, i, scale):
    run_correct_loop(corb, C.LOOP_SEEDS[i], C.LOOP_CURS[i % 3], scale, 1.2)


def test_correct_loop_with_an_exact_cap_without_normals_and_with_a_cap_too_small(corb):
    run_correct_loop(corb, C.LOOP_SEEDS[0], "middle", 0.8, 0.0, cap_delta=0)
    run_correct_loop(corb, C.LOOP_SEEDS[1], "largest", 0.8, 1.2, cap_delta=-1)

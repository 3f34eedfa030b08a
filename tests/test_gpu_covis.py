"""GPU parity, bit for bit: the covisibility graph on store records (corb_covis_*) against tests/covis_reference.py.  Every case builds both stores from the seeded
maps of tests/covis_cases.py, runs the calls on the device and in Python, and compares corb_covis_get of EVERY row -- not only the touched ones -- with the Python state."""
import numpy as np
import pytest

import covis_reference as R
import covis_cases as G
import records_reference as RR

pytestmark = pytest.mark.gpu
M_SMALL = 100            # max_connections of the shape cases: rows of 100, sorted as 128


class Dev:
    """a map in the two stores (keyframe k of kf_order in slot k, map point p of mp_order in slot p) with a graph over them"""

    def __init__(self, corb, m, M=0, F=None, O=12, kf_order=None, mp_order=None):
        self.corb = corb; self.m = m
        a = self.a = G.arrays(m, kf_order, mp_order)
        self.kf_order = [int(i) for i in a["kf_ids"]]; self.mp_order = [int(i) for i in a["mp_ids"]]
        self.slot = {k: s for s, k in enumerate(self.kf_order)}; self.mp_slot = {p: s for s, p in enumerate(self.mp_order)}
        K = len(self.kf_order); n_mp = len(self.mp_order)
        F = int(np.diff(a["feat_off"]).max()) if F is None else F
        self.KF = corb.KeyFrameStore(K, F); self.MP = corb.MapPointStore(max(n_mp, 1), O)
        meta = np.zeros(K, corb.KF_META_DTYPE); meta["id"] = a["kf_ids"]; meta["flags"] = a["kf_bad"].astype(np.uint32); meta["nlevels"] = 8
        kp = np.zeros(len(a["mp_id"]), corb.KP_DTYPE); kp["octave"] = a["octave"]
        self.KF.put_batch(0, meta, a["feat_off"], kp, None, a["u_right"], a["depth"], a["mp_id"])
        self.put_points(0, n_mp)
        self.g = corb.Covisibility(self.KF, self.MP, M)

    def put_points(self, first, n):
        a = G.arrays(self.m, self.kf_order, self.mp_order[first: first + n])
        rec = np.zeros(n, self.corb.MP_RECORD_DTYPE); rec["id"] = a["mp_ids"]; rec["n_obs"] = np.diff(a["obs_off"]); rec["flags"] = a["mp_bad"].astype(np.uint32)
        if n:
            self.MP.put(first, rec, a["obs_off"], a["obs_kf"], a["obs_idx"])
        self.MP.build_index(0, len(self.mp_order))

    def update(self, kids, python=True):
        fp = self.g.UpdateConnections([self.slot[k] for k in kids])
        if python:
            want = [R.update_connections(self.m, k) for k in kids]
            assert [None if int(f) == G.NO_ID else int(f) for f in fp] == want
        return fp

    def rows(self):
        out = []
        for s in range(len(self.kf_order)):
            (ai, aw), (oi, ow) = self.g.get(s)
            out.append((([int(i) for i in ai], [int(w) for w in aw]), ([int(i) for i in oi], [int(w) for w in ow])))
        return out

    def check(self):
        got = self.rows(); want = G.rows(self.m, self.kf_order)
        for s, (g, w) in enumerate(zip(got, want)):
            assert g == w, (s, self.kf_order[s], g, w)

    def close(self):
        self.g.close(); self.KF.close(); self.MP.close()


def fails_with(corb, code, fn, *args):
    with pytest.raises(corb.CorbError) as e:
        fn(*args)
    assert "(%d)" % code in str(e.value), str(e.value)


# (features of the keyframe, observations per point, distinct other observers): 0 = empty counter, 100 = max_connections; the table fills at 101
SHAPES = [(1, 1, 0), (1, 2, 1), (63, 2, 63), (64, 2, 64), (65, 2, 65), (255, 8, 100), (256, 2, 1), (257, 8, 64), (2049, 2, 65), (2049, 8, 100)]


@pytest.mark.parametrize("F,obs,distinct", SHAPES)
def test_update_of_one_keyframe_at_every_shape(corb, F, obs, distinct):
    d = Dev(corb, G.star_map(F, obs, distinct), M=M_SMALL, O=8)             # obs = 8: max_observations
    d.update([100]); d.check()
    if distinct == 0:
        assert d.rows()[0] == (([], []), ([], []))               # "This should not happen": nothing changes
    else:
        assert len(d.rows()[0][0][0]) == distinct
    d.update([100]); d.check()                                   # again: every AddConnection returns early
    d.close()


def test_one_observer_too_many_is_a_capacity_error_and_the_graph_stays(corb):
    m = G.star_map(255, 8, M_SMALL)
    m.kfs[200].mp_ids = [10000]                                  # keyframe 200 holds the point it observes: a counter of its own
    d = Dev(corb, m, M=M_SMALL, O=9)
    d.update([100, 200]); d.check()
    before = d.rows()
    assert len(before[0][0][0]) == M_SMALL
    m.mps[10000].obs[777777] = 0                                  # the 101st id, on the record of the first point
    d.put_points(d.mp_slot[10000], 1)
    fails_with(corb, -2, d.g.UpdateConnections, [d.slot[200], d.slot[100]])      # the first member alone would pass: count first, commit after
    assert d.rows() == before
    d.close()


def test_a_point_held_at_two_features_votes_twice(corb):
    m = G.star_map(40, 2, 2)
    m.kfs[100].mp_ids[1] = m.kfs[100].mp_ids[0]
    m.kfs[200].mp_ids = [10000]; m.mps[10000].obs[200] = 0
    d = Dev(corb, m, M=M_SMALL)
    d.update([100]); d.check()
    assert R.get_weight(m, 100, 200) == 21                       # 20 points, one of them twice
    d.update([200]); d.check()                                   # 200 counts 100 once: the weight changes, the row of 100 lists everything
    assert m.kfs[100].ordered == R.descending([(w, i) for i, w in m.kfs[100].weights.items()])
    d.close()


def test_weights_14_15_16_side_by_side(corb):
    m = G.star_map(20, 1, 0, weights=[(300, 14), (305, 15), (310, 16)])
    d = Dev(corb, m, M=M_SMALL)
    d.update([100]); d.check()
    assert m.kfs[100].ordered == [(310, 16), (305, 15)] and m.kfs[100].weights[300] == 14
    d.close()


def test_colliding_ids_in_both_id_tables(corb):
    rng = np.random.default_rng(5)
    kw = dict(G.RANDOM_MAPS["k20"])
    kf_ids = np.sort(RR.colliding_ids(kw["n_kf"], RR.id_table_cells(kw["n_kf"]), rng))
    n_points = len(G.random_map(ids=kf_ids, **kw).mps)            # (the ids do not change the map's shape)
    mp_ids = RR.colliding_ids(n_points, RR.id_table_cells(n_points), rng)
    assert RR.probe_chain(kf_ids, RR.id_table_cells(len(kf_ids)))[1] > 0 and RR.probe_chain(mp_ids, RR.id_table_cells(n_points))[1] > 0
    d = Dev(corb, G.random_map(ids=kf_ids, point_ids=mp_ids, **kw))
    d.update(d.kf_order); d.check()
    d.close()


@pytest.mark.parametrize("name", sorted(G.RANDOM_MAPS))
@pytest.mark.parametrize("n", [1, 2, 17])
def test_batches_in_two_orders(corb, name, n):
    for order in (1, -1):
        m = G.random_map(**G.RANDOM_MAPS[name])
        kf_order = list(np.random.default_rng(3).permutation(sorted(m.kfs)))      # slots are not in id order
        d = Dev(corb, m, kf_order=kf_order)
        batch = sorted(m.kfs)[3: 3 + n][::order]
        d.update(batch); d.check()
        d.update(sorted(m.kfs)[::order]); d.check()              # then the whole map, over the rows the batch left
        d.close()


def test_single_calls_equal_one_batch(corb):
    kw = G.RANDOM_MAPS["k40_wide"]
    a = Dev(corb, G.random_map(**kw)); b = Dev(corb, G.random_map(**kw))
    kids = sorted(a.m.kfs)[::-1]
    fa = a.update(kids)
    fb = np.concatenate([b.update([k]) for k in kids])
    assert np.array_equal(fa, fb) and a.rows() == b.rows()
    a.check()
    a.close(); b.close()


def test_erase_then_update_again(corb):
    m = G.random_map(**G.RANDOM_MAPS["k20"])
    d = Dev(corb, m)
    d.update(sorted(m.kfs)[::2]); d.check()                      # every other keyframe: the rest hear of their neighbours through AddConnection alone
    # a keyframe one of whose neighbours never listed it (that neighbour's map has no entry to erase)
    pick = [k for k in sorted(m.kfs) if any(o in m.kfs and k not in m.kfs[o].weights for o in m.kfs[k].weights)]
    assert pick
    for k in (pick[0], sorted(m.kfs)[10]):
        R.erase_connections(m, k); d.g.EraseConnections(d.slot[k]); d.check()
        assert d.rows()[d.slot[k]] == (([], []), ([], []))
        d.update([k]); d.check()
    d.close()


def test_queries(corb):
    m = G.random_map(**G.RANDOM_MAPS["k20"])
    d = Dev(corb, m)
    d.update(sorted(m.kfs)); d.check()
    to_slots = lambda ids: [-1 if i is None else d.slot[i] for i in ids]
    everything_with_unknown = 0
    for k in sorted(m.kfs):
        s = d.slot[k]; kf = m.kfs[k]
        everything_with_unknown += len(kf.ordered) == len(kf.weights) and any(i not in m.kfs for i, _ in kf.ordered)
        assert list(d.g.GetVectorCovisibleKeyFrames(s)) == to_slots(R.get_vector_covisibles(m, k))
        for N in (1, 10, 500):
            assert list(d.g.GetBestCovisibilityKeyFrames(s, N)) == to_slots(R.get_best_covisibles(m, k, N))
        ws = sorted({w for _, w in kf.ordered})
        for w in {1, 15, 10 ** 6} | {x + dx for x in ws[:1] + ws[-1:] + ws[len(ws) // 2: len(ws) // 2 + 1] for dx in (-1, 0, 1) if x + dx > 0}:
            assert list(d.g.GetCovisiblesByWeight(s, w)) == to_slots(R.get_covisibles_by_weight(m, k, w)), (k, w)
        for o in list(m.kfs)[:6]:
            assert d.g.GetWeight(s, d.slot[o]) == R.get_weight(m, k, o)
        sl, w = d.g.query(s)
        assert [int(x) for x in w] == [wk for i, wk in kf.ordered if i in m.kfs]
    assert everything_with_unknown >= 1                          # a row in the "everything" state with an id the store does not hold
    fails_with(corb, -2, d.g.query, d.slot[sorted(m.kfs)[5]], 0, 0, 0)
    d.close()


@pytest.mark.parametrize("name", sorted(G.CULLING_MAPS))
def test_keyframe_culling(corb, name):
    kw = G.CULLING_MAPS[name]
    m = G.culling_map(**kw)
    d = Dev(corb, m)
    d.update([7]); d.check()
    assert len(R.get_vector_covisibles(m, 7)) == kw["n_cov"] + kw.get("n_helpers", 3)
    for mono in (False, True):
        want = R.keyframe_culling(m, 7, mono, 35.0)
        ks, nm, nr, cu = d.g.KeyFrameCulling(d.slot[7], mono, 35.0)
        got = [(d.kf_order[int(s)], int(a), int(b), bool(c)) for s, a, b, c in zip(ks, nm, nr, cu)]
        assert got == want
    d.close()


def window_slots(d, k):
    local, fixed, points = R.local_window(d.m, k)
    return [d.slot[i] for i in local] + [d.slot[i] for i in fixed], len(local), [d.mp_slot[p] for p in points]


@pytest.mark.parametrize("name", sorted(G.RANDOM_MAPS))
def test_local_window_lists_in_the_reference_orders(corb, name):
    m = G.random_map(**G.RANDOM_MAPS[name])
    d = Dev(corb, m)
    d.update(sorted(m.kfs)); d.check()
    some_bad_covisible = 0
    for k in sorted(m.kfs)[::3]:
        ks, nl, ms = window_slots(d, k)
        some_bad_covisible += any(m.kfs[i].bad for i in R.get_vector_covisibles(m, k))
        got = d.g.LocalWindow(d.slot[k], len(ks), len(ms))       # the caps exactly enough
        assert (list(got[0]), got[1], list(got[2])) == (ks, nl, ms), k
        got = d.g.LocalWindow(d.slot[k], len(ks) + 7, len(ms) + 100)
        assert (list(got[0]), got[1], list(got[2])) == (ks, nl, ms), k
        fails_with(corb, -2, d.g.LocalWindow, d.slot[k], len(ks) - 1, len(ms))
        if ms:
            fails_with(corb, -2, d.g.LocalWindow, d.slot[k], len(ks), len(ms) - 1)
    assert some_bad_covisible >= 1
    d.check()                                                    # a window writes nothing
    d.close()


def _lba_stores(corb, synth, seed):
    """a synthetic local window (synth.local_ba_problem) in the stores, as tests/test_gpu_local_ba_store.py builds it, and the same map as a covis_reference.Map"""
    prob = synth.local_ba_problem(seed=seed, n_local=6, n_fixed=4, pts_per_kf=140, outlier_frac=0.12, max_obs=5)
    cm = synth.client_maps(prob, 1, 10)[0]
    F = max(len(k["kp"]) for k in cm["kf"]) + 3
    KF = corb.KeyFrameStore(10, F); MP = corb.MapPointStore(len(cm["mp_records"]), 16)
    m = R.Map()
    for s, k in enumerate(cm["kf"]):
        KF.put(s, k["kp"], k["desc"], k["ur"], None, keyframe_id=k["id"])
        cam = k["cam"]
        KF.set_meta(s, id=k["id"], client_id=1, flags=0, fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3], bf=cam[4], nlevels=8, Tcw=k["Tcw"].reshape(16),
                    inv_level_sigma2=np.concatenate([k["inv_level_sigma2"], np.zeros(8, np.float32)]))
        KF.set_map_points(s, k["mp_id"])
        m.kfs[int(k["id"])] = R.KeyFrame(int(k["id"]), [int(x) for x in k["mp_id"]], octave=k["kp"]["octave"].tolist(), u_right=k["ur"].tolist())
    rec, off = cm["mp_records"], cm["obs_off"]
    MP.put(0, rec, off, cm["obs_kf"], cm["obs_idx"]); MP.build_index(0, len(rec))
    for j in range(len(rec)):
        m.mps[int(rec["id"][j])] = R.MapPoint(int(rec["id"][j]), {int(cm["obs_kf"][t]): int(cm["obs_idx"][t]) for t in range(off[j], off[j + 1])})
    return KF, MP, m, [int(k["id"]) for k in cm["kf"]], [int(x) for x in rec["id"]]


def test_the_window_feeds_local_bundle_adjustment(corb, synth):
    out = []
    for route in ("device", "python"):
        KF, MP, m, kf_order, mp_order = _lba_stores(corb, synth, 2103)
        slot = {k: s for s, k in enumerate(kf_order)}; mp_slot = {p: s for s, p in enumerate(mp_order)}
        for k in kf_order:
            R.update_connections(m, k)
        local, fixed, points = R.local_window(m, kf_order[0])
        want = ([slot[i] for i in local + fixed], len(local), [mp_slot[p] for p in points])
        if route == "device":
            g = corb.Covisibility(KF, MP)
            g.UpdateConnections(np.arange(len(kf_order)))
            ks, nl, ms = g.LocalWindow(0, len(kf_order), len(mp_order))
            assert (list(ks), nl, list(ms)) == want
            g.close()
        else:
            ks, nl, ms = np.array(want[0], np.int32), want[1], np.array(want[2], np.int32)
        assert nl >= 2 and len(ms) > 100
        r = corb.LocalBundleAdjustmentStore(KF, ks, nl, MP, ms, scale_factor=1.2)
        out.append((r["poses"].tobytes(), r["points"].tobytes(), r["erase"].tobytes(), MP.get(0, len(mp_order))[0].tobytes()))
        KF.close(); MP.close()
    assert out[0] == out[1]


def test_a_full_row_of_a_neighbour_is_reported_not_overrun(corb):
    """max_connections = 2: keyframe 1 shares 16 points with each of 2, 3 and 4, which are updated one after the other -- the third AddConnection finds the row of 1 full"""
    m = R.Map()
    feats = {k: [] for k in (1, 2, 3, 4)}
    for k in (2, 3, 4):
        for _ in range(16):
            pid = 100 * k + len(feats[k])
            m.mps[pid] = R.MapPoint(pid, {1: len(feats[1]), k: len(feats[k])}); feats[1].append(pid); feats[k].append(pid)
    for k in feats:
        m.kfs[k] = R.KeyFrame(k, feats[k])
    d = Dev(corb, m, M=2)
    d.update([2, 3]); d.check()
    fails_with(corb, -5, d.g.UpdateConnections, [d.slot[4]])
    rows = d.rows()
    assert rows[d.slot[1]] == (([3, 2], [16, 16]), ([3, 2], [16, 16]))                      # untouched: no entry beyond the row
    assert rows[d.slot[4]] == (([1], [16]), ([1], [16]))                                    # the keyframe's own row is committed
    fails_with(corb, -2, d.g.UpdateConnections, [d.slot[1]])                                # and its own counter holds three ids: the capacity error, nothing written
    assert d.rows() == rows
    d.close()

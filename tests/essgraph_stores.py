"""The cases of tests/essgraph_cases.py in the two stores with a covisibility graph over them: rows as the definition's UpdateConnections left them, the tree, the
loop-edge sets, flags, poses, points and the two scratch fields OptimizeEssentialGraph reads.  The last keyframe slot stays EMPTY: it stands for every keyframe the
store does not hold (a loop-connection member, say)."""
import numpy as np

import covis_cases as G
import localmap_reference as LR
import loopfix_reference as XR
import essgraph_reference as ER

NO_ID = XR.NO_ID


class Dev:
    def __init__(self, corb, case, seed=0, th=3, max_obs=8, M=64, index=True):
        rng = np.random.default_rng(seed)
        m = case.m
        self.corb = corb; self.case = case; self.m = m
        self.order = [sorted(m.kfs)[i] for i in rng.permutation(len(m.kfs))]; self.mp_order = [sorted(m.mps)[i] for i in rng.permutation(len(m.mps))]
        self.slot = {k: s for s, k in enumerate(self.order)}
        K = len(self.order); n_mp = len(self.mp_order); self.K = K; self.empty_slot = K
        a = G.arrays(m, self.order, self.mp_order)
        F = max(len(m.kfs[k].mp_ids) for k in self.order)
        self.KF = corb.KeyFrameStore(K + 1, F); self.MP = corb.MapPointStore(n_mp, max_obs)
        meta = np.zeros(K, corb.KF_META_DTYPE); meta["id"] = a["kf_ids"]; meta["nlevels"] = 8
        for s, k in enumerate(self.order):
            meta["Tcw"][s] = m.kfs[k].Tcw.reshape(16); meta["TcwGBA"][s] = np.eye(4, dtype=np.float32).reshape(16)
        kp = np.zeros(len(a["mp_id"]), corb.KP_DTYPE); kp["octave"] = a["octave"]
        self.KF.put_batch(0, meta, a["feat_off"], kp, None, a["u_right"], a["depth"], a["mp_id"])
        rec = np.zeros(n_mp, corb.MP_RECORD_DTYPE); rec["id"] = a["mp_ids"]; rec["n_obs"] = np.diff(a["obs_off"])
        sc = np.zeros(n_mp, corb.MP_SCRATCH_DTYPE)
        for s, p in enumerate(self.mp_order):
            mp = XR.loop_point(m.mps[p])
            rec["flags"][s] = (1 if mp.bad else 0) | (2 if getattr(mp, "fixed", False) else 0)
            rec["world_pos"][s] = mp.pos; rec["normal"][s] = mp.normal; rec["min_distance"][s] = mp.min_distance; rec["max_distance"][s] = mp.max_distance
            rec["ref_kf_id"][s] = NO_ID if mp.ref_kf is None else mp.ref_kf
            sc["corrected_by_kf"][s] = mp.corrected_by; sc["corrected_reference"][s] = mp.corrected_ref
        self.MP.put(0, rec, a["obs_off"], a["obs_kf"], a["obs_idx"]); self.MP.set_scratch(0, sc)
        if index:
            self.MP.build_index(0, n_mp)
        self.g = corb.Covisibility(self.KF, self.MP, M)
        if index:
            # the rows: the definition connected every keyframe once, in ascending id, before any keyframe went bad
            self.g.UpdateConnections([self.slot[k] for k in sorted(m.kfs)], th=th)
            assert [list(self.g.get(s)[1][0]) for s in range(K)] == [[i for i, _ in m.kfs[k].ordered] for k in self.order]
        for s, k in enumerate(self.order):
            kf = LR.tree(ER.node(m.kfs[k]))
            self.g.SetTree(s, NO_ID if kf.parent is None else kf.parent, kf.first, sorted(kf.children))
            flags = (1 if kf.bad else 0) | (2 if kf.fixed else 0)
            if flags:
                self.KF.set_meta(s, flags=flags)

    def add_loop_edges(self):
        """the definition's sets through corb_covis_add_loop_edge, in descending id (the call sorts)"""
        for s, k in enumerate(self.order):
            for l in sorted(self.m.kfs[k].loop_edges, reverse=True):
                self.g.AddLoopEdge(s, self.slot[l])

    def slot_of(self, kid):
        return self.slot.get(kid, self.empty_slot)

    def args(self, min_weight):
        """the arguments of Covisibility.EssentialGraphPlan / OptimizeEssentialGraph for the case"""
        c = self.case
        ks = sorted(c.corrected)
        co = np.array([c.corrected[k] for k in ks], np.float64).reshape(len(ks), 8); nc = np.array([c.non_corrected[k] for k in ks], np.float64).reshape(len(ks), 8)
        lc = [(self.slot_of(k), [self.slot_of(j) for j in sorted(v)]) for k, v in c.loop_connections.items()]
        return dict(loop_slot=self.slot[c.loop_id], cur_slot=self.slot[c.cur_id], corr_slots=[self.slot[k] for k in ks], corrected=co, non_corrected=nc,
                    loop_connections=lc, min_weight=min_weight)

    def state(self):
        """every byte a call could write: headers, features' map-point ids, rows, trees, loop edges, mTcwBefGBA, map-point records, observation lists, scratch"""
        K = self.K
        kfs = [(self.KF.get_meta(s).tobytes(), self.KF.get_map_points(s).tobytes() if s < K else b"", self.g.GetPoseBeforeGBA(s).tobytes(),
                [x.tobytes() for pair in self.g.get(s) for x in pair], self.g.GetTree(s)[0], self.g.GetTree(s)[2].tobytes(), self.g.GetLoopEdges(s).tobytes()) for s in range(K + 1)]
        rec, okf, oidx = self.MP.get(0, len(self.mp_order))
        return kfs, rec.tobytes(), okf.tobytes(), oidx.tobytes(), self.MP.get_scratch(0, len(self.mp_order)).tobytes()

    def records(self):
        rec, _, _ = self.MP.get(0, len(self.mp_order))
        return [self.KF.get_meta(s) for s in range(self.K)], rec

    def close(self):
        self.g.close(); self.KF.close(); self.MP.close()


def compare_plan(dev, got, want):
    """v_slots, fixed, vi, vj, kind and the counts EQUAL; S, snc and the measurements equal as well (IEEE operations, uncontracted, in one order on both sides)"""
    assert [dev.order[s] for s in got["v_slots"]] == want["v_ids"]
    assert got["counts"] == want["counts"], (got["counts"], want["counts"])
    for k in ("fixed", "vi", "vj", "kind"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("S", "snc", "meas"):
        assert got[k].shape == want[k].shape
        if not np.array_equal(got[k], want[k]):
            rel = np.abs(got[k] - want[k]).max() / max(1.0, np.abs(want[k]).max())
            print("essential graph plan: %s differs from the definition by %.3g relative" % (k, rel))
            assert np.array_equal(got[k], want[k]), (k, rel)

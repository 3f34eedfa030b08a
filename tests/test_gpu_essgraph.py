"""GPU parity of Optimizer::OptimizeEssentialGraph on records (include/corb_essential_graph.h) against tests/essgraph_reference.py: the loop-edge sets, the plan
(corb_essential_graph_plan) and the whole call (corb_essential_graph_store) on the seeded cases of tests/essgraph_cases.py, the hand-written map and the hub.

Bars.  The plan's integers are EQUAL; so are S, snc and the measurements: IEEE +, -, x, / and sqrt in one order on both sides, nothing contracted (the finding of
tests/test_gpu_loopfix.py for the same algebra; a case that differed would be allowed that file's 1e-12 relative and be named in the commit message -- none does).
The records route and corb_optimize_essential_graph fed the plan's arrays run the same kernels on the same inputs in the same edge order: chi2, iterations, the final
estimates, every committed pose and every position are equal byte for byte.  Against the oracle the bars are tests/test_gpu_graph.py's (RTOL, its chi2 rules);
normal and distances keep the project's 2e-7 absolute, 2e-6 relative."""
import copy
import ctypes as C

import numpy as np
import pytest

import essgraph_cases as EC
import essgraph_reference as ER
import essgraph_stores as ES
import loopfix_reference as XR
from test_gpu_graph import RTOL

pytestmark = pytest.mark.gpu
NO_ID = XR.NO_ID


def fails_with(corb, code, fn, *args, **kw):
    with pytest.raises(corb.CorbError) as e:
        fn(*args, **kw)
    assert "(%d)" % code in str(e.value), str(e.value)


def make(corb, case, seed=0, **kw):
    d = ES.Dev(corb, case, seed, **kw)
    d.add_loop_edges()
    return d


def test_loop_edges_add_get_duplicate_clear_and_capacity(corb):
    c = EC.hub(40)
    for kf in c.m.kfs.values():
        kf.loop_edges = set()
    d = ES.Dev(corb, c, 3, th=1, max_obs=72, M=128)
    K = d.K
    assert all(len(d.g.GetLoopEdges(s)) == 0 for s in range(K + 1))                              # a fresh graph holds empty sets
    s0 = d.slot[10]
    for k in (40, 12, 30):
        d.g.AddLoopEdge(s0, d.slot[k])
    assert d.g.GetLoopEdges(s0).tolist() == [12, 30, 40]                                         # ascending id, one direction per call
    assert len(d.g.GetLoopEdges(d.slot[12])) == 0
    d.g.AddLoopEdge(s0, d.slot[30])
    assert d.g.GetLoopEdges(s0).tolist() == [12, 30, 40]
    fails_with(corb, -2, d.g.GetLoopEdges, s0, cap=2)
    fails_with(corb, -1, d.g.AddLoopEdge, s0, d.empty_slot)                                      # no keyframe there
    fails_with(corb, -1, d.g.AddLoopEdge, K + 1, 0)
    d.g.ClearLoopEdges(s0)
    assert len(d.g.GetLoopEdges(s0)) == 0
    others = [k for k in sorted(c.m.kfs) if k != 10]
    for k in others[:32][::-1]:
        d.g.AddLoopEdge(s0, d.slot[k])
    full = d.g.GetLoopEdges(s0)
    assert full.tolist() == others[:32]
    before = d.state()
    fails_with(corb, -2, d.g.AddLoopEdge, s0, d.slot[others[32]])                                # the 33rd id
    assert d.state() == before and np.array_equal(d.g.GetLoopEdges(s0), full)
    d.g.AddLoopEdge(s0, d.slot[others[5]])                                                       # a present id in a full set: nothing happens
    assert d.state() == before
    g2 = corb.Covisibility(d.KF, d.MP, 128)
    assert all(len(g2.GetLoopEdges(s)) == 0 for s in range(K + 1))
    g2.close(); d.close()


def host_route(corb, p, d, cur_id, fix_scale):
    """corb_optimize_essential_graph fed the plan's arrays, with the points the records route moves (the same vertex choice per point)"""
    rec = d.MP.get(0, len(d.mp_order))[0]; sc = d.MP.get_scratch(0, len(d.mp_order))
    rank = {int(s): r for r, s in enumerate(p["v_slots"])}
    ref = np.full(len(rec), -1, np.int32)
    for i in range(len(rec)):
        if int(rec["flags"][i]) & 3:
            continue
        idr = int(sc["corrected_reference"][i]) if int(sc["corrected_by_kf"][i]) == cur_id else int(rec["ref_kf_id"][i])
        if idr != NO_ID and idr in d.slot:
            ref[i] = rank.get(d.slot[idr], -1)
    g = dict(S=p["S"], fixed=p["fixed"], vi=p["vi"], vj=p["vj"], meas=p["meas"], points=rec["world_pos"].copy(), ref=ref)
    return corb.Optimizer.OptimizeEssentialGraph(g, 20, fix_scale), ref


def check_commit(d, m, before_meta, before_rec, p, S_final, result, moved, n, scale_factor, old):
    """the records after the call against the definition's map m (committed with the DEVICE's final estimates) and against the records before it"""
    metas, rec = d.records()
    assert {k: getattr(result, k) for k in n} == n
    for s, k in enumerate(d.order):
        want = copy.deepcopy(before_meta[s]); want["Tcw"] = m.kfs[k].Tcw.reshape(16)
        assert np.array_equal(metas[s]["Tcw"].reshape(4, 4), m.kfs[k].Tcw), (k, metas[s]["Tcw"], m.kfs[k].Tcw)
        assert metas[s].tobytes() == want.tobytes(), k                                           # nothing but Tcw
    want = before_rec.copy()
    for s, pid in enumerate(d.mp_order):
        mp = m.mps[pid]
        if pid not in moved:
            continue
        assert np.array_equal(rec["world_pos"][s], mp.pos), (pid, rec["world_pos"][s], mp.pos)
        want["world_pos"][s] = mp.pos
        if scale_factor > 0:
            probe = copy.copy(old.mps[pid]); probe.pos = rec["world_pos"][s].copy()
            XR.update_normal_and_depth(m, probe, lambda k: m.kfs[k].Tcw, scale_factor)
            for got, w in ((rec["normal"][s], probe.normal), (rec["min_distance"][s], probe.min_distance), (rec["max_distance"][s], probe.max_distance)):
                assert np.all(np.abs(np.asarray(got, np.float64) - w) <= 2e-7 + 2e-6 * np.abs(w)), (pid, got, w)
            for f in ("normal", "min_distance", "max_distance"):
                want[f][s] = rec[f][s]
    assert rec.tobytes() == want.tobytes()                                                       # nothing but the moved points' position, normal and distances


def run_case(corb, case, seed, min_weight, fix_scale, scale_factor, oracle=None, **kw):
    d = make(corb, case, seed, **kw)
    m = case.m
    want = ER.plan(m, **case.inputs(min_weight))
    state = d.state()
    p = d.g.EssentialGraphPlan(**d.args(min_weight))
    ES.compare_plan(d, p, want)
    assert d.state() == state                                                                    # the plan is pure
    if min_weight == 100:
        assert want["counts"]["n_kind"][3] == 0 and want["counts"]["n_kind"][0] <= 1
    host, ref = host_route(corb, p, d, case.cur_id, fix_scale)
    before_meta, before_rec = d.records()
    out = d.g.OptimizeEssentialGraph(bFixScale=fix_scale, iterations=20, scale_factor=scale_factor, **d.args(min_weight))
    r = out["result"]
    assert r.graph.as_dict() == want["counts"]
    # records route = host-array route, byte for byte
    assert r.iters_done == host["iters_done"] and out["chi2"].tobytes() == host["chi2"].tobytes() and out["S"].tobytes() == host["S"].tobytes()
    metas, rec = d.records()
    for rk, s in enumerate(p["v_slots"]):
        if not int(before_meta[s]["flags"]) & 2:
            assert metas[s]["Tcw"].tobytes() == host["Tiw"][rk].tobytes(), (rk, s)
        else:
            assert metas[s]["Tcw"].tobytes() == before_meta[s]["Tcw"].tobytes()
    assert rec["world_pos"].tobytes() == host["points"].tobytes()
    # ... = the definition's commit with these final estimates
    old = copy.deepcopy(m)
    n, moved = ER.commit(m, want, out["S"], case.cur_id, 0.0)
    check_commit(d, m, before_meta, before_rec, want, out["S"], r, moved, n, scale_factor, old)
    after = d.state()
    assert after[0] != state[0] and [x[1:] for x in after[0]] == [x[1:] for x in state[0]] and after[2:] == state[2:]      # rows, trees, loop edges, lists, scratch
    if oracle is not None:
        g = dict(S=want["S"], fixed=want["fixed"], vi=want["vi"], vj=want["vj"], meas=want["meas"], points=before_rec["world_pos"].copy(), ref=ref)
        R = oracle.optimize_essential_graph(g, 20, fix_scale)
        k = min(len(out["chi2"]), len(R["chi2"]))
        assert np.allclose(out["chi2"][:k], R["chi2"][:k], rtol=0, atol=1e-3 * R["chi2"][0])
        assert np.allclose(out["chi2"][:2], R["chi2"][:2], rtol=1e-4)
        assert abs(out["chi2"][-1] - R["chi2"][-1]) <= 1e-3 * R["chi2"][0]
        assert np.abs(out["S"] - R["S"]).max() <= RTOL * max(1.0, np.abs(R["S"]).max())
        free = [rk for rk, s in enumerate(p["v_slots"]) if not int(before_meta[s]["flags"]) & 2]
        T = np.stack([metas[p["v_slots"][rk]]["Tcw"].reshape(4, 4) for rk in free])
        assert np.abs(T - R["Tiw"][free]).max() <= RTOL * max(1.0, np.abs(R["Tiw"]).max())
        assert np.abs(rec["world_pos"] - R["points"]).max() <= RTOL * max(1.0, np.abs(R["points"]).max())
    d.close()
    return out


@pytest.mark.parametrize("min_weight", (3, 100))
@pytest.mark.parametrize("fix_scale", (False, True))
@pytest.mark.parametrize("seed", EC.SEEDS)
def test_plan_and_store_equal_the_definition_and_the_host_array_route(corb, seed, fix_scale, min_weight):
    run_case(corb, EC.seeded(seed), seed, min_weight, fix_scale, 1.2 if seed % 2 else 0.0)


def test_the_hand_written_map(corb):
    c = EC.hand_map()
    d = make(corb, c, 1, th=1)
    p = d.g.EssentialGraphPlan(**d.args(EC.HAND_MIN_WEIGHT))
    assert list(zip(p["vi"].tolist(), p["vj"].tolist(), p["kind"].tolist())) == EC.HAND_EDGES and p["counts"] == EC.HAND_COUNTS
    ES.compare_plan(d, p, ER.plan(c.m, **c.inputs(EC.HAND_MIN_WEIGHT)))
    d.close()


def test_the_hub_crosses_a_64_lane_round(corb):
    c = EC.hub()
    want = ER.plan(c.m, **c.inputs(3))
    newest = want["v_ids"].index(c.cur_id)
    assert int(((want["vi"] == newest) & (want["kind"] == 3)).sum()) > 64
    run_case(corb, EC.hub(), 5, 3, False, 1.2, th=1, max_obs=72, M=128)


@pytest.mark.parametrize("fix_scale", (False, True))
@pytest.mark.parametrize("seed", EC.SEEDS[:3])
def test_against_the_oracle(corb, pyorc, seed, fix_scale):
    run_case(corb, EC.seeded(seed), seed, 3, fix_scale, 1.2, oracle=pyorc)


def raw_plan(corb, d, min_weight, v_cap, e_cap):
    inp, keep = d.g._essential_graph_input(**d.args(min_weight))
    K = max(v_cap, 1) + 4; E = max(e_cap, 1) + 4
    arrays = [np.full(K, 0x55, np.int32), np.full((K, 8), 7.0), np.full(K, 0x55, np.uint8), np.full((K, 8), 7.0), np.full(E, 0x55, np.int32), np.full(E, 0x55, np.int32),
              np.full(E, 0x55, np.uint8), np.full((E, 8), 7.0)]
    cnt = corb.EssentialGraphCounts()
    rc = corb.load().corb_essential_graph_plan(d.g.h, C.byref(inp), v_cap, e_cap, *[a.ctypes.data_as(C.c_void_p) for a in arrays], C.byref(cnt))
    return rc, cnt.as_dict(), arrays


def test_caps_one_too_small_and_a_missing_index_write_nothing(corb):
    c = EC.seeded(EC.SEEDS[1])
    d = make(corb, c, 2)
    want = ER.plan(c.m, **c.inputs(3))
    K, E = want["counts"]["n_vertices"], want["counts"]["n_edges"]
    state = d.state()
    for v_cap, e_cap in ((K - 1, E), (K, E - 1)):
        rc, cnt, arrays = raw_plan(corb, d, 3, v_cap, e_cap)
        assert rc == -2 and cnt == want["counts"]
        assert all((a == (7.0 if a.dtype == np.float64 else 0x55)).all() for a in arrays)
    rc, cnt, arrays = raw_plan(corb, d, 3, K, E)
    assert rc == 0 and cnt == want["counts"] and np.array_equal(arrays[4][:E], want["vi"]) and (arrays[4][E:] == 0x55).all() and (arrays[1][K:] == 7.0).all()
    fails_with(corb, -2, d.g.OptimizeEssentialGraph, v_cap=K - 1, **d.args(3))
    assert d.g.last_result.graph.as_dict() == want["counts"] and d.state() == state
    a = d.args(3); a["corr_slots"] = list(a["corr_slots"][:-1]) + [a["corr_slots"][0]]
    fails_with(corb, -1, d.g.EssentialGraphPlan, **a)                                             # a slot twice
    rec, okf, oidx = d.MP.get(0, 1)
    d.MP.put(0, rec, np.array([0, int(rec["n_obs"][0])], np.int32), okf[0, :int(rec["n_obs"][0])], oidx[0, :int(rec["n_obs"][0])])      # a put invalidates the index
    state = d.state()
    fails_with(corb, -1, d.g.OptimizeEssentialGraph, **d.args(3))
    fails_with(corb, -1, d.g.EssentialGraphPlan, **d.args(3))
    assert d.state() == state
    d.close()


def test_a_dirty_workspace_and_repeated_runs_give_the_same_bytes(corb):
    """fresh arena, warm arena, lane 1 filled with a pattern (corb_scratch_fill), and the last state twice"""
    outs = []
    for state in ("fresh", "warm", "pattern", "pattern"):
        c = EC.seeded(EC.SEEDS[2])
        d = make(corb, c, 4)
        if state == "fresh":
            corb.release_scratch(0)
        if state == "pattern":
            corb.scratch_fill(1, 0x3F800000, 64 << 20); corb.scratch_fill(0, 0x3F800000, 8 << 20)
        p = d.g.EssentialGraphPlan(**d.args(3))
        o = d.g.OptimizeEssentialGraph(scale_factor=1.2, **d.args(3))
        metas, rec = d.records()
        outs.append((b"".join(p[k].tobytes() for k in ("v_slots", "S", "fixed", "snc", "vi", "vj", "kind", "meas")), p["counts"], o["chi2"].tobytes(), o["S"].tobytes(),
                     bytes(o["result"]), b"".join(x.tobytes() for x in metas), rec.tobytes()))
        d.close()
    for o in outs[1:]:
        assert o == outs[0]

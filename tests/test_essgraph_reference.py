"""The definition of Optimizer::OptimizeEssentialGraph on records (tests/essgraph_reference.py) checked without a GPU: a hand-written map whose edge list is written
out in tests/essgraph_cases.py, a consistent graph whose every measurement the oracle finds satisfied, the events the seeded cases must reach, and the exports."""
import collections
import os
import re

import numpy as np

import essgraph_cases as EC
import essgraph_reference as ER
import loopfix_reference as XR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_hand_written_map_gives_the_hand_written_edges():
    c = EC.hand_map()
    p = ER.plan(c.m, **c.inputs(EC.HAND_MIN_WEIGHT))
    assert p["v_ids"] == [1, 2, 4, 5] and p["fixed"].tolist() == [1, 1, 0, 0]
    assert list(zip(p["vi"].tolist(), p["vj"].tolist(), p["kind"].tolist())) == EC.HAND_EDGES
    assert p["counts"] == EC.HAND_COUNTS
    assert all(x > 0 for x in p["counts"]["n_kind"]) and all(x > 0 for x in p["counts"]["n_suppressed"])
    assert c.m.stats["lc_kept_by_exemption"] == 1 and c.m.stats["lc_below_weight"] == 1 and c.m.stats["dropped_own_bad"] == 1
    # vertices: Corrected where listed, else the pose; normal edges measure with NonCorrected where listed, loop connections with the vertex values
    for r, k in enumerate(p["v_ids"]):
        pose = XR.sim3_vec(XR.sim3_from_pose(c.m.kfs[k].Tcw))
        assert np.array_equal(p["S"][r], c.corrected[k] if k in c.corrected else pose)
        assert np.array_equal(p["snc"][r], c.non_corrected[k] if k in c.non_corrected else pose)
    for e, (vi, vj, kind) in enumerate(EC.HAND_EDGES):
        src = p["S"] if kind == 0 else p["snc"]
        assert np.array_equal(p["meas"][e], ER.measure(src[vi], src[vj]))
    assert not np.array_equal(ER.measure(p["S"][3], p["S"][2]), p["meas"][5])                    # (5 -> 4 is a normal edge: the corrected values are not used)


def test_a_loop_edge_set_is_a_set_of_at_most_32():
    c = EC.hand_map()
    ER.add_loop_edge(c.m, 1, 2)
    assert c.m.kfs[1].loop_edges == {2}
    for k in range(100, 131):
        ER.add_loop_edge(c.m, 1, k)
    before = set(c.m.kfs[1].loop_edges)
    try:
        ER.add_loop_edge(c.m, 1, 999)
        assert False
    except ER.CapacityError:
        pass
    assert c.m.kfs[1].loop_edges == before and len(before) == 32


def test_a_consistent_graph_has_no_residual(pyorc):
    """no loop connection and Corrected = NonCorrected = the poses: every measurement is Sjw * Swi of the vertices, so the oracle's chi2 is 0 to rounding and
    the commit moves nothing by more than rounding.  "Rounding" here is the float32 rounding of the poses: a rotation matrix orthonormal to 2^-24 per entry gives a
    quaternion that is a unit one to a few 2^-24 only, g2o never renormalises it and inverts it by conjugation, so an edge's residual is a few 2^-24 in the rotation
    part and that times |t| in the translation part.  The bound: 7 components per edge, each below 8 x 2^-24 x max(1, |t|)."""
    c = EC.seeded(EC.SEEDS[0])
    m = c.m
    pose = {k: XR.sim3_vec(XR.sim3_from_pose(m.kfs[k].Tcw)) for k in c.corrected}
    p = ER.plan(m, c.loop_id, c.cur_id, pose, pose, {}, 3)
    assert p["counts"]["n_kind"][0] == 0 and p["counts"]["n_edges"] > 10
    for e in range(len(p["vi"])):
        assert np.array_equal(p["meas"][e], ER.measure(p["S"][p["vi"][e]], p["S"][p["vj"][e]]))
    g = dict(S=p["S"], fixed=p["fixed"], vi=p["vi"], vj=p["vj"], meas=p["meas"], points=np.zeros((0, 3), np.float32), ref=np.zeros(0, np.int32))
    r = pyorc.optimize_essential_graph(g, 20, False)
    bound = len(p["vi"]) * 7 * (8 * 2.0 ** -24 * max(1.0, np.abs(p["S"][:, 4:7]).max())) ** 2
    print("consistent graph: chi2 %.3g -> %.3g, bound %.3g" % (r["chi2"][0], r["chi2"][-1], bound))
    assert r["chi2"][0] <= bound and r["chi2"][-1] <= r["chi2"][0]
    before = {pid: mp.pos.copy() for pid, mp in m.mps.items()}
    n, moved = ER.commit(m, p, r["S"], c.cur_id)
    assert n["n_points_moved"] == len(moved) > 0
    for pid in moved:
        assert np.abs(m.mps[pid].pos - before[pid]).max() <= 4e-6 * max(1.0, np.abs(before[pid]).max())


def test_the_seeded_cases_reach_every_event():
    stats = collections.Counter()
    for seed in EC.SEEDS:
        for min_weight in (3, 100):
            c = EC.seeded(seed)
            p = ER.plan(c.m, **c.inputs(min_weight))
            if min_weight == 100:                                   # only tree and loop edges plus the exempt pair remain
                assert p["counts"]["n_kind"][0] == (1 if c.loop_id in p["v_ids"] and c.cur_id in p["v_ids"] else 0) and p["counts"]["n_kind"][3] == 0
            n, moved = ER.commit(c.m, p, p["S"], c.cur_id)
            assert sum(n[k] for k in ("n_points_moved", "n_points_kept", "n_points_skipped")) > 0
            stats.update(c.m.stats)
    for k in ["kind_" + x for x in ER.KINDS] + ["suppressed_" + x for x in ER.SUPPRESSED] + ["dropped_lc_not_held", "dropped_lc_bad", "dropped_own_bad", "dropped_other_bad",
                                                                                             "lc_below_weight", "lc_kept_by_exemption", "point_corrected_reference",
                                                                                             "point_without_vertex", "point_fixed_reference", "point_no_reference"]:
        assert stats[k] > 0, (k, dict(stats))


def test_the_hub_emits_more_than_64_covisibility_edges_from_one_keyframe():
    c = EC.hub()
    p = ER.plan(c.m, **c.inputs(3))
    newest = p["v_ids"].index(c.cur_id)
    assert int(((p["vi"] == newest) & (p["kind"] == 3)).sum()) > 64


def test_every_export_is_declared_and_exported(corb):
    header = open(os.path.join(ROOT, "include", "corb_essential_graph.h")).read()
    L = corb.load()
    assert len(corb.ESSGRAPH_EXPORTS) == 5
    for name in corb.ESSGRAPH_EXPORTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(L, name), "libcorb_accel.so does not export %s" % name
    assert set(re.findall(r"\bint\s+(corb_\w+)\s*\(", header)) == set(corb.ESSGRAPH_EXPORTS)
    assert int(re.search(r"#define\s+CORB_COVIS_MAX_LOOP_EDGES\s+(\d+)", header).group(1)) == corb.Covisibility.MAX_LOOP_EDGES == 32

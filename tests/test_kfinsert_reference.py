"""CPU checks of the definition of keyframe insertion (tests/kfinsert_reference.py) and of the seeded cases (tests/kfinsert_cases.py): hand-worked answers for the
visit rule and the two duplicate rules, the closed form of the visit count against the serial loop, and the condition that the cases reach every kind and decision."""
import numpy as np
import pytest

import kfinsert_reference as R
import kfinsert_cases as G

TH = 35.0


def _depths(n_near, n_far, n_none=0):
    """near depths 1, 1 + 1/16, ... (below 35 up to 543 of them), then far depths, then features without depth; feature order = depth order"""
    return np.array([1.0 + 0.0625 * k for k in range(n_near)] + [40.0 + k for k in range(n_far)] + [-1.0] * n_none, np.float32)


@pytest.mark.parametrize("n_depth, want", [(0, 0), (1, 1), (99, 99), (100, 100), (101, 101), (102, 102), (257, 257)])
def test_all_near_depths_are_all_visited(n_depth, want):
    assert R.visit_order(_depths(n_depth, 0, 5), TH, 1) == list(range(want))
    assert R.visit_order(_depths(n_depth, 0, 5), TH, 2) == list(range(want))


@pytest.mark.parametrize("first_far, n_depth, want", [
    (0, 257, 101),          # every depth is far: the loop still visits 101 entries -- nPoints is tested after the increment
    (99, 257, 101),         # the far entry at sorted position 99 is entry number 100: not yet > 100
    (100, 257, 101),        # position 100 is entry number 101: the first that breaks, inclusive
    (101, 257, 102),
    (200, 257, 201),
    (0, 99, 99), (0, 100, 100), (0, 101, 101), (0, 102, 101), (99, 100, 100), (100, 101, 101), (101, 102, 102),
    (None, 257, 257),       # no far depth: all
])
def test_the_cut_is_the_first_far_entry_at_position_100_or_later_inclusive(first_far, n_depth, want):
    near = n_depth if first_far is None else first_far
    d = _depths(near, n_depth - near, 3)
    assert R.visit_order(d, TH, 1) == list(range(want))
    assert R.n_visited_closed_form(n_depth, near, 1) == want
    assert R.visit_order(d, TH, 0) == list(range(n_depth)) and R.n_visited_closed_form(n_depth, near, 0) == n_depth      # StereoInitialization takes every depth


def test_equal_depths_go_in_index_order_and_nan_and_inf_depths():
    d = np.array([3.0, 2.0, 3.0, np.nan, 2.0, np.inf, 0.0, -2.0, 3.0], np.float32)
    assert R.visit_order(d, TH, 1) == [1, 4, 0, 2, 8, 5]            # NaN fails z > 0; +inf is a depth, the last one
    assert R.visit_order(d, TH, 0) == [0, 1, 2, 4, 5, 8]
    assert R.visit_order(d, np.nan, 1) == [1, 4, 0, 2, 8, 5]        # no depth is beyond a NaN threshold
    # a depth equal to the threshold is not beyond it
    d = np.concatenate([np.full(100, TH, np.float32), [np.float32(TH) + np.float32(1e-5)] * 3])
    assert R.visit_order(d, TH, 1) == list(range(101))


@pytest.mark.parametrize("seed", range(20))
def test_closed_form_of_the_visit_count_equals_the_serial_loop(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 400)); d = rng.choice(np.array([0, -1, np.nan, 5, 20, 35, 36, 50, np.inf], np.float32), n)
    if seed % 2:
        d = np.where(d > 0, d + rng.uniform(0, 1, n).astype(np.float32), d).astype(np.float32)
    m = int((d > 0).sum()); near = int(((d > 0) & ~(d > np.float32(TH))).sum())
    for mode in (0, 1, 2):
        assert len(R.visit_order(d, TH, mode)) == R.n_visited_closed_form(m, near, mode)


def test_found_ratio_and_the_chain():
    assert R.found_ratio_culls(1, 5) and not R.found_ratio_culls(1, 4) and not R.found_ratio_culls(0, 0) and R.found_ratio_culls(0, 3) and not R.found_ratio_culls(3, 0)
    D = R.cull_decision
    assert D(True, 0, 3, 22, 10, 1, 3) == 1                         # bad comes first
    assert D(False, 1, 5, 22, 22, 9, 3) == 2
    assert D(False, 1, 1, 22, 20, 3, 3) == 3 and D(False, 1, 1, 22, 20, 4, 3) == 0 and D(False, 1, 1, 22, 21, 1, 3) == 0
    assert D(False, 1, 1, 22, 19, 4, 3) == 4 and D(False, 1, 1, 22, 19, 3, 3) == 3
    assert D(False, 1, 1, 22, -1, 9, 3) == 4                        # a temporal point's mnFirstKFid


def _two_keyframes():
    rng = np.random.default_rng(5)
    kfs = [G.keyframe(rng, 10, 8), G.keyframe(rng, 20, 8)]
    return rng, kfs


def test_a_point_held_by_several_features_is_added_by_the_lowest():
    rng, kfs = _two_keyframes()
    mps = [G.point(rng, 500, [(10, 3)]), G.point(rng, 501, [(10, 4), (20, 6)]), G.point(rng, 502, [(10, 5)], bad=True)]
    kfs[1]["mp_id"][:] = [501, 500, R.NO_MAP_POINT, 500, 9999, 502, 501, 500]
    sc = G._scene(kfs, mps, 4); R.build_index(sc, 0, 3)
    out, after = R.process_new_keyframe(sc, 1, 0, 2, 1.2, True)
    assert out["kind"].tolist() == [4, 3, 0, 4, 2, 1, 4, 4] and out["recent_slots"].tolist() == [1, 0, 1, 0] and out["n_added"] == 1
    assert after["mps"][0]["obs"] == [(10, 3), (20, 1)] and after["mps"][1]["obs"] == [(10, 4), (20, 6)] and sc["mps"][0]["obs"] == [(10, 3)]
    again, same = R.process_new_keyframe(sc, 1, 0, 2, 1.2, False)
    assert same is sc and again["kind"].tolist() == out["kind"].tolist()
    # a full list: the kinds are the same, nothing is written
    sc["O"] = 1
    out, after = R.process_new_keyframe(sc, 1, 0, 2, 1.2, True)
    assert out["capacity_error"] and after is sc and out["kind"].tolist() == [4, 3, 0, 4, 2, 1, 4, 4]


def test_a_slot_named_twice_in_the_recent_list_is_decided_by_its_first_occurrence():
    rng, kfs = _two_keyframes()
    mps = [G.point(rng, 500, [(10, 0)], found=1, visible=5, first_kf=20),       # culled by the ratio; its second mention finds it bad
           G.point(rng, 501, [(10, 1), (20, 1)], first_kf=20),                  # stays, twice
           G.point(rng, 502, [(10, 2)], first_kf=17, found=4, visible=4),       # weight 2 <= 3 two keyframes on: culled
           G.point(rng, 503, [(10, 3), (20, 3), (30, 3)], first_kf=15),         # old enough to leave the list, twice
           G.point(rng, 504, [(10, 4)], bad=True)]
    kfs[0]["u_right"][2] = 5.0
    for s in range(5):
        kfs[0]["mp_id"][s] = 500 + s; kfs[0]["flags"][s] = R.HAS_MP
    sc = G._scene(kfs, mps, 5); R.build_index(sc, 0, 5)
    mps[3]["obs"] = [(10, 3), (20, 3), (30, 3)]; kfs[0]["u_right"][3] = 5.0; kfs[1]["u_right"][3] = -1.0     # weights 2 + 1 + 1 (keyframe 30 is nowhere)
    lst = [0, 1, 0, 2, 3, 4, 1, 3, 2, 4]
    out, after = R.map_point_culling(sc, lst, 20, 3, 0, 2, True)
    assert out["decision"].tolist() == [2, 0, 1, 3, 4, 1, 0, 4, 1, 1] and out["kept_slots"].tolist() == [1, 1] and out["n_culled"] == 2
    assert after["mps"][0]["flags"] & R.MP_BAD and after["mps"][0]["obs"] == [] and int(after["kfs"][0]["mp_id"][0]) == R.NO_MAP_POINT and after["kfs"][0]["flags"][0] == 0
    assert int(after["kfs"][0]["mp_id"][1]) == 501 and int(after["kfs"][0]["mp_id"][2]) == R.NO_MAP_POINT and int(after["kfs"][0]["mp_id"][3]) == 503
    dry, same = R.map_point_culling(sc, lst, 20, 3, 0, 2, False)
    assert same is sc and dry["decision"].tolist() == out["decision"].tolist() and not sc["mps"][0]["flags"] & R.MP_BAD
    # keyframe 10 outside the named range: the observation there weighs 1 and its record keeps the id
    out, after = R.map_point_culling(sc, [2], 20, 3, 1, 1, True)
    assert out["decision"].tolist() == [3] and int(after["kfs"][0]["mp_id"][2]) == 502


def test_every_kind_and_decision_is_reached_at_least_eight_times():
    c = G.counts()
    assert all(c[1][k] >= 8 for k in range(4)), c[1]
    assert all(c[3][k] >= 8 for k in range(5)), c[3]
    assert all(c[4][k] >= 8 for k in range(5)), c[4]


def test_the_created_records_of_a_case():
    sc, a = G.points_case("d102_far100")
    out, after = R.create_stereo_points(sc, apply=True, **a)
    assert out["n_visited"] == 101 and out["n_created"] == int(np.isin(out["kind"], (1, 2)).sum()) > 0
    kf = after["kfs"][0]; k = 0
    for j, i in enumerate(out["order"]):
        if out["kind"][j] in (1, 2):
            p = after["mps"][a["first_mp_slot"] + k]
            assert p["id"] == 70000 + k and p["obs"] == [(17, int(i))] and int(kf["mp_id"][i]) == p["id"] and kf["flags"][i] & 1 and int(after["kfs"][1]["mp_id"][i]) == p["id"]
            assert p["n_visible"] == 1 and p["n_found"] == 1 and p["scratch"]["first_frame"] == 4242 and abs(np.linalg.norm(p["normal"]) - 1) < 1e-5
            k += 1
        else:
            assert int(kf["mp_id"][i]) == int(sc["kfs"][0]["mp_id"][i])
    short = dict(a, first_mp_slot=len(sc["mps"]) - out["n_created"] + 1)
    full, same = R.create_stereo_points(sc, apply=True, **short)
    assert full["capacity_error"] and same is sc and np.array_equal(full["order"], out["order"])

"""CPU: tests/covis_reference.py pinned by hand-worked known answers -- tiny maps whose expected rows are written out here, derived by hand from the reference text
(corbslam_client/src/KeyFrame.cc:133-168, :199-269, :404-502, :685-698; LocalMapping.cc:590-648; Optimizer.cc:493-544) -- and the seeded generators of
tests/covis_cases.py checked for the cases they exist for: a generator that never produces the hard case hides a failure."""
import collections

import pytest

import covis_reference as R
import covis_cases as G


def tiny(kf_ids, shared, bad_kfs=()):
    """keyframes kf_ids (in the cache) and, per entry (observers, n) of `shared`, n points seen by exactly those observers (ids outside kf_ids: not in the cache)"""
    m = R.Map()
    feats = {k: [] for k in kf_ids}
    pid = 1
    for observers, n in shared:
        for _ in range(n):
            obs = {}
            for k in observers:
                if k in feats:
                    obs[k] = len(feats[k]); feats[k].append(pid)
                else:
                    obs[k] = 0
            m.mps[pid] = R.MapPoint(pid, obs); pid += 1
    for k in kf_ids:
        m.kfs[k] = R.KeyFrame(k, feats[k], bad=k in bad_kfs)
    return m


def test_tie_in_weight_goes_to_the_higher_id_first():
    m = tiny([1, 2, 3, 4], [((1, 2), 16), ((1, 3), 16), ((1, 4), 20)])
    assert R.update_connections(m, 1) == 4
    assert m.kfs[1].weights == {2: 16, 3: 16, 4: 20}
    assert m.kfs[1].ordered == [(4, 20), (3, 16), (2, 16)]
    for k, w in ((2, 16), (3, 16), (4, 20)):                    # AddConnection(this, weight) on every listed keyframe
        assert m.kfs[k].weights == {1: w} and m.kfs[k].ordered == [(1, w)]


def test_no_weight_of_15_lists_the_lowest_id_among_the_maxima():
    m = tiny([1, 2, 3, 4], [((1, 2), 5), ((1, 3), 7), ((1, 4), 7)])
    assert R.update_connections(m, 1) == 3
    assert m.kfs[1].weights == {2: 5, 3: 7, 4: 7} and m.kfs[1].ordered == [(3, 7)]
    assert m.kfs[3].weights == {1: 7} and m.kfs[3].ordered == [(1, 7)]
    assert m.kfs[2].weights == {} and m.kfs[4].weights == {} and m.kfs[4].ordered == []


def test_an_id_outside_the_store_is_counted_but_never_listed_by_update():
    m = tiny([1, 2], [((1, 99), 20), ((1, 2), 16)])
    assert R.update_connections(m, 1) == 2
    assert m.kfs[1].weights == {2: 16, 99: 20} and m.kfs[1].ordered == [(2, 16)]
    assert R.get_weight(m, 1, 99) == 20 and R.get_weight(m, 1, 5) == 0
    m = tiny([1, 2], [((1, 99), 20), ((1, 2), 3)])              # the maximum over the keyframes of the cache, not over the counter
    assert R.update_connections(m, 1) == 2 and m.kfs[1].ordered == [(2, 3)]
    m = tiny([1], [((1, 99), 20)])                              # nothing of the cache is counted: the defined reading (the reference dereferences NULL)
    assert R.update_connections(m, 1) is None and m.kfs[1].weights == {99: 20} and m.kfs[1].ordered == []
    m = tiny([1], [((1,), 4)])                                  # empty counter: nothing changes
    m.kfs[1].weights = {8: 1}; m.kfs[1].ordered = [(8, 1)]
    assert R.update_connections(m, 1) is None and m.kfs[1].weights == {8: 1} and m.kfs[1].ordered == [(8, 1)]


def test_repeated_add_connection_keeps_a_thresholded_list_and_a_changed_weight_lists_everything():
    m = tiny([1, 2, 3], [((1, 2), 16), ((2, 3), 3)])
    R.update_connections(m, 2)
    assert m.kfs[2].weights == {1: 16, 3: 3} and m.kfs[2].ordered == [(1, 16)]                  # thresholded: 3 is counted, not listed
    assert m.kfs[1].ordered == [(2, 16)] and m.kfs[3].weights == {}
    R.update_connections(m, 1)                                  # AddConnection(2 <- 1, 16): the weight is what it was
    assert m.stats["early_return"] == 1
    assert m.kfs[2].weights == {1: 16, 3: 3} and m.kfs[2].ordered == [(1, 16)]
    # one more common point: the weight changes and the list of keyframe 2 is rebuilt from its whole map
    m.mps[1000] = R.MapPoint(1000, {1: len(m.kfs[1].mp_ids), 2: len(m.kfs[2].mp_ids)})
    m.kfs[1].mp_ids.append(1000); m.kfs[2].mp_ids.append(1000)
    R.update_connections(m, 1)
    assert m.kfs[1].ordered == [(2, 17)]
    assert m.kfs[2].weights == {1: 17, 3: 3} and m.kfs[2].ordered == [(1, 17), (3, 3)]          # everything
    assert R.get_vector_covisibles(m, 2) == [1, 3] and R.get_best_covisibles(m, 2, 1) == [1] and R.get_best_covisibles(m, 2, 5) == [1, 3]


def order_map():
    """keyframe 1 holds one of its 16 points in common with keyframe 2 at two features: 1 counts 2 seventeen times, 2 counts 1 sixteen times"""
    m = tiny([1, 2, 3], [((1, 2), 16), ((1, 3), 3)])
    m.kfs[1].mp_ids.append(m.kfs[1].mp_ids[0])
    return m


def test_update_a_then_b_differs_from_b_then_a():
    m = order_map()
    R.update_connections(m, 1); R.update_connections(m, 2)
    assert m.kfs[1].weights == {2: 16, 3: 3} and m.kfs[1].ordered == [(2, 16), (3, 3)]
    assert m.kfs[2].weights == {1: 16} and m.kfs[2].ordered == [(1, 16)]
    m = order_map()
    R.update_connections(m, 2); R.update_connections(m, 1)
    assert m.kfs[1].weights == {2: 17, 3: 3} and m.kfs[1].ordered == [(2, 17)]
    assert m.kfs[2].weights == {1: 17} and m.kfs[2].ordered == [(1, 17)]


def test_erase_connection_rebuilds_only_rows_that_held_the_entry():
    m = tiny([1, 2, 3], [((1, 2), 16), ((1, 3), 3), ((2, 3), 15)])
    R.update_connections(m, 1)                                  # 1: {2:16, 3:3} / [(2,16)];  2: {1:16} / [(1,16)];  3 never hears of 1
    R.update_connections(m, 2)                                  # 2: {1:16, 3:15} / [(1,16),(3,15)];  3: {2:15} / [(2,15)];  1: early return
    assert m.kfs[3].weights == {2: 15}
    R.erase_connections(m, 1)
    assert m.kfs[1].weights == {} and m.kfs[1].ordered == []
    assert m.kfs[2].weights == {3: 15} and m.kfs[2].ordered == [(3, 15)]
    assert m.kfs[3].weights == {2: 15} and m.kfs[3].ordered == [(2, 15)]


def test_covisibles_by_weight_follows_upper_bound_and_its_end_test():
    m = tiny([1, 2], [])
    m.kfs[1].weights = {2: 30, 50: 20, 9: 10}; R.update_best_covisibles(m.kfs[1]); m.kfs[9] = R.KeyFrame(9, [])
    assert m.kfs[1].ordered == [(2, 30), (50, 20), (9, 10)]
    assert R.get_covisibles_by_weight(m, 1, 20) == [2, None]    # unfiltered: the id outside the cache is a null
    assert R.get_covisibles_by_weight(m, 1, 21) == [2] and R.get_covisibles_by_weight(m, 1, 31) == []
    assert R.get_covisibles_by_weight(m, 1, 10) == []           # every weight reaches w: `it == end()` returns the empty vector
    assert R.get_vector_covisibles(m, 1) == [2, 9]


def culling_point(octaves, n_points=1, n_redundant=None):
    """keyframe 5 (octave 2 everywhere) with n_points points, each seen by 5 and by keyframes 6, 7, 8 at the given octaves (the first n_redundant points; the others
    by 5 alone); keyframe 1 lists 5"""
    n_redundant = n_points if n_redundant is None else n_redundant
    m = tiny([1, 5, 6, 7, 8], [((5, 6, 7, 8), n_redundant), ((5,), n_points - n_redundant)])
    m.kfs[5].octave = [2] * n_points
    for k, o in zip((6, 7, 8), octaves):
        m.kfs[k].octave = [o] * n_redundant
    m.kfs[1].weights = {5: 20}; m.kfs[1].ordered = [(5, 20)]
    return m


def test_culling_counts_an_observer_up_to_one_octave_above():
    assert R.keyframe_culling(culling_point((2, 3, 4)), 1, True, 0.0) == [(5, 1, 0, False)]     # exactly three others, one of them at octave + 2
    assert R.keyframe_culling(culling_point((2, 3, 3)), 1, True, 0.0) == [(5, 1, 1, True)]
    m = culling_point((2, 3, 3)); del m.mps[1].obs[8]                                           # Observations() == 3 is not `> thObs`
    assert R.keyframe_culling(m, 1, True, 0.0) == [(5, 1, 0, False)]


def test_culling_boundary_at_ten_points():
    assert R.keyframe_culling(culling_point((0, 0, 0), 10, 9), 1, True, 0.0) == [(5, 10, 9, False)]      # 9 > 9.0 is false
    assert R.keyframe_culling(culling_point((0, 0, 0), 10, 10), 1, True, 0.0) == [(5, 10, 10, True)]
    m = culling_point((0, 0, 0), 10, 10); m.kfs[5].depth = [1.0] * 8 + [50.0, -1.0]                    # stereo: two features leave before nMPs++
    assert R.keyframe_culling(m, 1, False, 35.0) == [(5, 8, 8, True)]
    m.kfs[5].id = 0; m.kfs[0] = m.kfs.pop(5); m.kfs[1].ordered = [(0, 20)]                               # mnId == 0 is skipped
    assert R.keyframe_culling(m, 1, False, 35.0) == [(0, 0, 0, False)]


def test_window_a_bad_covisible_keyframe_is_neither_local_nor_fixed():
    m = tiny([1, 2, 3, 4, 5, 6], [((1, 2, 3, 4, 77), 1), ((2, 3, 5, 6), 1), ((1, 2), 1)], bad_kfs=(3, 6))
    m.kfs[1].weights = {2: 20, 3: 18}; m.kfs[1].ordered = [(2, 20), (3, 18)]
    local, fixed, points = R.local_window(m, 1)
    assert local == [1, 2]                                      # 3 carries mnBALocalForKF but is bad
    assert points == [1, 3, 2]                                  # first appearance: keyframe 1's features, then keyframe 2's
    assert fixed == [4, 5]                                      # 3 is marked local, 77 is not in the cache, 6 is bad: marked, not listed


CASES = sorted(G.RANDOM_MAPS)


@pytest.mark.parametrize("name", CASES)
def test_seeded_maps_reach_every_case_of_update(name):
    total = collections.Counter()
    for order in (1, -1):
        m = G.random_map(**G.RANDOM_MAPS[name])
        for kid in sorted(m.kfs)[::order]:
            R.update_connections(m, kid)
        total += m.stats
    for what in ("tie", "fallback", "unknown", "bad_point", "early_return", "resort"):
        assert total[what] >= 1, (name, what, dict(total))
    print(name, dict(total))


@pytest.mark.parametrize("name", sorted(G.CULLING_MAPS))
def test_seeded_culling_maps_answer_both_ways(name):
    m = G.culling_map(**G.CULLING_MAPS[name])
    R.update_connections(m, 7)
    out = R.keyframe_culling(m, 7, False, 35.0) + R.keyframe_culling(m, 7, True, 35.0)
    n_cull = sum(1 for o in out if o[3]); n_keep = sum(1 for o in out if not o[3] and o[1] > 0)
    obs = collections.Counter(R.observations(m, p) for p in m.mps.values())
    if G.CULLING_MAPS[name].get("n_helpers", 3) == 3:
        assert n_cull >= 1 and n_keep >= 1 and obs[3] >= 1 and obs[4] >= 1, (name, n_cull, n_keep, dict(obs))
    else:
        assert n_keep >= 1
    print(name, n_cull, n_keep, dict(obs))

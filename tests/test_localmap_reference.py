"""tests/localmap_reference.py is the definition the device routes of the local map and the spanning tree are held against; here its readings are pinned by cases small
enough to work out by hand, and the seeded generators of tests/localmap_cases.py are checked to reach every event those readings are about.  CPU only."""
import collections

import covis_reference as R
import localmap_cases as C
import localmap_reference as LR

NO_ID = LR.NO_ID


def tiny(kfs, points, bad_kfs=(), bad_points=()):
    """kfs: {id: [point ids]}; points: {id: [observer ids]} (feature index = position of the point in that keyframe, 0 for a keyframe that is not held)"""
    m = R.Map()
    for k, ids in kfs.items():
        m.kfs[k] = R.KeyFrame(k, ids, bad=k in bad_kfs)
    for p, obs in points.items():
        m.mps[p] = R.MapPoint(p, {o: (kfs[o].index(p) if o in kfs and p in kfs[o] else 0) for o in obs}, bad=p in bad_points)
    return m


def connect(m, a, b, w):
    """a symmetric connection as two AddConnection calls leave it"""
    R.add_connection(m, m.kfs[a], b, w)
    if b in m.kfs:
        R.add_connection(m, m.kfs[b], a, w)


def test_a_vote_tie_goes_to_the_smaller_id():
    m = tiny({9: [101, 102], 5: [101, 102]}, {101: [5, 9], 102: [9, 5]})
    r = LR.update_local_map(m, LR.Frame([101, 102]), [])
    assert r["kfs"] == [5, 9] and r["ref"] == 5 and r["n_voted"] == 2 and r["mps"] == [101, 102] and not r["counter_empty"]


def test_a_bad_keyframe_with_the_most_votes_is_not_the_reference_and_not_listed():
    m = tiny({5: [101, 102, 103], 9: [103, 104]}, {101: [5], 102: [5], 103: [5, 9], 104: [9]}, bad_kfs={5})
    r = LR.update_local_map(m, LR.Frame([101, 102, 103]), [])
    assert r["kfs"] == [9] and r["ref"] == 9 and r["n_voted"] == 1
    assert r["mps"] == [103, 104]


def test_voters_that_are_all_bad_give_an_empty_list_and_no_points():
    m = tiny({5: [101]}, {101: [5]}, bad_kfs={5})
    r = LR.update_local_map(m, LR.Frame([101]), [5])
    assert r["kfs"] == [] and r["mps"] == [] and r["ref"] is None and not r["counter_empty"]


def test_a_bad_point_is_cleared_and_an_unresolved_id_is_kept():
    m = tiny({5: [101, 102]}, {101: [5], 102: [5]}, bad_points={101})
    f = LR.Frame([101, 424242, 102, NO_ID])
    r = LR.update_local_map(m, f, [])
    assert f.mp_ids == [NO_ID, 424242, 102, NO_ID] and r["n_cleared"] == 1 and r["kfs"] == [5] and r["mps"] == [102]


def test_an_empty_counter_keeps_the_previous_list_and_the_points_still_run():
    m = tiny({5: [101, 102], 9: [102, 103]}, {101: [5], 102: [5, 9], 103: [9]}, bad_points={101})
    f = LR.Frame([101, 424242, NO_ID])
    r = LR.update_local_map(m, f, [9, 5])
    assert r["counter_empty"] and r["kfs"] == [9, 5] and r["ref"] is None and r["n_voted"] == 0
    assert f.mp_ids == [NO_ID, 424242, NO_ID] and r["n_cleared"] == 1              # the loop of :1263 ran before the return
    assert r["mps"] == [102, 103]                                                    # UpdateLocalPoints on the old list; 101 is bad
    # an observer the store does not hold is no voter: the counter stays empty
    m.mps[104] = R.MapPoint(104, {9000001: 0})
    assert LR.update_local_map(m, LR.Frame([104]), [5])["counter_empty"]


def test_a_neighbour_the_store_does_not_hold_is_skipped():
    m = tiny({5: [101], 7: [102], 8: [103]}, {101: [5], 102: [7], 103: [8]})
    connect(m, 5, 9000001, 30); connect(m, 5, 7, 20); connect(m, 5, 8, 10)
    assert m.kfs[5].ordered == [(9000001, 30), (7, 20), (8, 10)]
    r = LR.update_local_map(m, LR.Frame([101]), [])
    assert r["kfs"] == [5, 7] and r["ref"] == 5 and r["mps"] == [101, 102]          # one neighbour per keyframe: 8 stays out


def test_the_neighbours_are_the_first_ten_held_ones():
    kfs = {5: [101]}; kfs.update({20 + i: [] for i in range(11)})
    m = tiny(kfs, {101: [5]})
    for i in range(11):
        connect(m, 5, 20 + i, 50 - i)
    LR.tree(m.kfs[5])
    for i in range(10):
        m.kfs[20 + i].bad = True                                                      # the ten best are bad; the eleventh is good but not among GetBestCovisibilityKeyFrames(10)
    assert LR.update_local_map(m, LR.Frame([101]), [])["kfs"] == [5]


def test_the_child_is_picked_in_ascending_id():
    m = tiny({5: [101], 8: [], 12: [], 30: []}, {101: [5]}, bad_kfs={8})
    LR.set_tree(m, 5, None, False, [30, 12, 8, 9000002])
    r = LR.update_local_map(m, LR.Frame([101]), [])
    assert r["kfs"] == [5, 12]                                                        # 8 is bad, 9000002 is not held, 30 comes later


def test_the_break_after_a_parent_ends_the_whole_walk():
    m = tiny({3: [], 5: [101], 9: [101], 11: []}, {101: [5, 9]})
    connect(m, 9, 11, 20)
    LR.set_tree(m, 5, 3, False, [])
    r = LR.update_local_map(m, LR.Frame([101]), [])
    assert r["kfs"] == [5, 9, 3]                                                      # 11, the neighbour of the later voter 9, is NOT added
    # without the parent the walk reaches 9
    LR.set_tree(m, 5, None, False, [])
    assert LR.update_local_map(m, LR.Frame([101]), [])["kfs"] == [5, 9, 11]
    # a parent that is already in the list does not break
    LR.set_tree(m, 5, 9, False, [])
    assert LR.update_local_map(m, LR.Frame([101]), [])["kfs"] == [5, 9, 11]
    # a bad parent is pushed all the same (:1349-1357 does not ask isBad)
    LR.set_tree(m, 5, 3, False, []); m.kfs[3].bad = True
    assert LR.update_local_map(m, LR.Frame([101]), [])["kfs"] == [5, 9, 3]


def test_the_walk_stops_when_the_list_holds_more_than_80():
    voters = list(range(1, 80))                                                       # 79 voters, each with one held neighbour of its own
    kfs = {k: [100000] for k in voters}; kfs.update({1000 + k: [] for k in voters})
    m = tiny(kfs, {100000: voters})
    for k in voters:
        connect(m, k, 1000 + k, 20)
    r = LR.update_local_map(m, LR.Frame([100000]), [])
    assert r["n_voted"] == 79 and r["kfs"] == voters + [1001, 1002]                   # 80 is not more than 80: the second push happens, the third iteration stops
    # 81 voters: the walk stops before its first iteration
    voters = list(range(1, 82))
    kfs = {k: [100000] for k in voters}; kfs.update({1000 + k: [] for k in voters})
    m = tiny(kfs, {100000: voters})
    for k in voters:
        connect(m, k, 1000 + k, 20)
    r = LR.update_local_map(m, LR.Frame([100000]), [])
    assert r["kfs"] == voters and m.stats["stop_80"] == 1


def test_local_points_take_the_first_occurrence_and_do_not_ask_the_keyframe():
    m = tiny({5: [101, 102, 101], 9: [103, 102, 424242, NO_ID, 104]}, {101: [5], 102: [5, 9], 103: [9], 104: [9]}, bad_kfs={9}, bad_points={104})
    assert LR.update_local_points(m, [9, 5]) == [103, 102, 101]                       # 9 is bad and still gives its points


def test_the_first_connection_rule_with_a_held_and_an_unheld_front():
    m = tiny({5: [], 7: [], 0: []}, {})
    LR.first_connection(m, 7, 5)
    assert LR.get_tree(m, 7) == (5, False, []) and LR.get_tree(m, 5) == (None, True, [7])
    LR.first_connection(m, 7, 0)                                                      # not the first connection any more
    assert LR.get_tree(m, 7) == (5, False, []) and LR.get_tree(m, 0) == (None, True, [])
    LR.first_connection(m, 5, 9000001)                                                # the cache does not hold the front: mpParent is set, the flag stays
    assert LR.get_tree(m, 5) == (9000001, True, [7])
    LR.first_connection(m, 5, 7)                                                      # so the next update sets it again
    assert LR.get_tree(m, 5) == (7, False, [7]) and LR.get_tree(m, 7) == (5, False, [5])
    LR.first_connection(m, 0, 5)                                                      # mnId 0 never gets a parent
    assert LR.get_tree(m, 0) == (None, True, [])
    LR.first_connection(m, 0, None)
    assert m.stats["first_held"] == 2 and m.stats["first_unheld"] == 1


def test_update_connections_grows_the_tree():
    m = tiny({1: list(range(100, 116)), 2: list(range(100, 116))}, {p: [1, 2] for p in range(100, 116)})
    assert LR.update_connections(m, 2) == 1
    assert LR.get_tree(m, 2) == (1, False, []) and LR.get_tree(m, 1) == (None, True, [2])
    assert LR.update_connections(m, 1) == 2
    assert LR.get_tree(m, 1) == (2, False, [2]) and LR.get_tree(m, 2) == (1, False, [1])


def test_change_parent_leaves_the_old_parents_set():
    m = tiny({1: [], 2: [], 3: []}, {})
    LR.change_parent(m, 3, 1); LR.change_parent(m, 3, 2)
    assert LR.get_tree(m, 3)[0] == 2 and LR.get_tree(m, 1)[2] == [3] and LR.get_tree(m, 2)[2] == [3]
    LR.erase_child(m, 1, 3); LR.erase_child(m, 1, 3)
    assert LR.get_tree(m, 1)[2] == []


def culled(children_links):
    """keyframe 10 with parent 2 and the children 20, 30, 40; children_links: [(a, b, w)] connections"""
    m = tiny({2: [], 10: [], 20: [], 30: [], 40: []}, {})
    LR.set_tree(m, 2, None, False, [10]); LR.set_tree(m, 10, 2, False, [20, 30, 40])
    for k in (20, 30, 40):
        LR.set_tree(m, k, 10, False, [])
    for a, b, w in children_links:
        connect(m, a, b, w)
    return m


def test_reparenting_over_two_rounds_and_the_quirk_when_no_child_is_left():
    m = culled([(20, 2, 40), (30, 20, 25), (40, 30, 90)])
    assert LR.reparent_children(m, 10) == (3, False)                                  # 20 -> 2, then 30 -> 20, then 40 -> 30: 90 counts only once 30 is a candidate
    assert [LR.get_tree(m, k)[0] for k in (20, 30, 40)] == [2, 20, 30]
    assert LR.get_tree(m, 2)[2] == [10, 20]                                           # every child found a parent: 10 is NOT erased from its parent's set, and not marked bad
    assert LR.get_tree(m, 10) == (2, False, [])
    assert m.stats["reparent_two_rounds"] == 1 and m.stats["quirk_not_bad"] == 1


def test_the_first_best_pair_stays_on_equal_weights():
    m = culled([(30, 2, 40), (20, 2, 40), (40, 2, 40)])
    m.kfs[20].bad = True                                                              # a bad child is skipped by the loop ...
    n, bad = LR.reparent_children(m, 10)
    assert [LR.get_tree(m, k)[0] for k in (20, 30, 40)] == [2, 2, 2] and (n, bad) == (3, True)      # ... and handed to the parent by the fallback
    assert LR.get_tree(m, 10)[2] == [20]                                              # the reference does not clear what the fallback hands over
    m = culled([(30, 2, 40), (20, 2, 40)])
    LR.reparent_children(m, 10)
    assert m.kfs[2].children == {20, 30, 40}                                          # (10 erased by the fallback for 40)


def test_the_fallback_to_the_original_parent_and_the_quirk_the_other_way():
    m = culled([(20, 2, 40)])
    assert LR.reparent_children(m, 10) == (3, True)                                   # 20 by the loop; 30 and 40 have no link to a candidate
    assert [LR.get_tree(m, k)[0] for k in (20, 30, 40)] == [2, 2, 2]
    assert LR.get_tree(m, 2)[2] == [20, 30, 40]                                       # 10 left its parent's set
    assert LR.get_tree(m, 10)[2] == [30, 40]
    # no held parent: the leftovers keep the culled keyframe as their parent and the reference does not mark it bad
    m = culled([])
    LR.set_tree(m, 10, 9000001, False, [20, 30])
    assert LR.reparent_children(m, 10) == (0, False) and LR.get_tree(m, 20)[0] == 10 and LR.get_tree(m, 10)[2] == [20, 30]
    # no children at all: nothing happens, the parent keeps the keyframe
    m = culled([])
    LR.set_tree(m, 10, 2, False, [])
    assert LR.reparent_children(m, 10) == (0, False) and LR.get_tree(m, 2)[2] == [10]
    assert m.stats["quirk_not_bad"] == 1


def test_a_keyframe_that_is_its_own_parent_erases_itself_from_its_own_set():
    """two keyframes that took each other as parents, one of them culled, leave the other as its own parent and child; its fallback then edits the set it walks"""
    m = culled([])
    LR.set_tree(m, 10, 10, False, [10, 20])
    assert LR.reparent_children(m, 10) == (2, True) and LR.get_tree(m, 10) == (10, False, [20]) and LR.get_tree(m, 20)[0] == 10


EVENTS = ["vote_tie", "bad_top_voter", "cleared", "unresolved_kept", "counter_empty", "neighbour_unheld", "child_pick", "child_pick_not_first", "parent_break",
          "parent_break_before_the_end", "stop_80", "first_held", "reparent_two_rounds", "fallback_parent", "quirk_sets_bad", "quirk_not_bad"]


def test_the_generators_reach_every_event():
    """(first_unheld is not in the list: UpdateConnections takes the front from the keyframes the store holds, so only the hand-worked case above can reach it)"""
    total = collections.Counter()
    most_voters = 0
    for name, (kw, frames) in C.LOCALMAP_CASES.items():
        m = C.grown_map(**kw)
        assert 8 <= len(m.kfs) <= 128
        for seed, n, first, width, extra in frames:
            f = C.frame_for(m, seed, n, first, width, **extra)
            most_voters = max(most_voters, len(LR.voters(m, f)))
            r = LR.update_local_map(m, f, sorted(m.kfs)[:3])
            assert len(set(r["kfs"])) == len(r["kfs"]) and len(set(r["mps"])) == len(r["mps"])
        for k in C.culling_sequence(m, 5, 6):
            C.set_bad_flag(m, k)
        total += m.stats
    for e in EVENTS:
        assert total[e] >= 1, e
    assert most_voters > 80

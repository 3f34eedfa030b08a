"""CPU tests of tests/loopdetect_reference.py, the definition behind include/corb_loop_detect.h, on the hand-built worlds of tests/loopdetect_cases.py: the answers are
written out here, derived by hand from the worlds' graphs (OLD7: 1 - 2 - 4 - 5, 2 - 3, 7 alone, 6 the filler) and from LoopClosing.cc:100-231.  Then the counts that
make the seeded walks worth running on the device: every outcome at least three times per walk, a candidate consistent with two previous groups, a previous group
met by two candidates -- on the definition alone.  The GPU tests (tests/test_gpu_loopdetect.py) compare the device with these same runs."""
import numpy as np
import pytest

import loopdetect_cases as G
import loopdetect_reference as R

GAP, NONE, NOT_ENOUGH, DETECTED = R.GAP, R.NONE, R.NOT_ENOUGH, R.DETECTED


def answers(name):
    return [a for _, a in G.run(G.hand(name)) if a is not None]


def brief(a):
    return a["outcome"], a["candidates"], a["enough"], a["groups"]


def test_the_counter_runs_0_1_2_3_and_the_fourth_keyframe_detects():
    a = answers("sequence")
    g = [1, 2, 3, 4]                                                # candidate 2 and its connections 1, 3, 4
    assert [brief(x) for x in a] == [(NOT_ENOUGH, [2], [], [(g, 0)]), (NOT_ENOUGH, [2], [], [(g, 1)]), (NOT_ENOUGH, [2], [], [(g, 2)]), (DETECTED, [2], [0], [(g, 3)])]
    # minScore is the filler's score: the one shared word, 0.3 / 6.3 against 0.2 -> min(a, b) = 0.3 / 6.3, rounded to float once
    assert all(x["minScore"].dtype == np.float32 and x["minScore"] == np.float32(0.3 / 6.3) for x in a)


def test_two_candidates_meet_one_previous_group_only_the_first_gives_a_group_and_both_are_enough():
    a = answers("two_candidates_one_group")
    assert brief(a[2]) == (NOT_ENOUGH, [2], [], [([1, 2, 3, 4], 2)])
    assert brief(a[3]) == (DETECTED, [1, 3], [0, 1], [([1, 2], 3)])        # candidate 1 = {1, 2} takes the group; candidate 3 = {2, 3} adds none, and no counter-0 group


def test_one_candidate_meets_two_previous_groups_and_gives_two_groups_with_different_counters():
    a = answers("one_candidate_two_groups")
    assert brief(a[0]) == (NOT_ENOUGH, [1], [], [([1, 2], 0)])
    assert brief(a[1]) == (NOT_ENOUGH, [1, 5], [], [([1, 2], 1), ([4, 5], 0)])
    assert brief(a[2]) == (NOT_ENOUGH, [4], [], [([2, 4, 5], 2), ([2, 4, 5], 1)])


def test_a_candidate_without_connections_has_the_group_of_itself():
    assert [brief(x) for x in answers("no_connections")] == [(NOT_ENOUGH, [7], [], [([7], 0)])]


def test_gap_leaves_the_groups_and_none_clears_them():
    w = G.hand("gap_and_none"); lc = w.reference()[0]
    out = G.run(w, lc)
    g = [1, 2, 3, 4]
    assert [brief(a) for _, a in out if a is not None] == [(NOT_ENOUGH, [2], [], [(g, 0)]), (GAP, [], [], [(g, 0)]), (NOT_ENOUGH, [2], [], [(g, 1)]), (NONE, [], [], [])]
    assert out[2][1]["minScore"] is None                                # :111 returns before minScore exists
    assert lc.live >= {100, 101, 102, 103} and lc.mLastLoopKFid == 0    # every outcome adds the keyframe; Reset put mLastLoopKFid back


def test_every_connected_keyframe_bad_leaves_minscore_at_one():
    a = answers("all_connected_bad")
    assert brief(a[0]) == (NONE, [], [], []) and a[0]["minScore"].view(np.uint32) == 0x3F800000


def test_an_unbound_covisible_keyframe_is_refused_before_anything_changes():
    w = G.hand("unbound_covisible"); lc, _, bow = w.reference()
    before = [o.state() for o in bow.values()]
    assert G.run(w, lc) == [(("detect", 101), "unbound")]
    assert [o.state() for o in bow.values()] == before and 101 not in lc.live and lc.mvConsistentGroups == []


def test_drop_takes_the_keyframe_out_of_every_stored_group():
    a = answers("drop")
    assert [x["groups"] for x in a] == [[([7], 0)], [([7], 1)], [([7], 0)], [([7], 1)]]      # after the drop the stored group is empty: candidate 7 starts again


def test_the_hub_gives_a_group_of_71_and_is_met_through_one_member():
    a = answers("hub")
    assert a[0]["groups"] == [(list(range(1, 72)), 0)] and a[1]["groups"] == [([3, 71], 1)]


def test_capacity_refusals_leave_the_state():
    w = G.hand("two_candidates_one_group"); lc = w.reference(max_candidates=1)[0]
    out = G.run(w, lc)
    assert out[3][1] == "capacity" and lc.groups() == [([1, 2, 3, 4], 2)] and 103 not in lc.live
    w = G.hand("one_candidate_two_groups"); lc = w.reference(max_groups=1)[0]
    lc.DetectLoop(100)
    with pytest.raises(R.Capacity):
        lc.DetectLoop(101)
    assert lc.groups() == [([1, 2], 0)] and 101 not in lc.live


def test_the_queue_stops_at_the_first_detection():
    w = G.hand("sequence"); lc = w.reference()[0]
    lc.InsertKeyFrame(0)
    for k in (100, 101, 102, 103):
        lc.InsertKeyFrame(k)
    assert lc.mlpLoopKeyFrameQueue == [100, 101, 102, 103] and lc.CheckNewKeyFrames()          # :90 id 0 is dropped
    assert [a["outcome"] for a in lc.DetectLoopQueue([100, 101, 102])] == [NOT_ENOUGH] * 3
    w2 = G.World(currents=[(100, [2]), (101, [2]), (102, [2]), (103, [2]), (104, [2])], script=[], **G.OLD7); lc2 = w2.reference()[0]
    assert [a["outcome"] for a in lc2.DetectLoopQueue([100, 101, 102, 103, 104])] == [NOT_ENOUGH] * 3 + [DETECTED] and 104 not in lc2.live


@pytest.mark.parametrize("seed", G.WALK_SEEDS)
def test_a_seeded_walk_takes_every_outcome_and_meets_both_special_cases(seed):
    w = G.walk(seed)
    assert len(w.cur_ids) == 40 and len(w.ids) <= G.N_SLOTS and max(w.slot.values()) >= 64
    c = G.stats(w)                                                      # (also checks the closed form against the serial loop at every keyframe)
    assert sum(c[o] for o in (GAP, NONE, NOT_ENOUGH, DETECTED)) == 40
    assert min(c[GAP], c[NONE], c[NOT_ENOUGH], c[DETECTED]) >= 3, dict(c)
    assert c["cand_two_groups"] >= 1 and c["group_two_cands"] >= 1, dict(c)
    m = w.map()
    assert max(len(k.weights) for k in m.kfs.values()) == 70 <= G.MAX_CONNECTIONS      # the hub's row is wider than a wavefront
    assert any(G.UNKNOWN in k.weights for k in m.kfs.values())                          # a row names a keyframe the store does not hold

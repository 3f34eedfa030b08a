"""tests/voctrain_reference.py, the definition of vocabulary training, against its own invariants on seeded cases and against a tree worked out by hand."""
import math
import numpy as np
import pytest

import dbow_reference as R
import voctrain_reference as V
import voctrain_cases as G


@pytest.mark.parametrize("name", ["k3L3n200", "k10L3n3000", "lowent", "repeat", "cap2small"])
def test_invariants_of_a_trained_tree(name):
    sets, k, L, seed, max_it = G.inputs(name)
    flat, st, members, settled = V.create(sets, k, L, seed, max_it, detail=True)
    assert G.same_flat(flat, G.expected(name)[0])
    desc = np.concatenate(sets); parent = flat["parent"]; n = len(parent)
    for i in range(n):
        if settled[i] and len(members[i]):                      # a node that ended by itself: the majority mean, or the single member, of its final group
            assert np.array_equal(flat["descriptor"][i], V.mean_value(desc[members[i]])), i
    # ids follow the source's creation order: siblings are consecutive, and the subtree of an earlier sibling comes before that of a later one
    kids = [[] for _ in range(n + 1)]
    for i in range(n):
        kids[parent[i]].append(i + 1)
    order = []

    def walk(p):
        order.extend(kids[p])
        for c in kids[p]:
            walk(c)
    walk(0)
    assert order == list(range(1, n + 1))
    assert [int(x) for x in flat["is_leaf"]] == [0 if kids[i] else 1 for i in range(1, n + 1)]
    v = R.Vocabulary(**flat)                                    # the flat result builds a vocabulary; word ids are the leaves in id order
    assert v.words.tolist() == [i for i in range(1, n + 1) if not kids[i]]
    depth = np.zeros(n + 1, int)
    for i in range(1, n + 1):
        depth[i] = depth[parent[i - 1]] + 1
    assert depth.max() <= L and all(len(c) <= k for c in kids)
    # the statistics add up
    assert st["nodes"] == n + 1 and st["words"] == v.n_words == int(flat["is_leaf"].sum())
    assert st["kmeans_nodes"] + st["trivial_nodes"] == sum(st["level_nodes"]) == sum(1 for c in kids if c)
    assert st["level_nodes"][:L] == [int(sum(1 for i in range(n + 1) if kids[i] and depth[i] == lv)) for lv in range(L)] and not any(st["level_nodes"][L:])
    assert st["max_iterations_seen"] == max(st["level_max_iterations"]) <= max_it and st["capped_nodes"] <= st["kmeans_nodes"] and st["short_nodes"] <= st["kmeans_nodes"]
    assert (st["capped_nodes"] > 0) == (name == "cap2small")
    # weights: ln(NDocs / Ni) on the words, 0 on inner nodes
    for i in range(n):
        assert flat["weight"][i] == 0.0 or (flat["is_leaf"][i] and 0.0 < flat["weight"][i] <= math.log(len(sets)))
    # text round trip, in the definition's own format and in the reference's spacing
    assert G.same_flat(R.Vocabulary.from_text(v.to_text()).flat(), flat)
    assert G.same_flat(R.Vocabulary.from_text(V.save_text(flat, 17)).flat(), flat)


def test_special_inputs_reach_the_rare_branches():
    low, rep = G.expected("lowent")[1], G.expected("repeat")[1]
    assert low["trivial_nodes"] >= 1 and low["tie_bits"] >= 1 and rep["short_nodes"] >= 1
    assert G.expected("k10L3n3000")[1]["empty_cluster_events"] >= 1


def test_one_image_gives_zero_weights_and_draws_are_in_rand_range():
    flat, _ = V.create([G.inputs("k3L3n200")[0][0]], 3, 2, 5)
    assert not flat["weight"].any()
    r = [V.draw(s, key, j) for s in (0, 1, 2 ** 64 - 1) for key in (0, 1, 21 ** 9 * 20) for j in range(4)]
    assert all(0 <= x <= 2 ** 31 - 1 for x in r) and len(set(r)) == len(r)
    assert V.child_key(V.child_key(0, 0, 19), 1, 0) == 20 + 21 and V.child_key(0, 0, 19) + 20 * sum(21 ** d for d in range(1, 10)) < 2 ** 64


def test_hand_worked_tree_k2_L2_five_descriptors():
    """A = 0, A1 = A with the first bit, B = all ones, B1 = B without the last bit, B2 = B without the last two; images {A, B, A1} and {B1, B2}; seed 1.
    root (key 0): draw 0 = 1216681718 -> int(0.5666 * 5) = 2, the first centre is A1.  min_dists = 1 255 0 254 253, sum 763; draw 1 = 1601554128 -> cut_d = 569.03;
      running sums 1 256 256 510 763: index 4, the second centre is B2.  Pass 1: groups {A, A1}, {B, B1, B2}.  Pass 2: the mean of {A, A1} needs 1 of 2: A1 (a tie bit);
      the mean of {B, B1, B2} needs 2 of 3: B1.  Nothing moves: nodes 1 = A1, 2 = B1.
    node 1: 2 features <= k: trivial, nodes 3 = A, 4 = A1.
    node 2 (key 2): draw 0 = 58835731 -> 0: B.  min_dists 0 1 2, sum 3; draw 1 = 904325824 -> cut_d = 1.26: index 2, B2.  Pass 1: B1 is 1 from both, the first wins:
      {B, B1}, {B2}.  Pass 2: the mean of {B, B1} needs 1 of 2: B; {B2} is copied.  Nodes 5 = B, 6 = B2.
    words 0 .. 3 = nodes 3 .. 6.  Descents: A -> 0, B -> 2, A1 -> 1; B1 -> 2 (1 from both leaves, the first wins), B2 -> 3: Ni = 1 1 2 1 of 2 images."""
    A = np.zeros(32, np.uint8); A1 = A.copy(); A1[0] = 0x80
    B = np.full(32, 255, np.uint8); B1 = B.copy(); B1[31] = 0xFE; B2 = B.copy(); B2[31] = 0xFC
    assert [V.draw(1, 0, 0), V.draw(1, 0, 1), V.draw(1, 2, 0), V.draw(1, 2, 1)] == [1216681718, 1601554128, 58835731, 904325824]
    flat, st = V.create([np.array([A, B, A1]), np.array([B1, B2])], 2, 2, 1)
    assert flat["parent"].tolist() == [0, 0, 1, 1, 2, 2] and flat["is_leaf"].tolist() == [0, 0, 1, 1, 1, 1]
    assert np.array_equal(flat["descriptor"], np.array([A1, B1, A, A1, B, B2]))
    ln2 = math.log(2.0)
    assert flat["weight"].tolist() == [0.0, 0.0, ln2, ln2, 0.0, ln2]
    assert [st[f] for f in V.STAT_FIELDS] == [7, 4, 2, 1, 0, 2, 0, 0] and st["level_nodes"][:3] == [1, 2, 0] and st["level_max_iterations"][:2] == [2, 2] and st["tie_bits"] == 2

"""CPU checks on the definition of place recognition (tests/dbow_reference.py), independent of the product: the word against a recursive argmin, the BowVector's
norm, the score against the dense L1 formula, the text loader's round trip, and one small case per quirk of KeyFrameDatabase.cc that would come out differently under
the "obvious" reading."""
import numpy as np
import pytest
import dbow_reference as R
import bow_cases as G


def recursive_word(v, d, node=0):
    """independent of Vocabulary.descend: numpy's argmin returns the first minimum"""
    kids = v.children[node]
    if not kids:
        return int(v.word_id[node])
    dist = [int(np.unpackbits(np.bitwise_xor(d, v.descriptor[c])).sum()) for c in kids]
    return recursive_word(v, d, kids[int(np.argmin(dist))])


@pytest.mark.parametrize("name", sorted(G.VOCABS))
def test_word_is_the_recursive_argmin_and_vectors_are_sorted_and_normalised(name):
    v = G.vocab(name)
    desc = G.features(name, 65, 5)
    for levelsup in (0, 2, 4, v.L, v.L + 1):
        word, value, node, off, idx, fw, fn = G.expected(name, 65, 5, levelsup)
        assert [recursive_word(v, d) for d in desc] == fw.tolist()
        assert np.all(np.diff(word.astype(np.int64)) > 0) and np.all(np.diff(node.astype(np.int64)) > 0)
        for j in range(len(node)):
            assert np.all(np.diff(idx[off[j]:off[j + 1]].astype(np.int64)) > 0) and off[j + 1] > off[j]
        if len(word):
            assert abs(value.sum() - 1.0) < 1e-12 and np.all(value > 0)
        kept = [i for i in range(len(desc)) if v.node_weight[v.words[fw[i]]] > 0]
        assert sorted(idx.tolist()) == kept and sorted(set(fw[kept].tolist())) == word.tolist()
        if levelsup >= v.L:
            assert node.tolist() == ([0] if kept else [])
        if levelsup == 0:
            assert all(v.words[fw[i]] == fn[i] for i in range(len(desc)))


def test_vocabularies_have_the_properties_the_cases_need():
    for name in G.VOCABS:
        v = G.vocab(name)
        w = v.node_weight[v.words]
        assert 0 < (w == 0).sum() or v.n_words < 10, name
        ties = sum(1 for kids in v.children for a, b in zip(kids, kids[1:]) if np.array_equal(v.descriptor[kids[0]], v.descriptor[b]))
        assert ties > 0 or name == "k2L1", name
    irr = G.vocab("k3L6irr")
    assert irr.word_id[1] >= 0 and irr.parent[1] == 0                     # a leaf at depth 1
    assert any(0 < len(k) < irr.k for k in irr.children) and G.vocab("k10L4").n_words == 10000
    kids = irr.children[0]
    assert kids != list(range(kids[0], kids[0] + len(kids)))             # siblings are not contiguous lines


def test_leaf_above_the_recording_level_is_recorded_itself():
    v = G.vocab("k3L6irr")
    d = v.descriptor[1].copy()                                           # an exact copy of the depth-1 leaf
    wid, w, nid = v.descend(d, 4)                                        # L - levelsup = 2 > depth 1
    assert wid == v.word_id[1] and nid == 1
    assert v.descend(d, 5)[2] == 1 and v.descend(d, 6)[2] == 0 and v.descend(d, 7)[2] == 0


def test_first_minimum_wins_a_tie():
    v = G.vocab("k10L3")
    for kids in v.children:
        dup = [b for b in kids[1:] if np.array_equal(v.descriptor[kids[0]], v.descriptor[b])]
        if dup and v.parent[kids[0]] == 0:
            d = v.descriptor[dup[0]]
            first = kids[0]
            nid = v.descend(d, v.L - 1)[2]                                # the node at depth 1
            assert nid == first != dup[0]
            return
    pytest.fail("the generator must duplicate a descriptor among the root's children")


def test_repeated_addition_is_not_count_times_weight():
    """addWeight adds w once per feature; with a weight whose multiples round, the two readings differ in the last bit"""
    parent = [0, 0]; leaf = [1, 1]; desc = np.zeros((2, 32), np.uint8); desc[1] = 255
    v = R.Vocabulary(2, 1, 0, 0, parent, leaf, desc, [0.1, 0.7])
    feats = np.zeros((11, 32), np.uint8); feats[10] = 255
    word, value, *_ = v.transform(feats, 0)
    a = np.float64(0.1)
    s = np.float64(0.1)
    for _ in range(9):
        s = s + a
    assert s != np.float64(10) * a                                       # 0.9999999999999999 against 1.0
    norm = s + np.float64(0.7)
    assert value.view(np.uint64).tolist() == np.array([s / norm, np.float64(0.7) / norm]).view(np.uint64).tolist()


def test_stopped_words_leave_both_vectors():
    v = R.Vocabulary(2, 1, 0, 0, [0, 0], [1, 1], np.array([[0] * 32, [255] * 32], np.uint8), [0.0, 2.0])
    feats = np.array([[0] * 32, [255] * 32, [0] * 32], np.uint8)
    word, value, node, off, idx = v.transform(feats, 0)
    assert word.tolist() == [1] and value.tolist() == [1.0] and node.tolist() == [2] and idx.tolist() == [1]
    word, value, node, off, idx = v.transform(feats[[0, 2]], 0)
    assert len(word) == len(value) == len(node) == len(idx) == 0 and off.tolist() == [0]


def test_score_is_the_dense_l1_formula_and_one_on_itself():
    r = np.random.default_rng(3)
    for _ in range(20):
        n = 200
        a = np.where(r.random(n) < 0.3, r.random(n), 0.0); b = np.where(r.random(n) < 0.3, r.random(n), 0.0)
        a /= a.sum(); b /= b.sum()
        sa = (np.nonzero(a)[0].astype(np.uint32), a[a > 0]); sb = (np.nonzero(b)[0].astype(np.uint32), b[b > 0])
        assert abs(R.score(sa, sb) - (1.0 - 0.5 * np.abs(a - b).sum())) < 1e-12
        assert abs(R.score(sa, sa) - 1.0) < 1e-12
    e = (np.zeros(0, np.uint32), np.zeros(0, np.float64))
    assert R.score(e, sa) == 0.0 and np.signbit(R.score(e, sa))          # -0 / 2: the source returns -0.0 without a common word


def test_text_loader_round_trips_and_skips_blank_lines(tmp_path):
    for name in ("k3L6irr", "k20L2"):
        v = G.vocab(name)
        u = R.Vocabulary.from_text(v.to_text() + "\n\n")
        assert (u.k, u.L, u.n_nodes, u.n_words) == (v.k, v.L, v.n_nodes, v.n_words)
        assert np.array_equal(u.parent, v.parent) and np.array_equal(u.descriptor, v.descriptor) and np.array_equal(u.word_id, v.word_id)
        assert u.node_weight.view(np.uint64).tolist() == v.node_weight.view(np.uint64).tolist() and u.children == v.children


def test_malformed_vocabularies_are_errors():
    d = np.zeros((2, 32), np.uint8)
    for args in ((21, 1, 0, 0, [0, 0], [1, 1]), (2, 1, 1, 0, [0, 0], [1, 1]), (2, 1, 0, 1, [0, 0], [1, 1]), (2, 2, 0, 0, [2, 0], [1, 0]), (2, 2, 0, 0, [0, 1], [1, 1]),
                 (2, 2, 0, 0, [0, 0], [0, 1]), (1, 1, 0, 0, [0, 0], [1, 1]), (2, 0, 0, 0, [0, 0], [1, 1])):
        with pytest.raises(ValueError):
            R.Vocabulary(*args, d, [1.0, 1.0])


# ---- KeyFrameDatabase quirks: two-word vocabularies, BowVectors written by hand ----
def bow(*pairs):
    return (np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.float64))


def test_min_common_words_truncates_a_float_product():
    # maxCommonWords = 5: 5 * 0.8f = 4.0000000596 -> 4 (an entry with 4 common words is NOT scored); in exact arithmetic 4.0 too, but 10 * 0.8f = 8.000000119 -> 8
    db = R.KeyFrameDatabase(16)
    q = R.KeyFrame(1, bow(*[(w, 0.1) for w in range(10)]))
    a = R.KeyFrame(0, bow(*[(w, 0.1) for w in range(10)]), "a"); b = R.KeyFrame(0, bow(*[(w, 0.125) for w in range(8)]), "b"); c = R.KeyFrame(0, bow(*[(w, 1 / 9) for w in range(9)]), "c")
    for o in (a, b, c):
        db.add(o)
    out = db.DetectRelocalizationCandidates(q)
    assert b.mRelocScore == 0 and b.mnRelocWords == 8 and c.mRelocScore > 0 and a.mRelocScore == 1      # 8 > 8 is false, 9 > 8 holds
    assert [o.name for o in out] == ["a", "c"]


def test_float_score_is_truncated_from_the_double():
    q = R.KeyFrame(1, bow((0, 1 / 3), (1, 2 / 3))); a = R.KeyFrame(0, bow((0, 0.3), (1, 0.7)), "a")
    db = R.KeyFrameDatabase(2); db.add(a)
    db.DetectRelocalizationCandidates(q)
    s = R.score(q.bow, a.bow)
    assert a.mRelocScore == np.float32(s) and np.float64(a.mRelocScore) != s and a.mRelocScore.dtype == np.float32


def test_loop_variant_starts_at_min_score_and_reloc_at_zero():
    def setup():
        db = R.KeyFrameDatabase(2)
        a = R.KeyFrame(0, bow((0, 0.5), (1, 0.5)), "a"); b = R.KeyFrame(0, bow((0, 0.9), (1, 0.1)), "b")
        db.add(a); db.add(b)
        return db, a, b
    q = R.KeyFrame(7, bow((0, 0.5), (1, 0.5)))
    db, a, b = setup()
    assert [o.name for o in db.DetectRelocalizationCandidates(q)] == ["a"]          # 0.6 is not above 0.75 * 1.0
    db, a, b = setup()
    assert [o.name for o in db.DetectLoopCandidates(q, 0.7)] == ["a"] and b.mLoopScore == np.float32(0.6)      # b scored, but below minScore: not kept
    db, a, b = setup()
    assert db.DetectLoopCandidates(q, 1.5) == [] and a.mLoopScore == 1              # nothing reaches minScore; the fields are written all the same
    db, a, b = setup()
    q2 = R.KeyFrame(7, bow((0, 0.9), (1, 0.1)))
    a.neighbours = [b]
    # loop: bestAccScore starts at minScore = 1.9: a's accumulated 0.6 + 1.0 = 1.6 and b's 1.0 are both below 0.75 * 1.9 -> none; reloc starts at 0 -> b via a's group
    assert db.DetectLoopCandidates(q2, 0.5) != [] and [o.name for o in db.DetectLoopCandidates(R.KeyFrame(8, q2.bow), 0.5)] == ["b"]


def test_reloc_adds_a_neighbours_stale_score_and_loop_tests_the_words():
    db = R.KeyFrameDatabase(12)
    a = R.KeyFrame(0, bow(*[(w, 0.1) for w in range(10)]), "a"); n = R.KeyFrame(0, bow((0, 1.0)), "n")
    db.add(a); db.add(n); a.neighbours = [n]
    n.mRelocScore = np.float32(0.5); n.mLoopScore = np.float32(0.5)                 # left by an earlier query
    q = R.KeyFrame(3, bow(*[(w, 0.1) for w in range(10)]))
    db.DetectRelocalizationCandidates(q)
    assert n.mnRelocQuery == 3 and n.mnRelocWords == 1 and n.mRelocScore == np.float32(0.5)       # n shares 1 word of 10: not scored now, its old score is added below
    acc = []
    orig = db._retain
    db._retain = lambda a_, b_: acc.append((a_, b_)) or orig(a_, b_)
    db.DetectRelocalizationCandidates(R.KeyFrame(4, q.bow))
    assert acc[0][0][0][0] == np.float32(1.5)
    acc.clear()
    db.DetectLoopCandidates(R.KeyFrame(5, q.bow), 0.0)
    assert acc[0][0][0][0] == np.float32(1.0)                                       # the loop variant asks mnLoopWords > minCommonWords of the neighbour: 1 > 8 fails


def test_a_repeated_query_id_accumulates_words_and_pushes_nothing():
    db = R.KeyFrameDatabase(4)
    a = R.KeyFrame(0, bow((0, 0.5), (1, 0.5)), "a"); db.add(a)
    q = R.KeyFrame(9, bow((0, 0.5), (1, 0.5)))
    assert [o.name for o in db.DetectRelocalizationCandidates(q)] == ["a"] and a.mnRelocWords == 2
    assert db.DetectRelocalizationCandidates(q) == [] and a.mnRelocWords == 4       # same id: no reset, nothing enters the list
    assert db.DetectMapFusionCandidatesFromDB(q) == [] and a.mnRelocWords == 6      # the two reloc variants share the fields
    fresh = R.KeyFrame(0, bow((0, 1.0)), "fresh"); db.add(fresh)
    assert db.DetectLoopCandidates(R.KeyFrame(0, q.bow), 0.0) == [] and fresh.mnLoopWords == 1 and a.mnLoopWords == 2      # query id 0 against fresh keyframes


def test_connected_keyframes_never_take_the_query_id():
    db = R.KeyFrameDatabase(4)
    a = R.KeyFrame(0, bow((0, 0.5), (1, 0.5)), "a"); b = R.KeyFrame(0, bow((0, 0.5), (1, 0.5)), "b"); db.add(a); db.add(b)
    q = R.KeyFrame(2, bow((0, 0.5), (1, 0.5))); q.connected = {a}
    assert [o.name for o in db.DetectLoopCandidates(q, 0.0)] == ["b"]
    assert a.mnLoopQuery == 0 and a.mnLoopWords == 1 and b.mnLoopWords == 2          # reset at every visit: 1, not 2


def test_clear_keeps_the_fields_and_order_is_word_then_insertion_and_duplicates_go():
    db = R.KeyFrameDatabase(4)
    a = R.KeyFrame(0, bow((1, 1.0)), "a"); b = R.KeyFrame(0, bow((0, 0.5), (1, 0.5)), "b"); c = R.KeyFrame(0, bow((1, 1.0)), "c")
    for o in (a, b, c):
        db.add(o)
    q = R.KeyFrame(1, bow((0, 0.5), (1, 0.5)))
    a.neighbours = [b]; c.neighbours = [b]
    # list order: b (word 0), then a and c (word 1, insertion order); a and c both name b as their best: b appears once, first
    assert [o.name for o in db.DetectRelocalizationCandidates(q)] == ["b"]
    db.erase(a); db.add(a)                                                          # a moves behind c in word 1's list
    a.neighbours = []; c.neighbours = []
    assert [o.name for o in db.DetectRelocalizationCandidates(R.KeyFrame(2, q.bow))] == ["b"]
    q3 = R.KeyFrame(3, bow((1, 1.0)))
    assert [o.name for o in db.DetectRelocalizationCandidates(q3)] == ["c", "a"]
    db.clear()
    assert a.mnRelocQuery == 3 and a.mRelocScore == 1 and db.DetectRelocalizationCandidates(R.KeyFrame(4, q.bow)) == []


@pytest.mark.parametrize("n_entries", [1, 2, 70, 300])
def test_sessions_produce_candidates_on_a_third_of_the_queries(n_entries):
    ops = G.session(n_entries); exp = G.session_expected(n_entries)
    q = [e for op, e in zip(ops, exp) if op[0] == "query"]
    assert len(ops) >= 300 and len(q) >= 60
    assert sum(1 for res, _ in q if res) * 3 >= len(q), (sum(1 for res, _ in q if res), len(q))
    kinds = [op[1] for op in ops if op[0] == "query"]
    assert set(kinds) == {0, 1, 2} and {op[3] for op in ops if op[0] == "query"} == set(range(6))
    assert any(op[0] == "clear" for op in ops) and any(op[0] == "erase" for op in ops)

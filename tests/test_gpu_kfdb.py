"""GPU tests: the keyframe database on the device (corb_kfdb_*) against the object emulation of KeyFrameDatabase.cc in tests/dbow_reference.py.  Seeded sessions of
300 and more steps (tests/bow_cases.py) on databases of 1, 2, 70 and 300 entries interleave set_bow / compute_bow, add, erase, clear, neighbour updates and the three
queries with ids from {0 .. 5}; after every query the candidate list is equal, order included, and the six fields of every entry are bit-equal.  That the sessions
produce candidates on a third of the queries is asserted on the definition alone (tests/test_dbow_reference.py)."""
import numpy as np
import pytest
import dbow_reference as R
import bow_cases as G

pytestmark = pytest.mark.gpu
MAX_WORDS = 128


@pytest.fixture(scope="module")
def voc(corb):
    f = G.vocab(G.SESSION_VOCAB).flat()
    v = corb.Vocabulary(f["k"], f["L"], f["parent"], f["is_leaf"], f["descriptor"], f["weight"])
    yield v
    v.close()


def same_state(got, want):
    return got.tobytes() == want.astype(got.dtype).tobytes()


@pytest.mark.parametrize("n_entries", [1, 2, 70, 300])
def test_session_follows_the_definition(corb, voc, n_entries):
    ops = G.session(n_entries); exp = G.session_expected(n_entries)
    db = corb.KeyFrameDatabase(voc, n_entries, MAX_WORDS)
    st = corb.KeyFrameStore(1, 128)
    n_q = n_cand = 0
    for k, (op, e) in enumerate(zip(ops, exp)):
        if op[0] == "set_bow":
            if k % 2:                                                      # ComputeBoW on a record ...
                kp = np.zeros(len(op[2]), corb.KP_DTYPE)
                st.put(0, kp, op[2]); st.compute_bow(0, voc, 4, db, [op[1]])
            else:                                                          # ... or the definition's vector set from the host
                db.set_bow(op[1], e[0], e[1])
            w, v = db.get_bow(op[1])
            assert np.array_equal(w, e[0]) and np.array_equal(v.view(np.uint64), e[1].view(np.uint64)), k
        elif op[0] == "add":
            db.add(op[1])
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "clear":
            db.clear()
        elif op[0] == "nb":
            db.set_neighbours(op[1], op[2])
        else:
            _, kind, q, qid, conn, ms = op
            got = db.detect(kind, q, qid, conn, ms)
            assert got.tolist() == e[0], (k, op[1:], got.tolist(), e[0])
            assert same_state(db.state(), e[1]), (k, op[1:])
            n_q += 1; n_cand += bool(e[0])
    assert n_q >= 60 and 3 * n_cand >= n_q
    db.close(); st.close()


def test_score_is_the_definition_bit_for_bit(corb, voc):
    v = G.vocab(G.SESSION_VOCAB)
    n = 70
    db = corb.KeyFrameDatabase(voc, n + 1, MAX_WORDS)
    bows = []
    for e, op in enumerate([o for o in G.session(n) if o[0] == "set_bow"][:n]):
        t = v.transform(op[2], 4); bows.append((t[0], t[1])); db.set_bow(e, t[0], t[1])
    db.set_bow(n, np.zeros(0, np.uint32), np.zeros(0, np.float64)); bows.append((np.zeros(0, np.uint32), np.zeros(0, np.float64)))
    for a in (0, 7, n):
        got = db.score(a, np.arange(n + 1))
        want = np.array([R.score(bows[a], b) for b in bows], np.float64)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), a
    assert db.score(7, [7])[0] == 1.0 or abs(db.score(7, [7])[0] - 1.0) < 1e-12
    assert len(db.score(0, [])) == 0
    db.close()


def bow(*pairs):
    return np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.float64)


def test_further_cases(corb, voc):
    db = corb.KeyFrameDatabase(voc, 6, 16)
    zero = np.zeros(6, corb.KFDB_STATE_DTYPE)
    db.set_bow(0, *bow((3, 0.5), (9, 0.5)))
    for kind in (0, 1, 2):                                                 # empty database
        assert len(db.detect(kind, 0, 5)) == 0
    assert same_state(db.state(), zero)
    db.set_bow(1, *bow((4, 0.5), (10, 0.5))); db.add(1)
    for kind in (0, 1, 2):                                                 # a query that shares no word
        assert len(db.detect(kind, 0, 5)) == 0
    assert same_state(db.state(), zero)
    db.add(0)                                                              # a query that is itself live: it is its own best candidate
    assert db.DetectRelocalizationCandidates(0, 5).tolist() == [0]
    s = db.state()
    assert s["reloc_query"][0] == 5 and s["reloc_words"][0] == 2 and s["reloc_score"][0] == 1 and s["reloc_query"][1] == 0
    for e in (2, 3, 4):
        db.set_bow(e, *bow((3, 0.4), (9, 0.6))); db.add(e)
    assert db.DetectLoopCandidates(0, 6, [0, 1, 2, 3, 4, 5], 0.0).tolist() == []          # all entries connected
    s = db.state()
    assert s["loop_query"].tolist() == [0] * 6 and s["loop_words"].tolist() == [1, 0, 1, 1, 1, 0]
    assert db.DetectLoopCandidates(0, 6, [], 0.0).tolist() == [0, 2, 3, 4]
    with pytest.raises(corb.CorbError, match="4 candidates, room for 2"):  # cap too small: the size needed comes back
        db.detect(2, 0, 7, cap=2)
    assert db.last_count == 4 and db.state()["reloc_query"].tolist() == [7, 0, 7, 7, 7, 0]
    import ctypes as C
    n = C.c_int(-1)
    assert corb.load().corb_kfdb_detect(db.h, 2, 0, 8, None, 0, C.c_float(0), None, 0, C.byref(n)) == -5 and n.value == 4
    db.close()


def test_argument_errors(corb, voc):
    db = corb.KeyFrameDatabase(voc, 3, 4)
    for bad, msg in ((lambda: corb.KeyFrameDatabase(voc, 0, 4), "bad argument"), (lambda: corb.KeyFrameDatabase(voc, 3, 0), "bad argument"),
                     (lambda: db.set_bow(3, *bow((1, 1.0))), "bad database / entry"), (lambda: db.set_bow(0, *bow((2, 0.5), (1, 0.5))), "ascend"),
                     (lambda: db.set_bow(0, *bow((1000, 1.0))), "ascend"),
                     (lambda: db.set_bow(0, *bow((1, 0.0))), "not above 0"), (lambda: db.set_bow(0, *bow((1, 0.5), (2, float("nan")))), "not above 0"), (lambda: db.set_bow(0, *bow((1, -0.5))), "not above 0"), (lambda: db.set_bow(0, *bow(*[(w, 0.2) for w in range(5)])), "5 words"),
                     (lambda: db.add(0), "no BowVector"), (lambda: db.erase(0), "not in the database"), (lambda: db.detect(1, 0, 1), "no BowVector"),
                     (lambda: db.get_bow(0), "no BowVector"), (lambda: db.score(0, [1]), "no BowVector"), (lambda: db.set_neighbours(0, [3] + [-1] * 9), "outside"),
                     (lambda: db.set_neighbours(3, [-1] * 10), "outside")):
        with pytest.raises(corb.CorbError, match=msg):
            bad()
    db.set_bow(0, *bow((1, 1.0))); db.add(0)
    for bad, msg in ((lambda: db.add(0), "already"), (lambda: db.set_bow(0, *bow((1, 1.0))), "erase it first"), (lambda: db.detect(3, 0, 1), "kind"),
                     (lambda: db.detect(0, 0, 1, [3]), "outside"), (lambda: db.detect(0, 0, 1, [], float("nan")), "NaN"), (lambda: db.score(0, [1]), "no BowVector")):
        with pytest.raises(corb.CorbError, match=msg):
            bad()
    db.close()

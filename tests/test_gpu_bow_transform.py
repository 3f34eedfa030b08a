"""GPU tests: the vocabulary transform on the device (corb_voc_*, corb_kf_store_compute_bow) against tests/dbow_reference.py, bit for bit: words, FeatureVector arrays,
per-feature word and node, and the BowVector's values as uint64.  Vocabularies and feature sets: tests/bow_cases.py (k = 2, 3, 10 on groups of 16 lanes, k = 20 on 32;
an irregular tree with a leaf at depth 1; stopped words; sibling ties).  n in {0, 1, 63, 64, 65, 257} crosses the 16- and 8-feature workgroups of the descent and the
powers of two of the sort; n = 8192 is the LDS limit."""
import numpy as np
import pytest
import bow_cases as G

pytestmark = pytest.mark.gpu
NS = (0, 1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def vocs(corb):
    out = {}
    for name in G.VOCABS:
        f = G.vocab(name).flat()
        out[name] = corb.Vocabulary(f["k"], f["L"], f["parent"], f["is_leaf"], f["descriptor"], f["weight"])
    yield out
    for v in out.values():
        v.close()


def same(got, want, what):
    names = ("word", "value", "fv_node", "fv_off", "fv_idx", "feat_word", "feat_node")
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, names[k], g.shape, w.shape)
        if g.dtype == np.float64:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, names[k])
        else:
            assert np.array_equal(g, w), (what, names[k])


@pytest.mark.parametrize("name", sorted(G.VOCABS))
def test_transform_is_the_definition_bit_for_bit(vocs, name):
    v = G.vocab(name)
    info = vocs[name].info()
    assert info == dict(k=v.k, L=v.L, n_nodes=v.n_nodes, n_words=v.n_words)
    for levelsup in (0, 2, 4, v.L, v.L + 1):
        got = vocs[name].transform_sets([G.features(name, n, 40 + n) for n in NS], levelsup, per_feature=True)      # a batch of sets of different sizes
        for n, g in zip(NS, got):
            same(g, G.expected(name, n, 40 + n, levelsup), (name, n, levelsup))
    for n in (1, 65):                                                        # ... equals the single calls
        same(vocs[name].transform(G.features(name, n, 40 + n), 4, per_feature=True), G.expected(name, n, 40 + n, 4), (name, n, "single"))


def test_a_set_of_stopped_words_gives_two_empty_vectors(vocs):
    v = G.vocab("k10L3")
    cand = np.random.default_rng(5).integers(0, 256, (1500, 32), dtype=np.uint8)
    desc = np.array([d for d in cand if v.descend(d, 2)[1] == 0][:10])      # features whose descent ends in a stopped word
    assert len(desc) == 10
    want = v.transform(desc, 2, per_feature=True)
    assert len(want[0]) == 0 and len(want[2]) == 0 and want[3].tolist() == [0]
    same(vocs["k10L3"].transform(desc, 2, per_feature=True), want, "stopped")


def test_text_loader_equals_create(corb, vocs, tmp_path):
    for name in ("k3L6irr", "k20L2"):
        p = tmp_path / (name + ".txt"); p.write_text(G.vocab(name).to_text() + "\n")
        t = corb.Vocabulary.from_text(str(p))
        assert t.info() == vocs[name].info()
        d = G.features(name, 257, 9)
        same(t.transform(d, 2, per_feature=True), vocs[name].transform(d, 2, per_feature=True), name)
        t.close()


def test_argument_errors(corb, vocs, tmp_path):
    f = G.vocab("k2L1").flat()
    def make(**kw):
        a = dict(f); a.update(kw)
        return corb.Vocabulary(a["k"], a["L"], a["parent"], a["is_leaf"], a["descriptor"], a["weight"], a["scoring"], a["weighting"])
    for kw, msg in ((dict(k=21), "k must"), (dict(L=0), "k must"), (dict(L=11), "k must"), (dict(scoring=1), "L1_NORM"), (dict(weighting=2), "TF_IDF"),
                    (dict(parent=np.array([2, 0], np.int32), is_leaf=np.array([1, 0], np.int32), L=2), "not before"),
                    (dict(parent=np.array([0, 1], np.int32), L=2), "is a leaf"), (dict(is_leaf=np.array([0, 1], np.int32)), "neither"), (dict(k=1), "more than k"),
                    (dict(parent=np.zeros(0, np.int32), is_leaf=np.zeros(0, np.int32), descriptor=np.zeros((0, 32), np.uint8), weight=np.zeros(0)), "empty")):
        with pytest.raises(corb.CorbError, match=msg):
            make(**kw)
    with pytest.raises(corb.CorbError, match="cannot open"):
        corb.Vocabulary.from_text(str(tmp_path / "missing.txt"))
    bad = tmp_path / "bad.txt"; bad.write_text("2 1 0 0\n0 1 1 2 3\n")                                       # a short line
    with pytest.raises(corb.CorbError, match="line 2"):
        corb.Vocabulary.from_text(str(bad))
    bad.write_text("2 1 3 0\n")
    with pytest.raises(corb.CorbError, match="L1_NORM"):
        corb.Vocabulary.from_text(str(bad))
    with pytest.raises(corb.CorbError, match="8192"):
        vocs["k2L1"].transform(np.zeros((corb.BOW_MAX_FEATURES + 1, 32), np.uint8), 0)
    L = corb.load(); off = np.array([1, 2], np.int32); z = np.zeros(8, np.int64)
    assert L.corb_voc_transform(vocs["k2L1"].h, corb._p(z), corb._p(off), 1, 0, *[corb._p(z)] * 7, None, None) == -1      # offset[0] != 0
    assert L.corb_voc_transform(None, corb._p(z), corb._p(off), 1, 0, *[corb._p(z)] * 7, None, None) == -1
    assert L.corb_voc_transform(vocs["k2L1"].h, corb._p(z), corb._p(off), 65536, 0, *[corb._p(z)] * 7, None, None) == -1      # the sets are one grid dimension
    assert b"at most 65535" in L.corb_last_error()


def kp_of(corb, n):
    kp = np.zeros(n, corb.KP_DTYPE); kp["angle"] = np.arange(n) % 360; kp["x"] = np.arange(n); kp["octave"] = 0
    return kp


def test_compute_bow_on_records(corb, vocs):
    name = "k10L3"; F = 512
    st = corb.KeyFrameStore(4, F)
    db = corb.KeyFrameDatabase(vocs[name], 4, F)
    ns = (F, 257, 0)
    big = G.features(name, F, 70)
    descs = [big, big[100:357].copy(), big[:0]]                              # slot 1 sees part of slot 0: the matcher below has something to find
    wants = [G.vocab(name).transform(d, 2) for d in descs]
    for s, d in enumerate(descs):
        st.put(s, kp_of(corb, len(d)), d, keyframe_id=10 + s)
    nbytes = st.record_bytes()
    st.compute_bow([0, 1, 2], vocs[name], 2, db, [3, 1, 0])
    assert st.record_bytes() == nbytes == corb.KeyFrameStore(1, F).record_bytes()
    for s, e, n in zip((0, 1, 2), (3, 1, 0), ns):
        want = wants[s]
        got = st.get(s)
        assert np.array_equal(got["desc"], descs[s]) and got["id"] == 10 + s
        for g, w in zip(got["fv"], want[2:5]):
            assert np.array_equal(g, w), (s, g, w)
        w, v = db.get_bow(e)
        assert np.array_equal(w, want[0]) and np.array_equal(v.view(np.uint64), want[1].view(np.uint64))
    assert np.all(db.state().view(np.uint8) == 0)
    # SearchByBoW on slots after compute_bow == after set_bow with the definition's vector
    flags = np.ones(F, np.uint8)
    st.set_flags(0, flags); st.set_flags(1, flags[:257])
    ref = corb.KeyFrameStore(2, F)
    for s in (0, 1):
        ref.put(s, kp_of(corb, len(descs[s])), descs[s], keyframe_id=10 + s)
        ref.set_bow(s, wants[s][2:5])
        ref.set_flags(s, flags[:ns[s]])
    L = corb.load()
    import ctypes as C
    def search(store):
        m = np.full(F, -7, np.int32); k = C.c_int(0)
        assert L.corb_search_by_bow_slots(1, store.h, 0, store.h, 1, C.c_float(0.9), 1, corb._p(m), C.byref(k)) == 0
        return m, k.value
    (ma, ka), (mb, kb) = search(st), search(ref)
    assert np.array_equal(ma, mb) and ka == kb and ka > 20
    # without a database the FeatureVector is written all the same
    st.put(3, kp_of(corb, 65), G.features(name, 65, 3))
    st.compute_bow(3, vocs[name], 4)
    for g, w in zip(st.get(3)["fv"], G.expected(name, 65, 3, 4)[2:5]):
        assert np.array_equal(g, w)
    # errors: a live entry, a slot twice, a database too small for the words
    db.add(1)
    with pytest.raises(corb.CorbError, match="erase it first"):
        st.compute_bow([1], vocs[name], 2, db, [1])
    with pytest.raises(corb.CorbError, match="twice"):
        st.compute_bow([1, 1], vocs[name], 2, db, [0, 2])
    with pytest.raises(corb.CorbError, match="share a device"):
        st.compute_bow([1], vocs["k2L1"], 2, db, [0])
    small = corb.KeyFrameDatabase(vocs[name], 2, 8)
    with pytest.raises(corb.CorbError, match="words, the database holds 8"):
        st.compute_bow([0], vocs[name], 2, small, [0])
    with pytest.raises(corb.CorbError, match="no BowVector"):
        small.add(0)
    for o in (small, db, ref, st):
        o.close()


def test_lds_limit(corb, vocs):
    """n = 8192 features is the largest set (128 KiB of LDS); a store of 8193 features per keyframe is an argument error"""
    name = "k10L4"; n = corb.BOW_MAX_FEATURES
    v = G.vocab(name); r = np.random.default_rng(11)
    leaves = v.words[r.integers(0, v.n_words, 3000)]
    desc = v.descriptor[leaves[r.integers(0, 3000, n)]].copy()
    desc[::5, 3] ^= 1
    got = vocs[name].transform(desc, 2, per_feature=True)
    want = v.transform(desc, 2, per_feature=True)
    same(got, want, "limit")
    st = corb.KeyFrameStore(1, n); st.put(0, kp_of(corb, n), desc)
    st.compute_bow(0, vocs[name], 2)
    for g, w in zip(st.get(0)["fv"], want[2:5]):
        assert np.array_equal(g, w)
    st.close()
    big = corb.KeyFrameStore(1, n + 1)
    with pytest.raises(corb.CorbError, match="8192"):
        big.compute_bow(0, vocs[name], 2)
    big.close()

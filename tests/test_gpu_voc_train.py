"""GPU tests: vocabulary training on the device (include/corb_voc_train.h) against tests/voctrain_reference.py.  Every assertion is exact: integers, and doubles compared
as uint64.  The sizes are the smallest that still cross each boundary: n <= k (trivial nodes), one workgroup per node, several tiles of 1024 per node (3000 features),
k = 20 (the 32-lane descent), and CORB_VOC_TRAIN_SMALL at 0 and 64 for the multi-workgroup kernels on small and mixed levels."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest

import dbow_reference as R
import voctrain_reference as V
import voctrain_cases as G

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))


def train(corb, name):
    sets, k, L, seed, max_it = G.inputs(name)
    return corb.Vocabulary.train(sets, k, L, seed, max_it)


def check(v, name):
    flat, st = G.expected(name)
    got = v.flat()
    assert G.same_flat(got, flat), name
    assert v.info() == dict(k=flat["k"], L=flat["L"], n_nodes=st["nodes"], n_words=st["words"])
    ts = v.train_stats
    for f in V.STAT_FIELDS + ("level_nodes", "level_max_iterations"):
        assert ts[f] == st[f], (name, f, ts[f], st[f])
    assert ts["launches"] > sum(ts["level_launches"]) > 0 and ts["elapsed_ms"] > 0        # the weights' launches come on top of the levels'


def same(got, want, what):
    """the transform tests' rule: same dtypes and shapes, integers equal, doubles equal as uint64"""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.shape, w.shape)
        if g.dtype == np.float64:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, k)
        else:
            assert np.array_equal(g, w), (what, k)


@pytest.mark.parametrize("name", G.CORE)
def test_train_equals_the_definition(corb, name):
    v = train(corb, name)
    check(v, name)
    if len(G.inputs(name)[0]) == 1:
        assert not v.flat()["weight"].any()                     # one image: ln(1 / 1)
    v.close()


@pytest.mark.parametrize("name", ["lowent", "repeat"])
def test_special_inputs(corb, name):
    low, rep = G.expected("lowent")[1], G.expected("repeat")[1]
    assert low["trivial_nodes"] >= 1 and low["tie_bits"] >= 1 and rep["short_nodes"] >= 1      # the rare branches are there, by the definition's own count
    v = train(corb, name)
    check(v, name)
    v.close()


@pytest.mark.parametrize("name", ["cap1", "cap2", "cap2small"])
def test_iteration_cap(corb, name):
    assert G.expected(name)[1]["capped_nodes"] >= 1 and G.expected(name)[1]["max_iterations_seen"] == G.CASES[name][6]
    v = train(corb, name)
    check(v, name)
    v.close()


def test_small_node_switch_gives_the_same_bytes(corb):
    names = ["k10L3n3000", "lowent"]
    runs = {}
    for value in ("0", "64", None):
        env = dict(os.environ)
        env.pop("CORB_VOC_TRAIN_SMALL", None)
        if value is not None:
            env["CORB_VOC_TRAIN_SMALL"] = value
        p = subprocess.run([sys.executable, os.path.join(TESTS, "voctrain_cases.py")] + names, capture_output=True, text=True, timeout=120, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        runs[value] = json.loads(p.stdout.strip().split("\n")[-1])
    for name in names:
        want = G.digest(*G.expected(name))
        for value in runs:
            assert runs[value][name]["digest"] == want, (name, value)
        assert runs["0"][name]["small"] == 0 and runs["0"][name]["large"] > 0 and runs["0"][name]["small_limit"] == 0
        assert runs["64"][name]["small"] > 0 and runs["64"][name]["large"] > 0 and runs["64"][name]["small_limit"] == 64      # both kernel families ran
        assert runs[None][name]["small_limit"] == 2048 and runs[None][name]["small"] > 0


def test_determinism_and_use(corb):
    sets, k, L, seed, max_it = G.inputs("k10L3n3000")
    a = corb.Vocabulary.train(sets, k, L, seed, max_it); b = corb.Vocabulary.train(sets, k, L, seed, max_it); c = corb.Vocabulary.train(sets, k, L, seed + 1, max_it)
    fa = a.flat()
    assert G.same_flat(fa, b.flat()) and not G.same_flat(fa, c.flat())
    ref = R.Vocabulary(**fa)
    fresh = [G.descriptors("clustered", n, np.random.default_rng(77 + n)) for n in (0, 1, 65, 257)]
    for levelsup in (0, 2):
        for d, got in zip(fresh, a.transform_sets(fresh, levelsup, per_feature=True)):
            same(got, ref.transform(d, levelsup, per_feature=True), (len(d), levelsup))
    for v in (a, b, c):
        v.close()


def kp_of(corb, n):
    kp = np.zeros(n, corb.KP_DTYPE); kp["angle"] = np.arange(n) % 360; kp["x"] = np.arange(n); kp["octave"] = 0
    return kp


def test_train_store_equals_train(corb):
    rng = np.random.default_rng(31)
    sizes = [64, 512, 0, 300, 129, 257]
    descs = [G.descriptors("clustered", n, rng) if n else np.zeros((0, 32), np.uint8) for n in sizes]
    st = corb.KeyFrameStore(8, 512)
    slots = [5, 0, 2, 7, 3, 1]
    for s, d in zip(slots, descs):
        st.put(s, kp_of(corb, len(d)), d, keyframe_id=100 + s)
    a = corb.Vocabulary.train_store(st, slots, 6, 3, 9)
    b = corb.Vocabulary.train(descs, 6, 3, 9)
    assert G.same_flat(a.flat(), b.flat()) and G.same_flat(a.flat(), V.create(descs, 6, 3, 9)[0])
    for f in V.STAT_FIELDS:
        assert a.train_stats[f] == b.train_stats[f]
    db = corb.KeyFrameDatabase(a, 8, 512)
    st.compute_bow(slots, a, 2, db, list(range(6)))
    ref = R.Vocabulary(**a.flat())
    for e, d in enumerate(descs):
        w, v = db.get_bow(e); want = ref.transform(d, 2)
        assert np.array_equal(w, want[0]) and np.array_equal(v.view(np.uint64), want[1].view(np.uint64))
    with pytest.raises(corb.CorbError, match="slot 0 is listed twice"):
        corb.Vocabulary.train_store(st, [5, 0, 0], 6, 3, 9)
    with pytest.raises(corb.CorbError, match="no training feature"):
        corb.Vocabulary.train_store(st, [2], 6, 3, 9)
    db.close(); a.close(); b.close(); st.close()


def test_get_and_save_text(corb, tmp_path):
    v = train(corb, "k3L3n200")
    flat = G.expected("k3L3n200")[0]
    p17, p0 = str(tmp_path / "v17.txt"), str(tmp_path / "v0.txt")
    v.save_text(p17, 17); v.save_text(p0)
    assert G.same_flat(R.Vocabulary.from_text(open(p17).read()).flat(), flat)
    t = corb.Vocabulary.from_text(p17)
    assert G.same_flat(t.flat(), v.flat())                      # reloads bit for bit
    assert open(p0, "rb").read() == V.save_text(flat, 0).encode() and open(p17, "rb").read() == V.save_text(flat, 17).encode()
    assert open(p0).readline() == "3 3  0 0\n" and open(p0).readlines()[1].split(" ")[-2] == ""      # the reference's spacing
    t.close(); v.close()
    # get on a vocabulary made by corb_voc_create returns what went in, inner nodes' weights included
    import bow_cases
    f = bow_cases.vocab("k3L6irr").flat(); f["weight"] = f["weight"] + np.arange(len(f["weight"])) * 0.125
    c = corb.Vocabulary(f["k"], f["L"], f["parent"], f["is_leaf"], f["descriptor"], f["weight"])
    assert G.same_flat(c.flat(), f)
    with pytest.raises(corb.CorbError, match="%d nodes, room for %d" % (len(f["parent"]), len(f["parent"]) - 1)):
        c.flat(cap_nodes=len(f["parent"]) - 1)
    import ctypes
    n = ctypes.c_int(0)
    assert corb.load().corb_voc_get(c.h, None, None, None, None, 0, ctypes.byref(n)) == -5 and n.value == len(f["parent"])      # CORB_ERR_OVERFLOW with the count
    with pytest.raises(corb.CorbError, match="weight_digits"):
        c.save_text(p0, 18)
    c.close()


def test_argument_errors(corb):
    sets, k, L, seed, _ = G.inputs("k3L3n200")
    for kw, msg in ((dict(k=1), r"k must be in \[2, 20\]"), (dict(k=21), r"k must be in \[2, 20\]"), (dict(L=0), r"L must be in \[1, 10\]"), (dict(L=11), r"L must be in \[1, 10\]"),
                    (dict(max_iterations=0), "max_iterations must be at least 1")):
        a = dict(k=k, L=L, seed=seed, max_iterations=100); a.update(kw)
        with pytest.raises(corb.CorbError, match=msg):
            corb.Vocabulary.train(sets, **a)
    with pytest.raises(corb.CorbError, match="no training feature"):
        corb.Vocabulary.train([sets[1], sets[1]], k, L, seed)
    d = np.ascontiguousarray(np.concatenate(sets))
    with pytest.raises(corb.CorbError, match=r"offset\[0\] != 0"):
        corb.Vocabulary._train_raw(d, np.array([1, 50, 200], np.int32), k, L, seed, 100, 0)
    with pytest.raises(corb.CorbError, match="offset decreases at image 1"):
        corb.Vocabulary._train_raw(d, np.array([0, 150, 100, 200], np.int32), k, L, seed, 100, 0)

"""GPU tests of map-fusion detection for a whole submap (include/corb_map_fusion.h): corb_kfdb_detect_batch, corb_search_by_bow_slots_batch and
corb_map_fusion_candidates_store against the definition (tests/fusion_reference.py, the oracle's SearchByBoW) and, byte for byte, against the single calls the
project already has, called one after the other in the same process.  The generators' conditions are asserted on the definition alone in
tests/test_fusion_reference.py.  The C++ mirror and corb::adapt::MapFusionDetectT run in a host program of their own (tests/host/fusion_adapter_main.cpp)."""
import os
import struct
import subprocess
import numpy as np
import pytest
import bow_cases as G
import fusion_cases as FC
import fusion_reference as F

pytestmark = pytest.mark.gpu
PATTERN_A, PATTERN_B = 0x00000001, 0x3F800000          # the fills of tests/test_gpu_workspace_states.py: a plausible count or index; 1.0f


def _voc(corb, name):
    f = G.vocab(name).flat()
    return corb.Vocabulary(f["k"], f["L"], f["parent"], f["is_leaf"], f["descriptor"], f["weight"])


@pytest.fixture(scope="module")
def voc(corb):
    v = _voc(corb, G.SESSION_VOCAB)
    yield v
    v.close()


def _same_state(got, want):
    return got.tobytes() == want.astype(got.dtype).tobytes()


def _single(db, entries, ids, kind=2):
    """the earlier route: one corb_kfdb_detect per query -> (offsets, candidates)"""
    off, cand = [0], []
    for e, i in zip(entries, ids):
        cand += db.detect(kind, int(e), int(i)).tolist(); off.append(len(cand))
    return np.array(off, np.int32), np.array(cand, np.int32)


# ---------------------------------------------------------------- (a) detect_batch ----------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, "1", "3"])
@pytest.mark.parametrize("n", [1, 2, 70, 300])
def test_detect_batch_equals_the_definition_and_the_single_calls(corb, voc, monkeypatch, n, chunk):
    if chunk is None:
        monkeypatch.delenv("CORB_KFDB_BATCH_CHUNK", raising=False)
    else:
        monkeypatch.setenv("CORB_KFDB_BATCH_CHUNK", chunk)
    entries, ids = FC.queries(n)
    want_off, want_cand, _, want_state = FC.expected(n)
    db = FC.build(corb, voc, n); twin = FC.build(corb, voc, n)
    off, cand = db.detect_batch(2, entries, ids)
    s_off, s_cand = _single(twin, entries, ids)
    assert off.tolist() == want_off.tolist() == s_off.tolist()
    assert cand.tolist() == want_cand.tolist() == s_cand.tolist()
    assert _same_state(db.state(), want_state) and db.state().tobytes() == twin.state().tobytes()
    if n == 70:                                         # a second call: a stored mnRelocQuery equal to a query id, an entry listed twice
        e2, i2 = FC.repeat_queries(db.state())
        ref = FC.database(n)[0].copy(); ref.state = want_state.copy()
        w_off, w_cand, _ = F.detect_batch(ref, e2, i2)
        off, cand = db.detect_batch(1, e2, i2); s_off, s_cand = _single(twin, e2, i2, kind=1)
        assert off.tolist() == w_off.tolist() == s_off.tolist() and cand.tolist() == w_cand.tolist() == s_cand.tolist()
        assert _same_state(db.state(), ref.state) and db.state().tobytes() == twin.state().tobytes()
    db.close(); twin.close()


def test_the_chunk_switch_sets_the_number_of_passes(corb, voc, monkeypatch):
    """the switch is read at every call: 144 queries run as one pass by default (2^20 / 128 queries fit), as 48 passes of 3 and as 144 of 1"""
    entries, ids = FC.queries(70)
    corb.bow_profile(True)
    try:
        for chunk, passes in ((None, 1), ("3", 48), ("1", 144), ("1000", 1)):
            if chunk is None:
                monkeypatch.delenv("CORB_KFDB_BATCH_CHUNK", raising=False)
            else:
                monkeypatch.setenv("CORB_KFDB_BATCH_CHUNK", chunk)
            db = FC.build(corb, voc, 70)
            corb.bow_profile_read()
            db.detect_batch(2, entries, ids)
            prof = corb.bow_profile_read()
            assert [prof[k][1] for k in ("fusion_common_kernel", "fusion_walk_kernel", "fusion_score_kernel", "fusion_seen_kernel", "fusion_select_kernel", "fusion_append_kernel")] == [passes] * 6, (chunk, prof)
            db.close()
    finally:
        corb.bow_profile(False)


def test_detect_batch_on_vectors_of_more_than_64_words(corb):
    """several ballot rounds per entry and several search steps per word: BowVectors of 365 .. 475 words on k10L4"""
    v = _voc(corb, FC.WIDE_VOCAB)
    ops = FC.wide_database()[1]; entries, ids = FC.wide_queries()
    want_off, want_cand, _, want_state = FC.wide_expected()
    db = corb.KeyFrameDatabase(v, FC.WIDE_N, 512); twin = corb.KeyFrameDatabase(v, FC.WIDE_N, 512)
    FC.apply_ops(db, ops); FC.apply_ops(twin, ops)
    off, cand = db.detect_batch(2, entries, ids); s_off, s_cand = _single(twin, entries, ids)
    assert off.tolist() == want_off.tolist() == s_off.tolist() and cand.tolist() == want_cand.tolist() == s_cand.tolist()
    assert _same_state(db.state(), want_state) and db.state().tobytes() == twin.state().tobytes()
    db.close(); twin.close(); v.close()


def test_detect_batch_arguments_and_overflow(corb, voc):
    n = 70
    db = FC.build(corb, voc, n)
    entries, ids = FC.queries(n)
    before = db.state().tobytes()
    no_bow = corb.KeyFrameDatabase(voc, 2, 8)
    for bad, msg in ((lambda: db.detect_batch(0, entries, ids), "kind"), (lambda: db.detect_batch(3, entries, ids), "kind"),
                     (lambda: db.detect_batch(2, [0, 1, 2], [5, 6, 5]), "listed twice"), (lambda: db.detect_batch(2, [0, n + FC.EXTRA], [5, 6]), "outside the database"),
                     (lambda: db.detect_batch(2, [0, -1], [5, 6]), "outside the database"), (lambda: no_bow.detect_batch(2, [0], [5]), "no BowVector"),
                     (lambda: db.detect_batch(2, np.zeros(65536, np.int32), np.arange(65536)), "queries per call")):
        with pytest.raises(corb.CorbError, match=msg):
            bad()
        assert db.last_rc == -1
    assert db.state().tobytes() == before                                   # CORB_ERR_ARG: nothing changed
    off, cand = db.detect_batch(2, [], [])
    assert off.tolist() == [0] and len(cand) == 0 and db.state().tobytes() == before
    want_off, want_cand, _, want_state = FC.expected(n)
    with pytest.raises(corb.CorbError, match="%d candidates, room for 10" % len(want_cand)):
        db.detect_batch(2, entries, ids, cap=10)
    assert db.last_rc == -5 and db.last_count == len(want_cand) and db.last_offsets.tolist() == want_off.tolist()
    assert _same_state(db.state(), want_state)                              # CORB_ERR_OVERFLOW: the fields are updated all the same
    db.close(); no_bow.close()


# ---------------------------------------------------------------- (b) SearchByBoW_batch ----------------------------------------------------------------
@pytest.fixture(scope="module")
def match_stores(corb, synth):
    """two stores of 8 keyframes, 60 .. 300 features each, views of one scene (so pairs match); slot 7 of each stays empty, slot 6 of B shares no node with anyone"""
    rng = np.random.default_rng(31)
    base = synth.correlated_descriptors(300, rng); base_angle = rng.uniform(0, 360, 300).astype(np.float32)
    A = corb.KeyFrameStore(8, 320); B = corb.KeyFrameStore(8, 320); host = {}
    for name, store in (("A", A), ("B", B)):
        for s in range(7):
            n = int(rng.integers(60, 301))
            src = rng.permutation(300)[:n]                  # (distinct scene points: a feature has one twin per other keyframe)
            bits = np.unpackbits(base[src], axis=1); bits ^= (rng.random(bits.shape) < 0.04).astype(np.uint8)
            desc = np.packbits(bits, axis=1)
            angle = ((base_angle[src] + rng.normal(0, 8, n)) % 360).astype(np.float32)
            node = np.where(rng.random(n) < 0.05, -1, src % 9)    # the vocabulary node follows the scene point; a few features have none
            ids = np.unique(node[node >= 0]); groups = [np.nonzero(node == k)[0] for k in ids]
            fv = ((ids * 7 + 3 + (name == "B" and s == 6)).astype(np.uint32), np.cumsum([0] + [len(g) for g in groups]).astype(np.int32), np.concatenate(groups).astype(np.uint32))
            valid = (rng.random(n) < 0.8).astype(np.uint8)
            kp = np.zeros(n, corb.KP_DTYPE); kp["angle"] = angle
            store.put(s, kp, desc, keyframe_id=100 * (name == "B") + s); store.set_bow(s, fv); store.set_flags(s, valid)
            host[name, s] = (desc, angle, valid, fv)
    yield A, B, host
    A.close(); B.close()


def _pairs(n_pairs):
    rng = np.random.default_rng(400 + n_pairs)
    a = rng.integers(0, 8, n_pairs); b = rng.integers(0, 8, n_pairs)
    if n_pairs >= 5:
        a[:3] = 2; b[1] = 7; b[2] = 6; a[4] = 7              # one slot in many pairs, an empty slot on either side, a pair without a common node
    return a.astype(np.int32), b.astype(np.int32)


@pytest.mark.parametrize("n_pairs", [1, 2, 5, 70])
@pytest.mark.parametrize("variant,ori", [(0, True), (0, False), (1, True), (1, False)])
def test_search_by_bow_batch_equals_the_single_calls_and_the_oracle(corb, pyorc, match_stores, variant, ori, n_pairs):
    A, B, host = match_stores
    sa, sb = _pairs(n_pairs)
    match, counts = A.SearchByBoW_batch(sa, B, sb, 0.75, ori, variant)
    lengths = []
    for p in range(n_pairs):
        m, n = A.SearchByBoW(int(sa[p]), B, int(sb[p]), 0.75, ori, variant)
        lengths.append(len(m))
        assert counts[p] == n and match[p, :len(m)].tobytes() == m.tobytes() and (match[p, len(m):] == -1).all(), p
        ha, hb = host.get(("A", int(sa[p]))), host.get(("B", int(sb[p])))
        if ha is None or hb is None:
            assert n == 0 and (match[p] == -1).all()
            continue
        r, rn = pyorc.search_by_bow(variant, ha[0], ha[1], ha[2], pyorc.FeatVec(*ha[3]), hb[0], hb[1], hb[2] if variant == 1 else np.ones_like(hb[2]), pyorc.FeatVec(*hb[3]), 0.75, ori)
        assert n == rn and np.array_equal(m, r), p
        if sb[p] == 6:
            assert n == 0
    assert match.shape[1] == max(lengths)
    if n_pairs >= 5:
        assert len(set(lengths)) > 2 and counts.max() >= 15                 # rows of different lengths under one stride, and pairs that do match
        with pytest.raises(corb.CorbError, match="match_stride"):
            A.SearchByBoW_batch(sa, B, sb, 0.75, ori, variant, stride=max(lengths) - 1)


# ---------------------------------------------------------------- (c) the chain ----------------------------------------------------------------
@pytest.fixture(scope="module")
def chain(corb, voc):
    c = FC.chain_case()
    glob, sub = FC.fill_stores(corb, c)
    yield c, glob, sub
    glob.close(); sub.close()


def _chain_db(corb, voc, c):
    db = corb.KeyFrameDatabase(voc, FC.N_GLOBAL + FC.N_SUB, 160)
    FC.apply_ops(db, c["ops"])
    return db


def _rows_array(corb, rows):
    """rows as an array of their six fields (the struct's padding is not compared)"""
    if isinstance(rows, np.ndarray):
        return np.stack([rows[f].astype(np.int64) for f in corb.FUSION_ROW_DTYPE.names], axis=1)
    return np.array(rows, np.int64).reshape(-1, 6)


def _earlier_route(corb, db, c, glob, sub, min_matches=15):
    """detect per query, SearchByBoW per pair, ids gathered on the host"""
    rows, ids, off = [], [], [0]
    for i, (qs, qe, qi) in enumerate(zip(c["query_slots"], c["query_entries"], c["query_ids"])):
        for e in db.detect(2, int(qe), int(qi)):
            slot = int(c["entry_slot"][e]); nm = 0; kept = False
            if slot >= 0:
                m, nm = glob.SearchByBoW(slot, sub, int(qs), 0.75, True, 0)
                kept = glob._n_any(slot) > 0 and not (int(glob.get_meta(slot)["flags"]) & corb.KF_BAD) and nm >= min_matches
            rows.append((i, int(e), slot, nm, int(kept), len(ids) if kept else -1))
            if kept:
                mp = glob.get_map_points(slot)
                ids += [int(mp[j]) if j >= 0 else corb.NO_MAP_POINT for j in m]
        off.append(len(rows))
    return rows, np.array(off, np.int32), np.array(ids, np.uint64)


def test_chain_equals_the_definition_and_the_earlier_route(corb, voc, chain):
    c, glob, sub = chain
    want_rows, want_off, want_ids, want_state = FC.chain_expected()
    db = _chain_db(corb, voc, c); twin = _chain_db(corb, voc, c)
    rows, off, ids = corb.map_fusion_candidates(db, sub, c["query_slots"], c["query_entries"], c["query_ids"], glob, c["entry_slot"])
    assert off.tolist() == want_off.tolist() and _rows_array(corb, rows).tobytes() == _rows_array(corb, want_rows).tobytes() and ids.tobytes() == want_ids.tobytes()
    assert _same_state(db.state(), want_state)
    e_rows, e_off, e_ids = _earlier_route(corb, twin, c, glob, sub)
    assert off.tobytes() == e_off.tobytes() and _rows_array(corb, rows).tobytes() == _rows_array(corb, e_rows).tobytes() and ids.tobytes() == e_ids.tobytes()
    assert db.state().tobytes() == twin.state().tobytes()
    assert rows["kept"].sum() >= 3 and (rows["slot"] < 0).any()
    # one query's slice of the ids goes straight to corb_pnp_ransac_store, and gives what the host-gathered rows give
    q = next(i for i in range(FC.N_SUB) if rows["kept"][off[i]:off[i + 1]].sum() >= 1)
    slot = int(c["query_slots"][q]); nq = sub._n_any(slot)
    kept = [r for r in rows[off[q]:off[q + 1]] if r["kept"]]
    a = ids[kept[0]["ids_offset"]: kept[0]["ids_offset"] + len(kept) * nq].reshape(len(kept), nq)
    b = np.stack([e_ids[r[5]: r[5] + nq] for r in e_rows[e_off[q]:e_off[q + 1]] if r[4]])
    MP, cam = FC.pnp_world(corb, c)
    rand = FC.pnp_draws()[: len(kept) * 300 * 4]
    ra = corb.PnPRansacStore(sub, slot, MP, cam, a, rand, min_inliers=10, epsilon=0.5); rb = corb.PnPRansacStore(sub, slot, MP, cam, b, rand, min_inliers=10, epsilon=0.5)
    assert len(ra) == len(rb) == len(kept) and ra[0]["n_corr"] == kept[0]["n_matches"]
    for x, y in zip(ra, rb):
        assert x["n_corr"] == y["n_corr"] and np.array_equal(x["index"], y["index"]) and x["counts"].tobytes() == y["counts"].tobytes() and x["records"].tobytes() == y["records"].tobytes()
    MP.close()
    # capacities: the rows first (after the detection alone), then the ids (with the rows complete); the sizes needed come back
    for caps, want in ((dict(cap_rows=3), (-5, len(want_rows), 0)), (dict(cap_ids=len(want_ids) - 1), (-5, len(want_rows), len(want_ids)))):
        d2 = _chain_db(corb, voc, c)
        with pytest.raises(corb.CorbError, match="room for"):
            corb.map_fusion_candidates(d2, sub, c["query_slots"], c["query_entries"], c["query_ids"], glob, c["entry_slot"], **caps)
        assert corb.map_fusion_candidates.last == want and _same_state(d2.state(), want_state)
        d2.close()
    before = db.state().tobytes()
    bad_slot = c["entry_slot"].copy(); bad_slot[0] = FC.N_GLOBAL
    for args, msg in (((c["query_slots"], c["query_entries"], c["query_ids"][::-1] * 0 + 1, c["entry_slot"]), "listed twice"),
                      ((c["query_slots"], c["query_entries"], c["query_ids"], bad_slot), "outside the global store")):
        with pytest.raises(corb.CorbError, match=msg):
            corb.map_fusion_candidates(db, sub, args[0], args[1], args[2], glob, args[3])
    assert db.state().tobytes() == before
    db.close(); twin.close()


# ---------------------------------------------------------------- (d) workspace ----------------------------------------------------------------
def _states(corb, run):
    """run() on a fresh arena, a warm one and one filled with either pattern: the bytes must be equal (the corb_scratch_fill rule of test_gpu_workspace_states.py)"""
    corb.release_scratch(0)
    outs = [run(), run()]
    size = max(corb.scratch_report(0)[0], 1 << 20)
    for word in (PATTERN_A, PATTERN_B):
        filled = corb.scratch_fill(0, word, size)
        outs.append(run())
        assert corb.scratch_report(0)[:2] == (filled, 1), "the call took memory outside the filled chunk"
        assert not (corb.scratch_read(0, 0, 1 << 20).view(np.uint32) == word).all(), "the call did not write into the filled chunk"
    for k, o in enumerate(outs[1:]):
        assert [x.tobytes() for x in o] == [x.tobytes() for x in outs[0]], ("fresh", "warm", "pattern A", "pattern B")[k + 1]
    corb.release_scratch(0)
    return outs[0]


def test_workspace_states_detect_batch(corb, voc, monkeypatch):
    monkeypatch.setenv("CORB_KFDB_BATCH_CHUNK", "50")
    entries, ids = FC.queries(70)

    def run():
        db = FC.build(corb, voc, 70)
        off, cand = db.detect_batch(2, entries, ids); st = db.state()
        db.close()
        return off, cand, st
    off, cand, st = _states(corb, run)
    assert cand.tolist() == FC.expected(70)[1].tolist() and _same_state(st, FC.expected(70)[3])


def test_workspace_states_search_by_bow_batch(corb, match_stores):
    A, B, _ = match_stores
    sa, sb = _pairs(70)
    for variant in (0, 1):
        match, counts = _states(corb, lambda: A.SearchByBoW_batch(sa, B, sb, 0.75, True, variant))
        assert counts.max() >= 15


def test_workspace_states_chain(corb, voc, chain):
    c, glob, sub = chain

    def run():
        db = _chain_db(corb, voc, c)
        rows, off, ids = corb.map_fusion_candidates(db, sub, c["query_slots"], c["query_entries"], c["query_ids"], glob, c["entry_slot"]); st = db.state()
        db.close()
        return _rows_array(corb, rows), off, ids, st
    rows, off, ids, st = _states(corb, run)
    assert ids.tobytes() == FC.chain_expected()[2].tobytes()


# ---------------------------------------------------------------- (e) the host mirror and the adapter ----------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_input(corb, c, best_first):
    """the chain case as tests/host/fusion_adapter_main.cpp reads it"""
    slot_entry = dict((int(s), e) for e, s in enumerate(c["entry_slot"][:FC.N_GLOBAL]) if s >= 0)
    rec = FC.pnp_records(corb, c, best_first); draws = FC.pnp_draws()
    blob = [struct.pack("<6i", FC.N_GLOBAL, FC.N_SUB, FC.CHAIN_F, 160, len(rec), len(draws))]
    nb = dict((op[1], op[2]) for op in c["ops"] if op[0] == "nb"); bow = dict((op[1], (op[2], op[3])) for op in c["ops"] if op[0] == "set_bow")
    keyframes = [(e, int(c["entry_slot"][e]), c["glob"].get(int(c["entry_slot"][e])), FC.STORE_IDS[0]) for e in range(FC.N_GLOBAL)] + \
                [(FC.N_GLOBAL + s, int(c["query_slots"][s]), c["sub"][int(c["query_slots"][s])], FC.STORE_IDS[1]) for s in range(FC.N_SUB)]
    for e, slot, x, first_id in keyframes:
        n = x["n"] if x is not None else 0
        kid = int(c["query_ids"][e - FC.N_GLOBAL]) if e >= FC.N_GLOBAL else first_id + max(slot, 0)
        blob.append(struct.pack("<iiiQ", slot, int(bool(x is not None and x["bad"])), n, kid))
        if slot >= 0 and n > 0:
            blob += [FC.keypoints(corb, x, first_id, slot).tobytes(), np.ascontiguousarray(x["desc"], np.uint8).tobytes(), x["mp_id"].astype("<u8").tobytes(),
                     struct.pack("<i", len(x["fv"][0])), x["fv"][0].astype("<u4").tobytes(), x["fv"][1].astype("<i4").tobytes(), x["fv"][2].astype("<u4").tobytes()]
        w, v = bow[e]
        blob += [struct.pack("<i", len(w)), w.astype("<u4").tobytes(), v.astype("<f8").tobytes(), np.asarray(nb.get(e, [-1] * 10), "<i4").tobytes()]
    blob += [np.array(FC.CAM, "<f4").tobytes(), rec.tobytes(), bytes(FC.camera(corb)), draws.astype("<i4").tobytes()]
    return b"".join(blob)


def _python_walk(corb, c, glob, sub, rows, off, ids, best_first):
    """detectKeyFrameInServerMap's loop (MapFusion.cpp:709-752) per keyframe in order through the Python harness: iterate(5) round-robin over the solvers that are not
    discarded; bNoMore discards a solver; ANY non-empty Tcw -- Refine()'s, or with bNoMore the running best -- ends the walk"""
    MP, cam = FC.pnp_world(corb, c, best_first)
    tried = 0; line = None
    for i in range(FC.N_SUB):
        kept = [r for r in range(off[i], off[i + 1]) if rows["kept"][r]]
        slot = int(c["query_slots"][i]); n = sub._n_any(slot)
        if not kept or n <= 0:
            continue
        a = ids[rows["ids_offset"][kept[0]]: rows["ids_offset"][kept[0]] + len(kept) * n].reshape(len(kept), n)
        out = corb.PnPRansacStore(sub, slot, MP, cam, a, FC.pnp_draws()[: len(kept) * 300 * 4], min_inliers=10, epsilon=0.5)
        tried += 1
        discarded = [False] * len(out); its = [0] * len(out)
        while not all(discarded) and line is None:
            for k, o in enumerate(out):
                if discarded[k]:
                    continue
                kind, b, its[k] = corb.pnp_replay(o["counts"], o["records"], o["ransac_min_inliers"], o["ransac_max_its"], its[k], 5)
                if kind != "refined":                           # bNoMore
                    discarded[k] = True
                if kind is not None:                            # !Tcw.empty()
                    rec = o["records"][b]; refined = kind == "refined"
                    line = "pose %d %d %d %d %s" % (i, kept[k], tried, int((o["refined_inliers"] if refined else o["best_inliers"])[b].sum()), kind) + \
                           "".join(" %08x" % int(x) for x in (rec["Tcw_refined"] if refined else rec["Tcw_best"]).view(np.uint32))
                    break
        if line:
            break
    MP.close()
    return line or "pose -1 -1 %d 0 none" % tried + " 00000000" * 12


@pytest.mark.parametrize("best_first", [False, True], ids=["refined", "best"])
def test_host_adapter_agrees_with_the_definition(corb, voc, chain, tmp_path, best_first):
    """corb::adapt::MapFusionDetectT and the mirror functions, compiled with -Wall -Werror on test doubles: the definition's text for the rows, offsets and ids, the
    batch form of DetectMapFusionCandidatesFromDB, and the walk -- a PnP call per keyframe in order, stopped at the first pose -- as the Python harness walks it"""
    c, glob, sub = chain
    exe = tmp_path / "fusion_adapter_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "corb-slam_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "fusion_adapter_main.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "corb-slam_amd"), "-lcorb_accel", "-Wl,-rpath," + os.path.join(ROOT, "corb-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    vtxt = tmp_path / "voc.txt"; vtxt.write_text(G.vocab(G.SESSION_VOCAB).to_text())
    (tmp_path / "in.bin").write_bytes(_host_input(corb, c, best_first))
    got = subprocess.check_output([str(exe), str(vtxt), str(tmp_path / "in.bin")]).decode().split("\n")[:-1]
    want_rows, want_off, want_ids, _ = FC.chain_expected()
    want = F.rows_text(want_rows, want_off, want_ids)
    assert got[:len(want)] == want
    assert got[len(want)] == "detect" + "".join(" %d" % d for d in np.diff(want_off))
    db = _chain_db(corb, voc, c)
    rows, off, ids = corb.map_fusion_candidates(db, sub, c["query_slots"], c["query_entries"], c["query_ids"], glob, c["entry_slot"])
    db.close()
    walk = _python_walk(corb, c, glob, sub, rows, off, ids, best_first)
    assert got[len(want) + 1] == walk, (got[len(want) + 1], walk)
    w = walk.split()
    if best_first:      # keyframe 0: a hypothesis with exactly mRansacMinInliers inliers is on record, its Refine() fails: bNoMore with mBestTcw ends the walk there
        n0 = int(rows["n_matches"][[r for r in range(off[0], off[1]) if rows["kept"][r]][0]])
        assert w[1:6] == ["0", str(off[0]), "1", str(n0 // 2), "best"], walk
    else:               # keyframe 0 finds no pose, keyframe POSE_QUERY a refined one
        assert w[1] == str(FC.POSE_QUERY) and w[3] == "2" and int(w[4]) >= 30 and w[5] == "refined", walk
    assert got[len(want) + 2] == "bow 1" and len(got) == len(want) + 3

"""GPU tests of include/corb_loop_detect.h: LoopClosing::DetectLoop on records, as one call and as a queue, against the definition (tests/loopdetect_reference.py) on
the worlds of tests/loopdetect_cases.py.  A keyframe store of 96 slots (two words per group, the second half-used), max_connections = 72, a hub row of 70
connections, keyframes of 60 and more features, BowVectors over the 1000 words of the small test vocabulary.  After every keyframe the outcome, the candidates as
entries and slots, the enough list, minScore's bits, the groups, the six fields of every entry and the live set equal the definition's.  What the definition's runs
contain is asserted on the CPU (tests/test_loopdetect_reference.py)."""
import functools

import numpy as np
import pytest

import bow_cases as B
import dbow_reference as DR
import loopdetect_cases as G
import loopdetect_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voc(corb):
    f = B.vocab(B.SESSION_VOCAB).flat()
    assert B.vocab(B.SESSION_VOCAB).n_words == G.N_VOCAB_WORDS
    v = corb.Vocabulary(f["k"], f["L"], f["parent"], f["is_leaf"], f["descriptor"], f["weight"])
    yield v
    v.close()


@pytest.fixture(scope="module")
def devs(corb, voc):
    """the worlds on the device, built once per module: stores and graph stay, database and detector are made per test (Dev.fresh)"""
    made = {}

    def get(key):
        if key not in made:
            made[key] = G.Dev(corb, voc, G.hand(key) if isinstance(key, str) else G.walk(key))
        return made[key]
    yield get
    for d in made.values():
        d.close()


def ref_state(w, bow):
    """the six fields of every database entry as the definition holds them, in entry order"""
    rows = [(0, 0, np.float32(0), 0, 0, np.float32(0))] * w.n_entries
    for kid, e in w.entry.items():
        rows[e] = bow[kid].state()
    return B.state_array(rows)


def same_answer(dev, got, want):
    """a device answer (LoopDetector.detect) against the definition's"""
    w = dev.w
    assert got["outcome"] == want["outcome"], (got, want)
    assert [dev.id_of_entry[e] for e in got["cand_entries"]] == want["candidates"] and got["cand_slots"] == [w.slot[k] for k in want["candidates"]], (got, want)
    assert got["enough"] == want["enough"] and got["n_groups"] == len(want["groups"]), (got, want)
    bits = 0 if want["minScore"] is None else int(np.float32(want["minScore"]).view(np.uint32))
    assert got["min_score_bits"] == bits, (hex(got["min_score_bits"]), hex(bits))


def host_live(dev, db=None):
    """the database's live set as its host side knows it: set_bow refuses an entry that is in the database, before anything changes.  An entry that is not takes the
    same BowVector again; its six fields are zero in these worlds (nothing is erased), so nothing changes either"""
    live = set()
    for kid, e in dev.w.entry.items():
        try:
            (db or dev.db).set_bow(e, *dev.w.words[kid])
        except dev.corb.CorbError as err:
            assert "erase it first" in str(err)
            live.add(kid)
    return live


def device_live(dev, db=None):
    """the live flags on the device, LAST in a test (it moves the relocalisation fields): a relocalisation query that holds every word of the world marks exactly the
    entries in the inverted file"""
    db = db or dev.db; w = dev.w
    probe = next(e for e in range(w.n_entries) if e not in dev.id_of_entry)
    words = np.unique(np.concatenate([w.words[k][0] for k in w.entry]))
    db.set_bow(probe, words, np.full(len(words), 1.0 / len(words)))
    db.detect(1, probe, 4242)
    st = db.state()
    return set(k for k, e in w.entry.items() if st["reloc_query"][e] == 4242)


def same_world(dev, lc, bow, det=None, db=None):
    assert dev.groups(det) == lc.groups()
    assert (db or dev.db).state().tobytes() == ref_state(dev.w, bow).tobytes()


def play(dev, script, lc, bow, det=None, check_live=False):
    """a script on the device and the definition side by side; [(op, device answer)]"""
    det = det or dev.det; w = dev.w; out = []
    for op in script:
        got = None
        if op[0] == "detect":
            got = det.detect(w.slot[op[1]])
            same_answer(dev, got, lc.DetectLoop(op[1]))
        elif op[0] == "last":
            det.set_last_loop(op[1]); lc.mLastLoopKFid = op[1]
            assert det.get_last_loop() == op[1]
        elif op[0] == "reset":
            det.reset(); lc.RequestReset()
            assert det.get_last_loop() == 0
        elif op[0] == "clear":
            det.clear_groups(); lc.mvConsistentGroups = []
        elif op[0] == "drop":
            det.drop_slot(w.slot[op[1]]); lc.drop(op[1])
        same_world(dev, lc, bow, det)
        if check_live:
            assert host_live(dev) == lc.live
        out.append((op, got))
    return out


# ---------------------------------------------------------------- 1. the hand-built worlds ----------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in G.HAND if n != "unbound_covisible"])
def test_hand_built_world(devs, name):
    dev = devs(name); dev.fresh()
    lc, _, bow = dev.w.reference()
    out = play(dev, dev.w.script, lc, bow, check_live=True)
    assert [a["outcome"] for _, a in out if a] == [a["outcome"] for _, a in G.run(dev.w) if a]
    assert device_live(dev) == lc.live
    if name == "hub":
        assert [len(g) for g, _ in dev.det.get_groups()] == [2]
    if name == "all_connected_bad":
        assert out[0][1]["min_score_bits"] == 0x3F800000


# ---------------------------------------------------------------- 2. the seeded walks ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(seed):
    """the definition's run of a walk, once: per script step (op, answer, groups, states, live)"""
    w = G.walk(seed); lc, _, bow = w.reference()
    steps = []
    G.run(w, lc, lambda op, ans, lc: steps.append((op, ans, lc.groups(), ref_state(w, bow).tobytes(), set(lc.live))))
    return steps


class HostRoute:
    """DetectLoop by the five calls a host walks today -- corb_covis_query, corb_kfdb_score with the minimum on the host, corb_kfdb_detect(kind 0) with the connected
    set uploaded, one corb_covis_get per candidate, corb_kfdb_add -- and the group logic in Python (the definition's closed form)"""

    def __init__(self, dev, db):
        self.dev = dev; self.db = db; self.last = 0; self.groups = []

    def detect(self, kid):
        dev = self.dev; w = dev.w; e = w.entry[kid]; slot = w.slot[kid]
        if kid < self.last + 10:
            self.db.add(e)
            return R.GAP
        cov = [int(s) for s in dev.g.query(slot)[0] if not int(dev.KF.get_meta(int(s))["flags"]) & 1]
        ms = np.float32(1)
        for s in self.db.score(e, [w.entry[dev.id_of_slot[s]] for s in cov]):
            if np.float32(s) < ms:
                ms = np.float32(s)
        held = lambda ids: [int(i) for i in ids if int(i) in w.slot]
        conn = [w.entry[i] for i in held(dev.g.get(slot)[0][0]) if i in w.entry]
        cands = [dev.id_of_entry[int(c)] for c in self.db.detect(0, e, kid, conn, float(ms))]
        if not cands:
            self.db.add(e); self.groups = []
            return R.NONE
        cg = [set(held(dev.g.get(w.slot[c])[0][0])) | {c} for c in cands]
        self.groups, enough = R.closed_form(cg, self.groups)
        self.db.add(e)
        return R.DETECTED if enough else R.NOT_ENOUGH


@pytest.mark.parametrize("seed", G.WALK_SEEDS)
def test_seeded_walk_follows_the_definition_and_the_host_route_leaves_the_same_bytes(devs, seed):
    dev = devs(seed); det = dev.fresh(); w = dev.w
    db2 = dev.new_db(); host = HostRoute(dev, db2)
    for op, ans, groups, states, live in expected(seed):
        if op[0] == "detect":
            got = det.detect(w.slot[op[1]])
            same_answer(dev, got, ans)
            assert host.detect(op[1]) == ans["outcome"]
        else:
            det.set_last_loop(op[1]); host.last = op[1]
        assert dev.groups() == groups == [(sorted(s), c) for s, c in host.groups]
        assert dev.db.state().tobytes() == states == db2.state().tobytes()
    assert host_live(dev) == live == host_live(dev, db2)
    # 6. existing behaviour: on the database the detector worked on, corb_kfdb_score and corb_kfdb_detect(kind 0) still give the definition's bytes
    lc, _, bow = w.reference(); G.run(w, lc)
    kids = sorted(w.entry)
    for q in (w.cur_ids[-1], w.cur_ids[3], 7):
        got = dev.db.score(w.entry[q], [w.entry[k] for k in kids])
        want = np.array([DR.score(bow[q].bow, bow[k].bow) for k in kids], np.float64)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        conn = kids[5:9]
        bow[q].mnId = 5000 + q; bow[q].connected = set(bow[k] for k in conn)
        want_c = [o.name for o in lc.mpKeyFrameDB.DetectLoopCandidates(bow[q], np.float32(0.02))]
        got_c = [dev.id_of_entry[int(c)] for c in dev.db.detect(0, w.entry[q], 5000 + q, [w.entry[k] for k in conn], float(np.float32(0.02)))]
        assert got_c == want_c and dev.db.state().tobytes() == ref_state(w, bow).tobytes()
    assert device_live(dev) == live
    db2.close()


# ---------------------------------------------------------------- 3. the queue ----------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 3, 8])
@pytest.mark.parametrize("seed", G.WALK_SEEDS)
def test_queue_matches_the_single_calls_and_stops_at_the_first_detection(devs, seed, chunk):
    dev = devs(seed); det = dev.fresh(); w = dev.w
    steps = [s for s in expected(seed) if s[0][0] == "detect"]
    pending = list(w.cur_ids); k = 0; stopped_early = 0
    while pending:
        ids = pending[:chunk]
        got = det.detect_queue([w.slot[i] for i in ids])
        assert 1 <= len(got) <= len(ids)
        for a in got:
            same_answer(dev, a, steps[k][1]); k += 1
        assert all(a["outcome"] != R.DETECTED for a in got[:-1])
        assert len(got) == len(ids) or got[-1]["outcome"] == R.DETECTED          # it stops only at a detection
        _, _, groups, states, live = steps[k - 1]
        assert dev.groups() == groups and dev.db.state().tobytes() == states      # the keyframes behind the stopping one left no trace
        if len(got) < len(ids):
            stopped_early += 1
            assert not (host_live(dev) & set(ids[len(got):]))
        if got[-1]["outcome"] == R.DETECTED:
            det.set_last_loop(ids[len(got) - 1])                                  # CorrectLoop (:591), then the queue goes on
        pending = pending[len(got):]
    assert k == 40 and (chunk == 1 or stopped_early >= 1)
    assert host_live(dev) == steps[-1][4] and device_live(dev) == steps[-1][4]


def test_queue_argument_errors_are_found_before_anything_runs(devs, corb):
    dev = devs("sequence"); det = dev.fresh(); w = dev.w
    before = dev.db.state().tobytes()
    for bad, msg in (([w.slot[100], w.slot[100]], "listed twice"), ([w.slot[100], G.N_SLOTS], "slot 96 of 96"), ([w.slot[100], w.slot[2]], "in the database already"),
                     (list(range(65)), "bad argument")):
        with pytest.raises(corb.CorbError, match=msg):
            det.detect_queue(bad)
    assert det.detect_queue([]) == [] and dev.db.state().tobytes() == before and dev.groups() == [] and host_live(dev) == set(w.old_ids)


# ---------------------------------------------------------------- 4. drop_slot (also the "drop" world above) ----------------------------------------------------------------
def test_drop_slot_clears_the_bit_and_the_candidate_is_no_longer_consistent(devs):
    dev = devs("two_candidates_one_group"); det = dev.fresh(); w = dev.w
    lc, _, bow = w.reference()
    play(dev, [("detect", 100), ("detect", 101), ("detect", 102)], lc, bow)
    assert dev.groups() == [([1, 2, 3, 4], 2)]
    # candidate 3 = {2, 3} shares only 2 and 3 with the stored group, candidate 1 = {1, 2} only 1 and 2: without 2 and 3 the former is no longer consistent
    play(dev, [("drop", 2), ("drop", 3)], lc, bow)
    assert dev.groups() == [([1, 4], 2)]
    got = det.detect(w.slot[103])
    same_answer(dev, got, lc.DetectLoop(103))
    assert got["enough"] == [0] and dev.groups() == [([1, 2], 3), ([2, 3], 0)] == lc.groups()


# ---------------------------------------------------------------- 5. errors ----------------------------------------------------------------
def snapshot(dev):
    return dev.groups(), dev.db.state().tobytes(), host_live(dev), dev.det.get_last_loop()


def test_argument_errors_change_nothing(devs, corb):
    dev = devs("unbound_covisible"); det = dev.fresh(); w = dev.w
    lc, _, bow = w.reference()
    before = snapshot(dev)
    with pytest.raises(corb.CorbError, match=r"\(-1\).*covisible keyframe of slot %d has no bound database entry" % w.slot[101]):
        det.detect(w.slot[101])                                                  # 100 is covisible with 101 and has no entry
    with pytest.raises(corb.CorbError, match=r"\(-1\).*no bound database entry"):
        det.detect(w.slot[100])                                                  # the keyframe itself is unbound
    empty = next(s for s in range(G.N_SLOTS) if s not in dev.id_of_slot)
    with pytest.raises(corb.CorbError, match=r"\(-1\).*slot %d is empty" % empty):
        det.detect(empty)
    dev.KF.put(empty, np.zeros(0, corb.KP_DTYPE), np.zeros((0, 32), np.uint8), keyframe_id=555)
    with pytest.raises(corb.CorbError, match=r"\(-1\).*holds no feature"):
        det.detect(empty)
    for s in (-1, G.N_SLOTS):
        with pytest.raises(corb.CorbError, match=r"\(-1\).*slot %d of 96" % s):
            det.detect(s)
    with pytest.raises(corb.CorbError, match=r"\(-1\)"):
        det.bind([0, 0], [1, 2])
    with pytest.raises(corb.CorbError, match=r"\(-1\)"):
        det.bind([0], [w.n_entries])
    with pytest.raises(corb.CorbError, match=r"\(-1\)"):
        det.drop_slot(G.N_SLOTS)
    assert snapshot(dev) == before
    assert G.run(w, lc) == [(("detect", 101), "unbound")] and device_live(dev) == lc.live


def test_capacity_errors_leave_groups_and_live_set(devs, corb):
    dev = devs("two_candidates_one_group"); det = dev.fresh(max_candidates=1); w = dev.w
    lc, _, bow = w.reference()
    play(dev, [("detect", 100), ("detect", 101), ("detect", 102)], lc, bow)
    groups, live = dev.groups(), host_live(dev)
    with pytest.raises(corb.CorbError, match=r"\(-2\).*has 2 candidates, max_candidates = 1"):
        det.detect(w.slot[103])
    assert det.last_result["n_candidates"] == 2 and dev.groups() == groups == [([1, 2, 3, 4], 2)] and host_live(dev) == live and 103 not in live
    assert device_live(dev) == live

    dev = devs("one_candidate_two_groups"); det = dev.fresh(max_groups=1); w = dev.w
    lc, _, bow = w.reference()
    play(dev, [("detect", 100)], lc, bow)
    with pytest.raises(corb.CorbError, match=r"\(-2\).*more than max_groups = 1"):
        det.detect_queue([w.slot[101], w.slot[102]])                             # in the queue form the error ends the queue at that keyframe
    assert det.last_answers == [] and dev.groups() == [([1, 2], 0)] and host_live(dev) == set(w.old_ids) | {100}
    assert device_live(dev) == set(w.old_ids) | {100}

"""CPU tests of the definition of whole-submap detection (tests/fusion_reference.py): its batch, computed stage by stage the way the device computes it, equals its own
one-by-one session through dbow_reference's text of KeyFrameDatabase.cc; and the conditions the generators of tests/fusion_cases.py are kept for hold on the
definition's side, before any device is consulted."""
import numpy as np
import pytest
import fusion_cases as C
import fusion_reference as F


@pytest.mark.parametrize("n", [1, 2, 70, 300])
def test_batch_equals_one_by_one(n):
    off, cand, ev, state = C.expected(n)
    db = C.database(n)[0].copy()
    lists = F.one_by_one(db, *C.queries(n))
    assert [len(l) for l in lists] == np.diff(off).tolist() and [e for l in lists for e in l] == cand.tolist()
    assert db.state.tobytes() == state.tobytes()


def test_batch_equals_one_by_one_on_wide_vectors_and_across_calls():
    off, cand, ev, state = C.wide_expected()
    db = C.wide_database()[0].copy()
    lists = F.one_by_one(db, *C.wide_queries())
    assert [e for l in lists for e in l] == cand.tolist() and db.state.tobytes() == state.tobytes()
    assert min(len(b[0]) for b in db.bow) > 64 and ev["candidates"] >= len(lists)       # every list beyond one ballot round, and matched
    # a second call whose first id is the one the first call's last query left in the entries it met: those visits add to the count and push nothing
    a = C.database(70)[0].copy(); b = a.copy()
    e, i = C.queries(70)
    F.detect_batch(a, e, i); F.one_by_one(b, e, i)
    e2, i2 = C.repeat_queries(a.state)
    assert (a.state["reloc_query"] == i2[0]).sum() >= 2
    o2, c2, _ = F.detect_batch(a, e2, i2); l2 = F.one_by_one(b, e2, i2)
    assert [x for l in l2 for x in l] == c2.tolist() and a.state.tobytes() == b.state.tobytes()


def test_the_generators_meet_their_conditions():
    """not measurements: the definition alone meets these with the project's generator and this query order"""
    table = {70: (140, 150, 507, 70), 300: (600, 637, 2705, 288), 2: (4, 4, 5, 0)}      # entries: queries, candidates, non-zero stale additions, stale neighbour becomes best
    for n, want in table.items():
        ev = C.expected(n, with_random=False)[2]
        assert (ev["queries"], ev["candidates"], ev["stale_additions"], ev["stale_best"]) == want, (n, ev)
    ev = C.expected(70)[2]
    assert ev["stale_additions"] >= 100 and ev["stale_best_queries"] >= 10 and ev["none"] >= 1 and ev["three"] >= 1, ev


def test_the_chain_case_discards_for_every_reason():
    c = C.chain_case()
    rows, off, ids, state = C.chain_expected()
    kept_queries = set(r[0] for r in rows if r[4])
    assert len(kept_queries) >= 3
    dropped = [r for r in rows if not r[4]]
    assert any(r[2] < 0 for r in dropped), "no row without a record"
    assert any(r[2] >= 0 and c["glob"][r[2]]["bad"] and r[3] >= 15 for r in dropped), "no row of a bad keyframe that would have been kept"
    assert any(r[2] >= 0 and not c["glob"][r[2]]["bad"] and r[3] < 15 for r in dropped), "no row with fewer than min_matches"
    for r in rows:                                          # the kept rows' ids are consecutive, each n(query slot) long
        if r[4]:
            n = c["sub"][int(c["query_slots"][r[0]])]["n"]
            assert r[5] + n <= len(ids) and (ids[r[5]:r[5] + n] != F.NO_MAP_POINT).sum() == r[3]
    assert len(ids) == sum(c["sub"][int(c["query_slots"][r[0]])]["n"] for r in rows if r[4])


def test_the_switches_of_the_new_sources_are_run_by_the_gpu_tests():
    """corb_fusion.cpp reads its development switch through call_switch(), at every call: every name it passes is set by tests/test_gpu_fusion.py, and the new
    sources read no other switch"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = set()
    for f in ("corb_fusion.cpp", "fusion_kernels.hip", "fusion_internal.h", "bow_device.h", "match_device.h"):
        src = open(os.path.join(root, "corb-slam_amd", "csrc", f)).read()
        names |= set(re.findall(r'call_switch\s*\(\s*"([^"]+)"', src))
        assert not re.findall(r'\bgetenv\s*\(\s*"', src), f
    assert names == {"CORB_KFDB_BATCH_CHUNK"}
    gpu = open(os.path.join(root, "tests", "test_gpu_fusion.py")).read()
    assert all('monkeypatch.setenv("%s"' % n in gpu for n in names)

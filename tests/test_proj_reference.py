"""The Python restatement of the projection matchers (tests/proj_reference.py) against the CPU oracle on every case of tests/proj_cases.py and on the seeded scenes
the older GPU tests use, and the kinds of decision those inputs reach.  No GPU.

1. Per input the restatement's match array, count and (initialisation) prev_matched bit pattern equal pyorc's: this is what makes the kind counts trustworthy.
2. Per case every kind that proj_cases.SUPPLIES says the case is there for is counted > 0 on the oracle's data: a failure names the input to repair.
3. Summed over the cases every required kind is > 0 and every unreachable kind (proj_reference.UNREACHABLE, with the reasons) is 0.
4. The facts the cases lean on, asserted on the oracle's own output: which feature wins a tie, 100 / 101, the ratio equalities, u_right == 0, the window edge,
   roundf on the half, 1 of 10 and 1 of 11 in ComputeThreeMaxima."""
import numpy as np
import pytest

import proj_cases as PC
import proj_reference as R


def same(a, b):
    return PC.as_bytes(a) == PC.as_bytes(b)


@pytest.mark.parametrize("case", PC.CASES)
def test_restatement_equals_oracle(pyorc, case):
    o = PC.oracle(pyorc, case); r = PC.restated(case)
    res, notes = r[:-2], r[-1]
    if not same(o, res):
        bad = np.nonzero(o[0] != res[0])[0]
        raise AssertionError("%s: the restatement differs from the oracle at %s (oracle %s, restated %s; counts %d / %d)" %
                             (PC.describe(case), bad[:8].tolist(), o[0][bad[:8]].tolist(), res[0][bad[:8]].tolist(), o[-1], res[-1]))
    c = PC.build(case)
    assert len(notes) == len(c["mps"] if c["kind"] == "map" else c["last"] if c["kind"] == "frame" else c["pm"])


@pytest.mark.parametrize("case", PC.CASES)
def test_case_supplies_its_kinds(pyorc, case):
    kinds = PC.restated(case)[-2]
    print(case, {k: v for k, v in kinds.items() if v})
    for k in PC.SUPPLIES[case]:
        assert kinds[k] > 0, "%s: the oracle's data no longer shows kind '%s'" % (PC.describe(case), k)
    for k in R.UNREACHABLE:
        assert kinds[k] == 0, "%s reaches '%s', argued unreachable: %s" % (PC.describe(case), k, R.UNREACHABLE[k])
    c = PC.build(case)
    assert (kinds["cand_over"] > 0) == bool(c["overflow"]), PC.describe(case)


def test_every_kind_is_reached(pyorc):
    named = set(k for c in PC.CASES for k in PC.SUPPLIES[c])
    assert named >= set(R.REQUIRED), "the case table names no supplier for %s" % sorted(set(R.REQUIRED) - named)
    total = {k: 0 for k in R.ALL_KINDS}
    for case in PC.CASES:
        for k, v in PC.restated(case)[-2].items():
            total[k] += v
    print(total)
    for k in R.REQUIRED:
        assert total[k] > 0, "no case reaches kind '%s'" % k
    for k in R.UNREACHABLE:
        assert total[k] == 0, k


def test_cases_are_deterministic():
    for case in PC.CASES:
        a, b = PC.BUILDERS[case](), PC.BUILDERS[case]()
        assert a.keys() == b.keys()
        for k in a:
            for x, y in zip(*(([v[f] for f in sorted(v)] if isinstance(v, dict) else [v]) for v in (a[k], b[k]))):
                assert (x.tobytes() == y.tobytes()) if isinstance(x, np.ndarray) else x == y, (case, k)


SCENES = [("map", dict(n=300)), ("map", dict(n=300, dense=True)), ("frame", dict(n=300)), ("frame", dict(n=300, dense=True)), ("init", dict(n=300))]


@pytest.mark.parametrize("kind,args", SCENES)
def test_restatement_equals_oracle_on_seeded_scenes(pyorc, synth, kind, args):
    if kind == "init":
        f1, f2, pm, _ = synth.monocular_init_pair(**args)
        cases = [dict(kind="init", f1=f1, f2=f2, pm=pm, win=w, ratio=r, ori=o) for w, r, o in ((100, 0.9, 1), (40, 0.8, 0))]
    else:
        s = synth.tracking_scene(**args)
        if kind == "map":
            cases = [dict(kind="map", frame=s["cur"], mps=s["mps"], desc=s["last_desc"], th=th, nnratio=r) for th, r in ((1.0, 0.8), (3.0, 0.8), (5.0, 0.9))]
        else:
            cases = [dict(kind="frame", cur=s["cur"], Tcw=s["Tcw"], Tlw=s["Tlw"], fx=s["fx"], fy=s["fy"], cx=s["cx"], cy=s["cy"], bf=s["bf"], mb=s["mb"], last=s["last"],
                          desc=s["last_desc"], th=th, mono=m, ori=o) for m, th, o in ((0, 7.0, 1), (1, 15.0, 1), (0, 15.0, 0))]
    for c in cases:
        o = PC.oracle_call(pyorc, c); r = PC.restate_call(c)
        assert same(o, r[:-2]), (kind, args, {k: v for k, v in c.items() if not hasattr(v, "__len__")})
        assert o[-1] > 0
        for k in R.UNREACHABLE:
            assert r[-2][k] == 0, k


def _matched_to(result, query):
    return np.nonzero(result[0] == query)[0].tolist()


def test_facts_on_the_oracle(pyorc):
    """the facts the issue states as checked, read from the oracle's own output (query and feature numbers follow the builders of proj_cases.py)"""
    o = PC.oracle(pyorc, "map_grid"); c = PC.build("map_grid")
    assert _matched_to(o, 0) == [1], "x = 1232 is out of the grid, x = 1230 is in"
    assert _matched_to(o, 8) == [6] and _matched_to(o, 9) == [8], "|dx| == r and |dy| == r are excluded, 3.75 is in"
    ur = c["frame"]["u_right"]
    q = {float(x): i for i, x in enumerate(c["mps"]["proj_x"])}
    assert ur[_matched_to(o, q[100.0])[0]] == -1.0, "u_right just above r is rejected"
    assert ur[_matched_to(o, q[200.0])[0]] == 94.0, "u_right at |err| == r is accepted"
    assert [ur[f] for f in _matched_to(o, q[300.0]) if c["frame"]["keys_un"]["y"][f] == 50] == [0.0], "u_right == 0 is not a stereo value"
    # ties: the winner has the higher feature index across columns and rows, the lower inside a cell
    o = PC.oracle(pyorc, "map_ties")
    assert _matched_to(o, 0) == [1] and _matched_to(o, 1) == [3] and _matched_to(o, 2) == [4]
    assert _matched_to(o, 3) == [6] and _matched_to(o, 4) == [], "100 is accepted, 101 rejected"
    o = PC.oracle(pyorc, "map_ratio")
    assert _matched_to(o, 0) == [0] and _matched_to(o, 1) == [] and _matched_to(o, 2) == [4], "40 / 80 accepted, 41 / 80 rejected at one level, accepted across levels"
    o = PC.oracle(pyorc, "frame_chain")
    assert _matched_to(o, 0) == [1] and _matched_to(o, 1) == [3] and _matched_to(o, 2) == [4]
    for case in ("map_lists", "frame_lists"):
        assert np.all(PC.oracle(pyorc, case)[0][:90] >= 0), "the lists of 12, 13 and 65 are emptied: whichever feature sits at list position 12 is matched"
    for case, first in (("map_deep", 0), ("frame_chain", 27)):
        assert np.all(PC.oracle(pyorc, case)[0][first:first + 20] >= 0), "the 20 features of the queries in [1024, 2048) are all matched"
    # the rotation pass
    o = PC.oracle(pyorc, "frame_rot"); notes = PC.restated("frame_rot")[-1]
    assert o[1] == 19 and "bin 1," in notes[19] and "bin 12," in notes[20] and _matched_to(o, 19) == [] and _matched_to(o, 20) == [], "rot = 15 is bin 1, rot = -10 bin 12"
    assert R.roundf(np.float32(15.0) * (np.float32(1.0) / np.float32(30))) == 1.0 and np.round(np.float32(0.5)) == 0.0 and np.float32(0.1) * np.float32(10) == np.float32(1.0)
    assert PC.oracle(pyorc, "frame_hist_tenth")[1] == 11 and PC.oracle(pyorc, "frame_hist_eleventh")[1] == 11, "1 of 10 is kept, 1 of 11 dropped"
    o = PC.oracle(pyorc, "frame_hist_max3")
    assert o[1] == 26 and _matched_to(o, 26) == [] and _matched_to(o, 27) == [], "the overwritten query's entry removes the later query's match: 28 matched, 2 subtracted"
    # initialisation
    o = PC.oracle(pyorc, "init_basic")
    assert o[0][:5].tolist() == [0, -1, -1, 4, -1], "50 accepted, 51 rejected, 40 / 80 at 0.5 rejected, 39 accepted, equal best and second rejected"
    assert o[0][5] == -1 and o[0][6] == 10 and o[0][9:13].tolist() == [11, 12, -1, 13], "levels; <= at equality; a steal resets the earlier partner"
    o = PC.oracle(pyorc, "init_rot")
    assert o[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, -1, 8, -1, -1, 10] and o[2] == 10, "the lost partner's entry makes bin 1 hold 11: the bin-4 match is removed"

"""The numpy restatement of Frame::ComputeStereoMatches (tests/stereo_reference.py) against the CPU oracle on every case of tests/stereo_cases.py, and the kinds
of decision those cases reach.  No GPU.

1. Per case the restatement's u_right and depth bit patterns and n_matched equal pyorc.stereo_match's: this is what makes the kind counts trustworthy.
2. Per case every kind that stereo_cases.SUPPLIES says the case is there for is counted > 0 on the oracle's data: a failure names the input to repair.
3. Summed over the cases every required kind is > 0 and every unreachable kind (stereo_reference.UNREACHABLE, with the arguments) is 0.
No case is skipped or filtered: a kind that the oracle stops producing fails the test."""
import numpy as np
import pytest

import stereo_cases as SC
import stereo_reference as R


@pytest.mark.parametrize("case", SC.CASES)
def test_restatement_equals_oracle(pyorc, synth, case):
    o = SC.oracle(pyorc, synth, case)
    ur, dp, nm, kinds, decision = SC.restated(pyorc, synth, case)
    what = SC.describe(case)
    bad = np.nonzero((ur.view(np.uint32) != o["u_right"].view(np.uint32)) | (dp.view(np.uint32) != o["depth"].view(np.uint32)))[0]
    assert len(bad) == 0, "%s: the restatement differs from the oracle at left keypoints %s (restated decisions %s)" % (what, bad[:8].tolist(), [decision[i] for i in bad[:8]])
    assert nm == o["n_matched"], what
    # the decisions account for every left keypoint, and the outputs agree with them
    assert len(decision) == len(o["kl"]) and set(decision) <= set(R.DECISIONS)
    kept = np.array([d in ("kept", "clamp_kept") for d in decision], bool)
    assert np.array_equal(kept, ur >= 0) and np.array_equal(kept, dp > 0) and int(kept.sum()) == nm, what
    assert np.all(ur[~kept].view(np.uint32) == np.float32(-1).view(np.uint32)) and np.all(dp[~kept].view(np.uint32) == np.float32(-1).view(np.uint32)), what


@pytest.mark.parametrize("case", SC.CASES)
def test_case_supplies_its_kinds(pyorc, synth, case):
    kinds = SC.restated(pyorc, synth, case)[3]
    print(case, {k: v for k, v in kinds.items() if v})
    for k in SC.SUPPLIES[case][1]:
        assert kinds[k] > 0, "%s: the oracle's data no longer shows kind '%s'" % (SC.describe(case), k)
    for k in R.UNREACHABLE:
        assert kinds[k] == 0, "%s reaches '%s', which the front-end was argued not to reach: keep the input and move the kind to the required list" % (SC.describe(case), k)


def test_every_kind_is_reached(pyorc, synth):
    assert set(k for c in SC.CASES for k in SC.SUPPLIES[c][1]) >= set(R.REQUIRED), "the case table names no supplier for %s" % sorted(set(R.REQUIRED) - set(k for c in SC.CASES for k in SC.SUPPLIES[c][1]))
    total = {k: 0 for k in R.REQUIRED + R.UNREACHABLE}
    for case in SC.CASES:
        for k, v in SC.restated(pyorc, synth, case)[3].items():
            total[k] += v
    print(total)
    for k in R.REQUIRED:
        assert total[k] > 0, "no case reaches kind '%s'" % k
    for k in R.UNREACHABLE:
        assert total[k] == 0, k


def test_clamp_survives(pyorc, synth):
    """the zero-disparity clamp: at least one clamped match survives the median filter, with uR = float(double(uL) - 0.01) and depth = bf / 0.01f in the oracle's output"""
    case = "partial"
    o = SC.oracle(pyorc, synth, case); decision = SC.restated(pyorc, synth, case)[4]
    idx = [i for i, d in enumerate(decision) if d == "clamp_kept"]
    assert len(idx) >= 1, SC.describe(case)
    bf = np.float32(SC.CONFIGS[SC.SUPPLIES[case][0]][2])
    for i in idx:
        uL = o["kl"]["x"][i]
        assert o["u_right"][i] == np.float32(float(uL) - 0.01) and o["depth"][i] == bf / np.float32(0.01)
        assert o["u_right"][i] < uL


def test_geometries(pyorc, synth):
    """what the two further geometries are there for: 8 levels whose top level still has >= 62 px per axis, odd sizes (a level-0 row pitch that differs from the
    width), keypoints on every level (all branches of the device's level select); 2 levels"""
    o = SC.oracle(pyorc, synth, "deep_plain")
    w, h, _, _, nl, _, _ = SC.GEOMETRIES["deep"]
    assert nl == 8 and w % 2 == 1 and h % 2 == 1 and w % 4 != 0 and min(o["levels_l"][-1].shape) >= 62
    matched_levels = set(int(x) for x in o["kl"]["octave"][o["u_right"] >= 0])
    assert set(int(x) for x in o["kl"]["octave"]) == set(range(8)) and matched_levels == set(range(8)), matched_levels
    o2 = SC.oracle(pyorc, synth, "flat2_plain")
    assert len(o2["levels_l"]) == 2 and set(int(x) for x in o2["kl"]["octave"][o2["u_right"] >= 0]) == {0, 1}

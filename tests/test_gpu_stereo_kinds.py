"""stereo_rows_kernel, stereo_match_kernel, stereo_filter_kernel and stereo_pack_kernel by kind of decision (pytest -m gpu): every case of tests/stereo_cases.py
through the stereo front-end, keypoints, descriptors, mvuRight and mvDepth as bit patterns and the match count against the CPU oracle.  All comparisons are exact.

Which decisions of Frame::ComputeStereoMatches the cases reach is counted on the ORACLE's data by the numpy restatement (tests/stereo_reference.py lists the
kinds and the decisions no input can reach; tests/test_stereo_reference.py asserts the restatement equal to the oracle, every kind present and which case
supplies which).  Here the case table must name a supplier among the cases this module runs for every required kind, so dropping a case cannot pass quietly; a
mismatch is reported with the case, the kinds it is there for and the restatement's decision for the keypoints that differ.

Routes: one batch per configuration (one handle per (geometry, fx, bf): 320 x 120 with 4 levels at three intrinsics, 701 x 231 with 8 levels -- odd sizes, a
level-0 pitch that differs from the width, every branch of the level select -- and 152 x 74 with 2 levels); the base cases through the per-frame call at n = 1,
2 and 3 with every case in every result block, a sparse frame after a dense one and a frame whose matches are all rejected after one with matches; the same
batch twice; the slots in reverse order."""
import numpy as np
import pytest

import stereo_cases as SC
import stereo_reference as R

pytestmark = pytest.mark.gpu

FIELDS = ("kl", "dl", "kr", "dr", "u_right", "depth")
# the per-frame route's order (cyclic): two_rects, lt4, flat_right, flat_flat, flat_left and rect7 are sparse frames behind dense ones; "same" (median 0: all of
# its matches rejected) and noise_roll5 / binary_roll4 (the same) follow frames that keep matches
FRAME_ORDER = ["plain", "two_rects", "partial", "same", "tile16", "lt4", "alt_rows", "flat_right", "half_contrast", "noise_roll5", "flat_flat", "swapped",
               "binary_roll4", "flat_left", "right_flat_below", "rect7"]


def frontend(corb, config, max_frames):
    geo, fx, bf = SC.CONFIGS[config]
    w, h, nf, sf, nl, ini, mn = SC.GEOMETRIES[geo]
    return corb.StereoFrontend(nfeatures=nf, scaleFactor=sf, nlevels=nl, iniThFAST=ini, minThFAST=mn, width=w, height=h, max_frames=max_frames, fx=fx, bf=bf)


def as_bytes(o):
    return tuple(np.ascontiguousarray(o[k]).tobytes() for k in FIELDS) + (int(o["n_matched"]),)


def run_batch(corb, synth, config, cases, twice=False):
    sf = frontend(corb, config, len(cases))
    try:
        for s, c in enumerate(cases):
            sf.upload(s, *SC.images(synth, c))
        sf.run(len(cases)); sf.sync()
        outs = [sf.fetch(s) for s in range(len(cases))]
        if twice:
            sf.run(len(cases)); sf.sync()
            return outs, [sf.fetch(s) for s in range(len(cases))]
        return outs
    finally:
        sf.close()


_batches = {}


def batch(corb, synth, config):
    """results of the configuration's cases in table order, one batch; computed once"""
    if config not in _batches:
        _batches[config] = run_batch(corb, synth, config, SC.cases_of(config))
    return _batches[config]


def check_against_oracle(pyorc, synth, case, out, route):
    o = SC.oracle(pyorc, synth, case)
    what = "%s, %s" % (SC.describe(case), route)
    assert len(out["kl"]) == len(o["kl"]) and out["kl"].tobytes() == o["kl"].tobytes(), "left keypoints: " + what
    assert len(out["kr"]) == len(o["kr"]) and out["kr"].tobytes() == o["kr"].tobytes(), "right keypoints: " + what
    assert np.array_equal(out["dl"], o["dl"]) and np.array_equal(out["dr"], o["dr"]), "descriptors: " + what
    bad = np.nonzero((out["u_right"].view(np.uint32) != o["u_right"].view(np.uint32)) | (out["depth"].view(np.uint32) != o["depth"].view(np.uint32)))[0]
    if len(bad):
        decision = SC.restated(pyorc, synth, case)[4]
        rows = ["iL %d: oracle decision %s, oracle (uR %r, depth %r), device (uR %r, depth %r)" % (i, decision[i], float(o["u_right"][i]), float(o["depth"][i]),
                                                                                               float(out["u_right"][i]), float(out["depth"][i])) for i in bad[:6]]
        raise AssertionError("mvuRight / mvDepth differ at %d of %d left keypoints: %s\n%s" % (len(bad), len(o["kl"]), what, "\n".join(rows)))
    assert out["n_matched"] == o["n_matched"], "n_matched %d, oracle %d: %s" % (out["n_matched"], o["n_matched"], what)


@pytest.mark.parametrize("config", list(SC.CONFIGS))
def test_batch_matches_oracle(corb, pyorc, synth, config):
    cases = SC.cases_of(config)
    assert cases, config
    outs = batch(corb, synth, config)
    for case, out in zip(cases, outs):
        check_against_oracle(pyorc, synth, case, out, "batch of %d" % len(cases))


@pytest.mark.parametrize("n", [1, 2, 3])
def test_frames_call_equals_batch(corb, pyorc, synth, n):
    """corb_stereo_frames at n frames per call (stereo_pack_kernel): call c holds the cases FRAME_ORDER[c + 5 k], k < n, so every result block sees every case in
    FRAME_ORDER's cyclic order; the result buffer is reused, so a block holds the previous frame's entries beyond the new counts"""
    assert sorted(FRAME_ORDER) == sorted(SC.cases_of("base"))
    ref = dict(zip(SC.cases_of("base"), batch(corb, synth, "base")))
    sf = frontend(corb, "base", 4)
    try:
        lay = sf.frame_layout()
        result = np.zeros(n * lay.frame_bytes, np.uint8)
        m = len(FRAME_ORDER)
        for c in range(m):
            cases = [FRAME_ORDER[(c + 5 * k) % m] for k in range(n)]
            packed = np.ascontiguousarray(np.stack([np.stack(SC.images(synth, x)) for x in cases]))
            res = sf.frames(packed, result)
            for k, case in enumerate(cases):
                o = sf.unpack_frame(res, k)
                route = "per-frame call %d, block %d of %d" % (c, k, n)
                assert o["status"] == 0, route
                if as_bytes(o) != as_bytes(ref[case]):
                    check_against_oracle(pyorc, synth, case, o, route)           # says where, if the per-frame route is the one that is wrong
                    raise AssertionError("the per-frame route differs from the batch route: %s, %s" % (SC.describe(case), route))
    finally:
        sf.close()


@pytest.mark.parametrize("config", ["base", "deep"])
def test_same_batch_twice(corb, synth, config):
    cases = SC.cases_of(config)
    first, second = run_batch(corb, synth, config, cases, twice=True)
    for case, a, b in zip(cases, first, second):
        assert as_bytes(a) == as_bytes(b), "the second run of the same batch differs: " + SC.describe(case)
    for case, a, b in zip(cases, first, batch(corb, synth, config)):
        assert as_bytes(a) == as_bytes(b), "another handle gives other bytes: " + SC.describe(case)


@pytest.mark.parametrize("config", ["base", "deep"])
def test_slot_order_reversed(corb, synth, config):
    """a frame does not see its neighbours' row tables, candidate ranges or SAD lists"""
    cases = SC.cases_of(config)
    rev = run_batch(corb, synth, config, cases[::-1])[::-1]
    for case, a, b in zip(cases, rev, batch(corb, synth, config)):
        assert as_bytes(a) == as_bytes(b), "the frame's bytes depend on its slot: " + SC.describe(case)


def test_kinds_present():
    """by the CPU module's case table (asserted on the oracle's data in test_stereo_reference.py), not by the device"""
    ran = [c for config in SC.CONFIGS for c in SC.cases_of(config)]
    assert sorted(ran) == sorted(SC.CASES), "a case belongs to no configuration this module runs"
    supplied = set(k for c in ran for k in SC.SUPPLIES[c][1])
    assert supplied >= set(R.REQUIRED), "no case supplies %s" % sorted(set(R.REQUIRED) - supplied)
    per_frame = set(k for c in FRAME_ORDER for k in SC.SUPPLIES[c][1])
    only_intrinsics = {"left_better", "disp_big", "single_match"}                     # need a small fx: another handle, the batch route only
    assert per_frame >= set(R.REQUIRED) - only_intrinsics, sorted(set(R.REQUIRED) - only_intrinsics - per_frame)

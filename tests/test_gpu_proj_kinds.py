"""proj_grid_kernel, proj_prepare_map / _frame_kernel, init_prepare_kernel, proj_candidates_kernel, proj_resolve_kernel and init_resolve_kernel by kind of decision
(pytest -m gpu): every case of tests/proj_cases.py through corb_search_by_projection_map, corb_search_by_projection_frame and corb_search_for_initialization against
the CPU oracle -- the match array, the count and, for initialisation, vnMatches12 and vbPrevMatched as bit patterns.  All comparisons are exact.

Which decisions the cases reach is counted on the ORACLE's data by the Python restatement (tests/proj_reference.py lists the kinds; tests/test_proj_reference.py
asserts the restatement equal to the oracle, every kind present and which case supplies which).  Here the case table must name a supplier among the cases this
module runs for every required kind, so dropping a case cannot pass quietly; a mismatch is reported with the case, the kinds it is there for and the restatement's
decision for the first queries that differ.  Every call is made twice and must give the same bytes.

A case whose window holds more candidates than the list (256; 2048 for initialisation) must raise CORB_ERR_OVERFLOW, and the next ordinary call through the same
entry point must give its oracle bits: the status word does not stick.

Limits: the map overload at 6 000 features with 12 000 queries (the first size at which proj_resolve_kernel's dynamic LDS, 9 n + nq + 16 bytes, passes 64 KiB) and
with 60 000 queries (114 016 bytes) equals the oracle; 6 001 features and 60 001 queries are refused with CORB_ERR_ARG."""
import numpy as np
import pytest

import proj_cases as PC
import proj_reference as R

pytestmark = pytest.mark.gpu

RUN = [c for c in PC.CASES]
AFTER_OVERFLOW = {"map": "map_ratio", "frame": "frame_hist_tenth", "init": "init_basic"}       # the ordinary call that follows an overflow, per entry point


def report(case, c, o, g):
    """the first differing entries with the restatement's decision for the queries involved"""
    notes = PC.restated(case)[-1]
    bad = np.nonzero(o[0] != g[0])[0]
    rows = []
    for i in bad[:6]:
        if c["kind"] == "init":
            rows.append("F1 feature %d: oracle %d, device %d; restated: %s" % (i, o[0][i], g[0][i], notes[i]))
        else:
            qs = sorted(set(int(q) for q in (o[0][i], g[0][i]) if q >= 0))
            rows.append("feature %d: oracle query %d, device query %d; restated: %s" % (i, o[0][i], g[0][i], "; ".join("query %d: %s" % (q, notes[q]) for q in qs)))
    if c["kind"] == "init" and not len(bad):
        pm = np.nonzero(o[1].view(np.uint32) != g[1].view(np.uint32))[0]
        rows.append("prev_matched differs at rows %s" % pm[:6].tolist())
    return "%s: %d entries differ, count %d (oracle %d)\n%s" % (PC.describe(case), len(bad), g[-1], o[-1], "\n".join(rows))


def check(corb, pyorc, case):
    c = PC.build(case); o = PC.oracle(pyorc, case)
    g = PC.device_call(corb, c)
    assert len(g) == len(o)
    if PC.as_bytes(g) != PC.as_bytes(o):
        raise AssertionError(report(case, c, o, g))
    assert PC.as_bytes(PC.device_call(corb, c)) == PC.as_bytes(g), "the second call gives other bytes: " + PC.describe(case)


@pytest.mark.parametrize("case", [c for c in RUN if not PC.build(c)["overflow"]])
def test_case_equals_oracle(corb, pyorc, case):
    check(corb, pyorc, case)


@pytest.mark.parametrize("case", [c for c in RUN if PC.build(c)["overflow"]])
def test_overflow_is_reported_and_does_not_stick(corb, pyorc, case):
    c = PC.build(case)
    for _ in range(2):
        with pytest.raises(corb.CorbError) as e:
            PC.device_call(corb, c)
        assert "(-5)" in str(e.value), str(e.value)                  # CORB_ERR_OVERFLOW
    nxt = AFTER_OVERFLOW[c["kind"]]
    assert PC.build(nxt)["kind"] == c["kind"]
    check(corb, pyorc, nxt)


def test_nan_projection_has_no_match(corb, pyorc):
    """a point at the camera centre: u = v = NaN passes the bound tests; (int)floorf(NaN) is undefined in C, so only the common outcome is asserted -- no feature
    carries that query, on either side (the whole arrays are compared in test_case_equals_oracle)"""
    for case in ("frame_forward", "frame_backward", "frame_neither"):
        c = PC.build(case); notes = PC.restated(case)[-1]
        qs = [i for i, s in enumerate(notes) if "nan" in s]
        assert len(qs) == 1, notes
        assert not np.any(PC.oracle(pyorc, case)[0] == qs[0]) and not np.any(PC.device_call(corb, c)[0] == qs[0])


def test_kinds_present():
    """by the CPU module's case table (asserted on the oracle's data in test_proj_reference.py), not by the device"""
    assert sorted(RUN) == sorted(PC.CASES), "a case of the table is not run by this module"
    supplied = set(k for c in RUN for k in PC.SUPPLIES[c])
    assert supplied >= set(R.REQUIRED), "no case supplies %s" % sorted(set(R.REQUIRED) - supplied)
    for kind in ("map", "frame", "init"):
        assert any(PC.build(c)["overflow"] for c in RUN if PC.build(c)["kind"] == kind), "no overflow case for the %s entry point" % kind


# ---- limits ----
_limit = {}


def limit_scene(nq, n=6000, live=None):
    """n features spread over the image and nq map queries at (jittered) feature positions whose descriptors are their feature's with a few bits flipped; with `live`
    only every (nq // live)-th query is valid, so valid queries sit at indices up to nq"""
    key = (nq, n, live)
    if key not in _limit:
        rng = np.random.default_rng(991 + nq)
        keys = np.zeros(n, PC.KP_DTYPE)
        keys["x"] = rng.uniform(5, PC.W - 5, n).astype(np.float32); keys["y"] = rng.uniform(5, PC.H - 5, n).astype(np.float32); keys["octave"] = rng.integers(0, 8, n)
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        frame = dict(keys_un=keys, u_right=np.where(rng.random(n) < 0.5, keys["x"] - 20, -1).astype(np.float32), desc=desc, claimed=(rng.random(n) < 0.05).astype(np.uint8),
                     min_x=0.0, min_y=0.0, max_x=PC.W, max_y=PC.H, scale=PC.SCALE)
        src = rng.integers(0, n, nq)
        mps = np.zeros(nq, PC.TRACKED_DTYPE)
        mps["proj_x"] = keys["x"][src] + rng.normal(0, 1.5, nq); mps["proj_y"] = keys["y"][src] + rng.normal(0, 1.5, nq); mps["proj_xr"] = mps["proj_x"] - 20
        mps["view_cos"] = rng.choice([0.9, 0.9985], nq); mps["level"] = np.minimum(keys["octave"][src] + rng.integers(0, 2, nq), 7)
        mps["claims"] = rng.random(nq) < 0.9
        mps["valid"] = 1 if live is None else (np.arange(nq) % (nq // live) == 7)
        flip = np.unpackbits(desc[src], axis=1) ^ (rng.random((nq, 256)) < 0.05).astype(np.uint8)
        _limit[key] = (frame, mps, np.packbits(flip, axis=1))
    return _limit[key]


@pytest.mark.parametrize("nq,live", [(12000, None), (60000, 2000)])
def test_map_overload_at_its_limits(corb, pyorc, nq, live):
    frame, mps, desc = limit_scene(nq, live=live)
    assert 9 * 6000 + nq + 16 > 64 * 1024 and len(frame["keys_un"]) == 6000
    o = pyorc.search_by_projection_map(frame, mps, desc, 1.0, 0.8)
    assert o[1] > 1000 and o[0].max() >= nq - nq // 8, "the scene matches, also at its last queries"
    g = corb.ORBmatcher(0.8, True).SearchByProjection(frame, mps, desc, 1.0)
    bad = np.nonzero(o[0] != g[0])[0]
    assert len(bad) == 0 and g[1] == o[1], "%d features differ, first %s: oracle %s, device %s; count %d (oracle %d)" % (len(bad), bad[:6].tolist(), o[0][bad[:6]].tolist(),
                                                                                                                g[0][bad[:6]].tolist(), g[1], o[1])
    g2 = corb.ORBmatcher(0.8, True).SearchByProjection(frame, mps, desc, 1.0)
    assert g2[1] == g[1] and g2[0].tobytes() == g[0].tobytes()


def test_beyond_the_limits_is_refused(corb):
    frame, mps, desc = limit_scene(12000)
    big = dict(frame); n = 6001
    big["keys_un"] = np.resize(frame["keys_un"], n); big["u_right"] = np.resize(frame["u_right"], n); big["desc"] = np.resize(frame["desc"], (n, 32)); big["claimed"] = np.zeros(n, np.uint8)
    with pytest.raises(corb.CorbError) as e:
        corb.ORBmatcher(0.8, True).SearchByProjection(big, mps[:10], desc[:10], 1.0)
    assert "(-1)" in str(e.value), str(e.value)                      # CORB_ERR_ARG
    with pytest.raises(corb.CorbError) as e:
        corb.ORBmatcher(0.8, True).SearchByProjection(frame, np.resize(mps, 60001), np.resize(desc, (60001, 32)), 1.0)
    assert "(-1)" in str(e.value), str(e.value)

"""CPU checks of the seeded random case lists of tests/test_gpu_random_*.py: the lists are the same on every collection, the generated problems sit on both
sides of every route boundary they are meant to straddle, and the oracle alone flags what the >8-stage case needs it to flag (so that the GPU test cannot
pass by the oracle ignoring those stages as well)."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_random_ba as RB  # noqa: E402
import test_gpu_random_matchers as RM  # noqa: E402
import test_gpu_random_rgbd as RR  # noqa: E402


def _fingerprint(x):
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, dict):
        return tuple((k, _fingerprint(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(_fingerprint(v) for v in x)
    return repr(x)


def test_case_lists_are_deterministic():
    """a fresh import draws the same cases with the same ids (a failing id names a case that re-runs alone)"""
    for mod, lists in ((RB, ("BA_CASES", "POSE_CASES", "WINDOW_CASES", "STAGE_CASES")), (RM, ("SCW_CASES", "INIT_CASES", "MAP_CASES", "FRAME_CASES", "BOW_CASES")),
                       (RR, ("RGBD_CASES",))):
        before = {k: _fingerprint(getattr(mod, k)) for k in lists}
        again = importlib.reload(mod)
        for k in lists:
            assert _fingerprint(getattr(again, k)) == before[k], k
    for ids in ([RB.ba_case_id(c) for c in RB.BA_CASES], [RB.pose_case_id(c) for c in RB.POSE_CASES], [RB.window_case_id(c) for c in RB.WINDOW_CASES],
                [RB.stage_case_id(c) for c in RB.STAGE_CASES], [RR.rgbd_case_id(c) for c in RR.RGBD_CASES]):
        assert len(set(ids)) == len(ids)
    assert [RB.stage_list(c) for c in RB.STAGE_CASES] == [RB.stage_list(c) for c in RB.STAGE_CASES]


def test_generated_problems_are_deterministic(synth):
    for c in RB.BA_CASES[:3] + RB.WINDOW_CASES[:1]:
        mk = RB.ba_case_problem if "free" in c else RB.window_case_problem
        a, b = mk(synth, c), mk(synth, c)
        assert _fingerprint({k: a[k] for k in ("poses", "pose_fixed", "points", "point_fixed", "edges")}) == \
            _fingerprint({k: b[k] for k in ("poses", "pose_fixed", "points", "point_fixed", "edges")})


def _expected_route(c, free, nE, nL):
    """the route corb_ba.cpp takes (corb_ba_solve_ex): solver 0 picks dense up to 256 free poses; the fused one-workgroup optimiser only on the automatic
    choice with sp <= BA_SMALL_SP (96) and at most BA_SMALL_EDGES (2 048) edges and points; the in-LDS solve for sp <= 128; row Schur from 64 free poses;
    the coarse levels from 256 (with 16-pose blocks, the default from 128) unless pc_multilevel = 1"""
    solver = c["solver"] or (1 if free <= 256 else 2)
    if solver == 1:
        if c["solver"] == 0 and 6 * free <= 96 and nE <= 2048 and nL <= 2048:
            return RB.FUSED
        return RB.LDS if 6 * free <= 128 else RB.DENSE
    if c["ml"] != 1 and free >= 256:
        return RB.PCG_ML
    return RB.PCG_ROW if free >= 64 else RB.PCG


@pytest.fixture(scope="module")
def ba_problems(synth):
    return [RB.ba_case_problem(synth, c) for c in RB.BA_CASES]


def test_global_ba_cases_cover_every_route_on_both_sides_of_its_boundary(ba_problems):
    seen = {}
    for c, p in zip(RB.BA_CASES, ba_problems):
        free = int((p["pose_fixed"] == 0).sum()); nE = RB.active_edges(p)
        e = p["edges"]; act = ~((p["pose_fixed"][e["pose"]] != 0) & (p["point_fixed"][e["point"]] != 0))
        nL = len(np.unique(e["point"][act & (p["point_fixed"][e["point"]] == 0)]))
        assert free == c["free"], RB.ba_case_id(c)
        if c["edges"]:
            assert nE == c["edges"], RB.ba_case_id(c)
        assert _expected_route(c, free, nE, nL) == c["route"], RB.ba_case_id(c)
        seen.setdefault(c["route"], []).append((free, nE, c))
    assert set(seen) == {RB.FUSED, RB.LDS, RB.DENSE, RB.PCG, RB.PCG_ROW, RB.PCG_ML}
    frees = {f for f, _, _ in sum(seen.values(), [])}
    assert {15, 16, 17, 21, 22, 63, 64, 255, 256, 257} <= frees
    edges = {n for _, n, c in sum(seen.values(), []) if c["edges"]}
    assert {2047, 2048, 2049} <= edges
    # fused: 16 free poses with 2 048 edges, not with 2 049; 16 free poses on the automatic choice without the fused path only when the edges are too many
    assert any(f == 16 and n == 2048 for f, n, _ in seen[RB.FUSED]) and any(f == 16 and n == 2049 for f, n, _ in seen[RB.LDS])
    assert max(f for f, _, _ in seen[RB.FUSED]) == 16 and any(f == 17 for f, _, _ in seen[RB.LDS])
    assert max(f for f, _, _ in seen[RB.LDS]) == 21 and min(f for f, _, _ in seen[RB.DENSE]) == 22
    assert max(f for f, _, _ in seen[RB.PCG]) == 63 and min(f for f, _, _ in seen[RB.PCG_ROW]) == 64
    assert max(f for f, _, c in seen[RB.DENSE] if c["solver"] == 0) == 256 and min(f for f, _, c in seen[RB.PCG_ML] if c["solver"] == 0) == 257
    assert min(f for f, _, _ in seen[RB.PCG_ML]) == 256 and any(f == 255 for f, _, _ in seen[RB.PCG_ROW])
    assert any(c["ml"] == 1 and f >= 256 for f, _, c in seen[RB.PCG_ROW])          # the coarse levels switched off above their size
    assert any(c["devflat"] for c in RB.BA_CASES) and {True, False} == {c["robust"] for c in RB.BA_CASES}
    assert {1, 2, 3, 4, 5, 6} <= {c["clients"] for c in RB.BA_CASES} and any(c["fix_kf"] for c in RB.BA_CASES)
    assert any(p["point_fixed"].any() for p in ba_problems)


def test_staged_cases_cover_both_routes_and_stage_counts(synth, pyorc):
    dev = []
    for c in RB.WINDOW_CASES:
        p = RB.window_case_problem(synth, c)
        e = p["edges"]
        assert np.all(np.diff(e["point"]) >= 0)                                           # grouped ...
        assert not np.all(np.diff(e[RB.moved_order(e)]["point"]) >= 0)                   # ... and the moved copy is not
        if c["edges"]:
            assert (len(e) if c["count"] == "raw" else RB.active_edges(p)) == c["edges"]
        dev.append((len(e), RB.active_edges(p), RB.window_expects_device(p)))
    assert any(n == 2048 and not d for n, _, d in dev) and any(n == 2047 and not d for n, _, d in dev)      # raw edge count at / below BA_SMALL_EDGES: host
    assert any(a == 2049 and d for _, a, d in dev) and sum(d for _, _, d in dev) >= 3                         # active edges just above it: device
    counts = {c["n_stages"] for c in RB.STAGE_CASES}
    assert {1, 4, 8, 9, 12, 15} <= counts
    for c in RB.STAGE_CASES:
        st = RB.stage_list(c)
        assert len(st) == c["n_stages"] <= 15 and all(s[7] == 0 for s in st[1:])        # corb_ba_staged_device_wanted: <= 15 stages, no reset after the first
        p, pf, pts, ff = RB.stage_case_problem(synth, c)
        assert RB.window_expects_device(p) and pf[p["edges"]["point"][ff]] and p["pose_fixed"][p["edges"]["pose"][ff]]
    sizes = {c["n"] for c in RB.POSE_CASES}
    assert {60, 63, 64, 65, 255, 256, 257, 511, 512, 2049, 3000} <= sizes and {0, 1} == {c["solver"] for c in RB.POSE_CASES}


@pytest.mark.parametrize("c", [c for c in RB.STAGE_CASES if c["late_depth"]], ids=[RB.stage_case_id(c) for c in RB.STAGE_CASES if c["late_depth"]])
def test_oracle_flags_the_edge_that_stages_after_the_eighth_decide(synth, pyorc, c):
    """the >8-stage cases: the oracle flags the observation behind the fixed camera, which only a stage after the eighth tests for depth; replaying the first
    eight stages alone would leave it unflagged"""
    p, pf, pts, ff = RB.stage_case_problem(synth, c)
    stages = RB.stage_list(c)
    assert len(stages) > 8 and not any(s[4] for s in stages[:8]) and all(s[4] for s in stages[8:])
    a = (p["poses"], p["pose_fixed"], pts, pf, p["edges"], p["fx"], p["fy"], p["cx"], p["cy"], p["bf"])
    r = pyorc.ba_solve_staged(*a, stages)
    assert r["outlier"][ff] == 1 == RB.stage_flags_behind(stages, ff, r)
    assert RB.stage_flags_behind(stages[:8], ff, r) == 0


def test_pose_cases_have_outliers_in_the_oracle(synth, pyorc):
    """every PoseOptimization case has something to classify (the GPU test asserts flags equal to these)"""
    for c in RB.POSE_CASES:
        q = RB.pose_case_problem(synth, c)
        n = c["n"]
        r = pyorc.ba_solve_staged(q["Tcw0"].reshape(1, 16), np.zeros(1, np.uint8), q["points"], np.ones(n, np.uint8), RB.pose_edges(pyorc, q),
                                  q["fx"], q["fy"], q["cx"], q["cy"], q["bf"], pyorc.POSE_OPT_STAGES)
        assert 0 < r["outlier"].sum() < n, RB.pose_case_id(c)


def test_matcher_and_rgbd_cases_reach_their_edges():
    assert any(c["n1"] < 64 for c in RM.BOW_CASES) and any(c["n1"] > 2048 or c["n2"] > 2048 for c in RM.BOW_CASES)
    assert any(c["n"] < 64 for c in RM.MAP_CASES) and any(c["n"] > 2048 for c in RM.MAP_CASES)
    assert {w % 4 for w, _ in RR.SIZES} >= {0, 1, 2, 3} and {(129, 97), (403, 263), (1283, 381)} <= set(RR.SIZES)
    cs = RR.RGBD_CASES
    assert {1, 3, 4} <= {c["channels"] for c in cs} and {0, 1} <= {c["rgb"] for c in cs if c["channels"] > 1} and {"u16", "f32"} <= {c["depth"] for c in cs if c["sensor"] == "rgbd"}
    assert {1.0, 2.5, 5000.0} <= {c["cam"]["depth_map_factor"] for c in cs if c["sensor"] == "rgbd"}
    k = [c["cam"] for c in cs]
    assert any(x["k1"] < 0 for x in k) and any(x["k1"] > 0 for x in k) and any(x["k3"] != 0 for x in k) and any(x["k1"] == 0 and (x["p1"] or x["p2"]) for x in k)
    assert any(c["sensor"] == "mono" for c in cs)
    # frame 1 of a packed batch starts at an unaligned byte offset on the odd sizes
    assert any((c["w"] * c["h"] * (c["channels"] + (0 if c["sensor"] == "mono" else 2 if c["depth"] == "u16" else 4))) % 4 for c in cs)

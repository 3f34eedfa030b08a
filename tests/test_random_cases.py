"""CPU checks of the seeded random case lists of tests/test_gpu_random_*.py: the lists are the same on every collection, the generated problems sit on both
sides of every route boundary they are meant to straddle, and the oracle alone flags what the >8-stage case needs it to flag (so that the GPU test cannot
pass by the oracle ignoring those stages as well).  For the loop-closing optimisers (tests/test_gpu_random_loop.py): the lists reach every size and structure
they name, the oracle alone takes the branches the cases were built for, its decisions do not move when an input moves by one unit in the last place (so that
equal flags and iteration counts are a fair demand on the GPU), and the mpmath reference of the Sim3 arithmetic agrees with scipy's matrix logarithm."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_random_ba as RB  # noqa: E402
import test_gpu_random_loop as RL  # noqa: E402
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


# ---- the loop-closing optimisers: tests/test_gpu_random_loop.py ----
def test_loop_case_lists_are_deterministic():
    global RL
    lists = ("SIM3_CASES", "SIM3_BATCHES", "GRAPH_CASES")
    before = {k: _fingerprint(getattr(RL, k)) for k in lists}
    sweep = _fingerprint(RL.sweep_points())
    RL = importlib.reload(RL)
    for k in lists:
        assert _fingerprint(getattr(RL, k)) == before[k], k
    assert _fingerprint(RL.sweep_points()) == sweep
    for ids in ([RL.sim3_case_id(c) for c in RL.SIM3_CASES], [RL.sim3_batch_id(b) for b in RL.SIM3_BATCHES], [RL.graph_case_id(c) for c in RL.GRAPH_CASES]):
        assert len(set(ids)) == len(ids)
    assert [c["i"] for c in RL.SIM3_CASES] == list(range(len(RL.SIM3_CASES))) and [c["i"] for c in RL.GRAPH_CASES] == list(range(len(RL.GRAPH_CASES)))
    keys = ("p1c", "p2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "R12", "t12", "s12", "fx1", "fy2")
    for c in RL.SIM3_CASES[5:9]:
        a, b = RL.sim3_case_problem(c), RL.sim3_case_problem(c)
        assert _fingerprint({k: a[k] for k in keys}) == _fingerprint({k: b[k] for k in keys})


def _sim3_runs():
    """every (case, th2, fix_scale) the GPU tests run: each case singly with its own values, and as a member of its batches with the batch's"""
    return [(c, c["th2"], c["fix_scale"]) for c in RL.SIM3_CASES] + [(RL.SIM3_CASES[m], b["th2"], b["fix_scale"]) for b in RL.SIM3_BATCHES for m in b["members"]]


def test_sim3_cases_reach_every_size_branch_and_setting():
    cs = RL.SIM3_CASES
    assert set(RL.SIM3_SIZES) == {0, 1, 3, 6, 7, 9, 10, 11, 63, 64, 65, 255, 256, 257, 513, 2000} <= {c["n"] for c in cs}
    qs = [RL.sim3_case_problem(c) for c in cs]
    for c, q in zip(cs, qs):
        assert len(q["p1c"]) == len(q["obs2"]) == len(q["inv_sigma2_1"]) == c["n"]
        assert len({np.float32(q[k]) for k in ("fx1", "fy1", "fx2", "fy2")}) == 4 and len({np.float32(q[k]) for k in ("cx1", "cy1", "cx2", "cy2")}) == 4     # unequal intrinsics
        assert q["fx1"] != q["fx2"] and q["fy1"] != q["fy2"] and q["cx1"] != q["cx2"] and q["cy1"] != q["cy2"]
        if c["n"]:
            assert q["p1c"][:, 2].min() > 1.0 and q["p2c"][:, 2].min() > 1.0                                  # in front of both cameras
        # the initial and the true rotation take the branch the case names
        for R in (q["R12"], q["R_true"]):
            assert RL.quat_branch(R) == ((True, None) if c["pivot"] is None else (False, c["pivot"])), RL.sim3_case_id(c)
    br = {RL.quat_branch(q["R12"]) for q in qs}
    assert br == {(True, None), (False, 0), (False, 1), (False, 2)}
    assert max(c["angle"] for c in cs) >= 170
    runs = _sim3_runs()
    assert {6.0, 10.0, 20.0} == {th2 for _, th2, _ in runs} and {True, False} == {bool(fs) for _, _, fs in runs}
    assert {0.5, 2.5} <= {c["scale"] for c in cs}
    assert set(sum((b["members"] for b in RL.SIM3_BATCHES), [])) == set(range(len(cs)))                    # every case also runs inside a batch
    assert any(cs[b["members"][k]]["n"] == 0 and cs[b["members"][k - 1]]["n"] > 10 and cs[b["members"][k + 1]]["n"] > 10
               for b in RL.SIM3_BATCHES for k in range(1, len(b["members"]) - 1))                          # n = 0 between two ordinary problems
    assert all(cs[m]["fix_scale"] for b in RL.SIM3_BATCHES if b["fix_scale"] for m in b["members"])


def test_sim3_oracle_takes_the_branches_the_cases_were_built_for(pyorc):
    cs = RL.SIM3_CASES
    # exactly 10 and exactly 9 survivors of the first round
    for ci, surv in ((RL.SURV10, 10), (RL.SURV9, 9)):
        c = cs[ci]; q = RL.sim3_case_problem(c)
        r = pyorc.optimize_sim3(q, c["th2"], c["fix_scale"])
        assert c["n"] - r["round1_removed"] == surv and np.array_equal(r["removed"].astype(bool), q["bad"])
        if surv == 10:
            assert r["n_in"] == 10 and r["iters_done"] > r["round1_iters"] and r["s"] != q["s12"]
        else:
            assert r["n_in"] == 0 and r["iters_done"] == r["round1_iters"]
            assert r["s"] == q["s12"] and np.array_equal(r["R"], q["R12"]) and np.array_equal(r["t"], q["t12"])          # the estimate is untouched
    # nBad == 0: nothing removed in round one, the second round runs at most 5 iterations
    c = cs[RL.CLEAN]; q = RL.sim3_case_problem(c)
    r = pyorc.optimize_sim3(q, c["th2"], c["fix_scale"])
    assert r["round1_removed"] == 0 and r["removed"].sum() == 0 and r["n_in"] == c["n"] and r["round1_iters"] < r["iters_done"] <= r["round1_iters"] + 5
    # n < 7.  The stop after ten rejected trials (qmax == 10: s3_ldlt7 refuses the system ten times) is what n = 0 does: H = 0 and lambda = 1e-5 max diag(H) = 0.
    # With 1 <= n < 7 pairs H is rank deficient but H + lambda I is not (lambda = 1e-5 max diag(H) > 0): the factorisation succeeds and the first round runs
    # its iterations with every trial accepted -- measured here, not assumed; the second round never runs (n - nBad < 10)
    small = [c for c in cs if c["n"] < 7]
    assert {c["n"] for c in small} == {0, 1, 3, 6}
    for c in small:
        q = RL.sim3_case_problem(c)
        r = pyorc.optimize_sim3(q, c["th2"], c["fix_scale"])
        assert r["n_in"] == 0 and r["s"] == q["s12"] and r["iters_done"] == r["round1_iters"]
        if c["n"] == 0:
            assert (r["round1_iters"], r["round1_trials"], r["last_accepted"]) == (1, 10, False)
        else:
            assert r["round1_iters"] == 5 and r["round1_trials"] == 5 and r["last_accepted"], (RL.sim3_case_id(c), r["round1_iters"], r["round1_trials"])
    # somewhere a trial is rejected and the optimisation goes on (the restore of s_bak), and somewhere the last trial is rejected (the check from the estimate is skipped there)
    rs = [pyorc.optimize_sim3(RL.sim3_case_problem(c), th2, fs) for c, th2, fs in _sim3_runs() if c["n"] >= 10]
    assert any(r["trials"] > r["iters_done"] and r["n_in"] > 0 for r in rs)


def _moved_one_ulp(q):
    n = len(q["obs1"])
    q2 = dict(q)
    if n:
        o = q["obs1"].copy(); o[n // 2, 0] = np.nextafter(o[n // 2, 0], np.float32(np.inf)); q2["obs1"] = o
    return q2


def test_sim3_oracle_decisions_are_stable_and_agree_with_its_own_estimate(pyorc):
    """every run of the GPU tests: one observation moved by one float32 ulp changes no flag and no count (a seed that fails is replaced in the list, not tolerated
    at GPU time), and where the second round ran and its last trial was accepted, the oracle's flags are those its own estimate gives in numpy float64, with at most
    2 % of the pairs inside the band around the threshold that the comparison leaves out"""
    checked = 0
    for c, th2, fs in _sim3_runs():
        q = RL.sim3_case_problem(c)
        r = pyorc.optimize_sim3(q, th2, fs)
        r2 = pyorc.optimize_sim3(_moved_one_ulp(q), th2, fs)
        assert np.array_equal(r["removed"], r2["removed"]) and r["n_in"] == r2["n_in"] and r["iters_done"] == r2["iters_done"], (RL.sim3_case_id(c), th2, fs)
        if RL.second_round_ran(q, r):
            _, decided = RL.sim3_flags_from_estimate(q, r, th2)
            assert (~decided).sum() <= RL.BAND_CAP * c["n"], (RL.sim3_case_id(c), th2, fs)
            checked += RL.sim3_check_flags(q, r, th2, r["last_accepted"])
        else:
            assert r["n_in"] == 0
    assert checked >= 20


@pytest.fixture(scope="module")
def graph_problems(synth):
    return [RL.graph_case_problem(synth, c) for c in RL.GRAPH_CASES]


def test_graph_cases_reach_every_size_and_structure(graph_problems):
    cs = RL.GRAPH_CASES
    st = [RL.graph_structure(g) for g in graph_problems]
    for c, g, s in zip(cs, graph_problems, st):
        assert s["nP"] == c["nP"] and g["K"] == c["nP"] + c["nfix"] and int(g["fixed"].sum()) == c["nfix"], RL.graph_case_id(c)
        assert s["isolated_free"] == (1 if c["iso"] else 0)
        assert len(g["points"]) == len(g["ref"]) == c["n_points"]
        assert np.all(g["vi"] != g["vj"]) and g["vi"].min() >= 0 and max(g["vi"].max(), g["vj"].max()) < g["K"]
        # every component but the isolated vertex holds a fixed vertex: the chain joins all other vertices, and there is a fixed one
        reach = np.zeros(g["K"], bool); reach[g["fixed"].astype(bool)] = True
        for _ in range(g["K"]):
            reach[g["vi"][reach[g["vj"]]]] = True; reach[g["vj"][reach[g["vi"]]]] = True
        assert int((~reach).sum()) == (1 if c["iso"] else 0)
        assert c["scales"] or c["far"] is not None or np.array_equal(g["S"][:, 7], np.ones(g["K"]))
        assert (np.abs(g["meas"][:, 7] - 1.0).max() == 0.0) == (not c["scales"])
        if c["scales"]:
            assert 0.7 <= g["meas"][:, 7].min() < 0.95 and 1.05 < g["meas"][:, 7].max() <= 1.4
        if c["traj"] == "line":
            assert np.array_equal(g["S"][:, :3], np.zeros((g["K"], 3))) and np.array_equal(g["meas"][:, :3], np.zeros((len(g["meas"]), 3)))       # identity rotations
    assert set(RL.GRAPH_NP) == {1, 4, 5, 9, 10, 18, 19, 37, 150, 260} <= {s["nP"] for s in st}
    assert all(1 <= c["nfix"] <= 6 for c in cs) and {1, 6} <= {c["nfix"] for c in cs}
    assert any(s["free_free_up"] > 0 and s["free_free_down"] > 0 for s in st)                              # both orientations among free-free pairs (flip 0 and 1)
    assert any(2 <= s["max_parallel"] <= 4 for s in st)
    assert any(s["fixed_vi"] > 0 and s["fixed_vj"] > 0 and s["both_fixed"] > 0 and s["fixed_inside"] >= 2 for s in st)
    assert sum(s["isolated_free"] for s in st) == 1
    big = st[RL.GRAPH_BIG]
    assert big["E"] > 65536 and 35 <= graph_problems[RL.GRAPH_BIG]["K"] <= 45 and big["max_parallel"] >= 256 and big["both_fixed"] > 0
    assert {0, 1, 20} == {c["iters"] for c in cs} and {0, 1, 400} == {c["n_points"] for c in cs} and {True, False} == {c["fix_scale"] for c in cs}
    assert any(c["traj"] == "line" for c in cs)
    g = graph_problems[1]
    assert (g["ref"] == -1).any() and (g["ref"] >= g["K"]).any() and ((g["ref"] >= 0) & (g["ref"] < g["K"])).any()
    assert RL.graph_structure(graph_problems[RL.GRAPH_REPEAT])["max_parallel"] >= 2


def test_graph_oracle_is_stable_and_rejects_a_trial_on_the_far_start(pyorc, graph_problems):
    """one measurement entry moved by one ulp leaves every case's iteration count as it is; the far start makes the oracle reject Levenberg trials (push / pop) and
    then accept one; points whose reference is -1 or >= K come back untouched"""
    for c, g in zip(RL.GRAPH_CASES, graph_problems):
        R = pyorc.optimize_essential_graph(g, c["iters"], c["fix_scale"])
        R2 = pyorc.optimize_essential_graph(RL.graph_perturbed(g), c["iters"], c["fix_scale"])
        assert R["iters_done"] == R2["iters_done"], RL.graph_case_id(c)
        assert np.isfinite(R["S"]).all() and np.isfinite(R["chi2"]).all()
        out = (g["ref"] < 0) | (g["ref"] >= g["K"])
        assert np.array_equal(R["points"][out], g["points"][out])
        if c["iters"] == 0:
            assert R["iters_done"] == 0 and R["trials"] == 0 and np.array_equal(R["S"], g["S"])
        if c["iso"]:
            assert np.array_equal(R["S"][g["iso"]], g["S"][g["iso"]])                                    # the isolated free vertex has nothing to move it
        if c["i"] == RL.GRAPH_FAR:
            assert R["trials"] > R["iters_done"] and R["chi2"][-1] < R["chi2"][-2]                         # rejected trials, then an accepted one that lowered chi2
    assert RL.GRAPH_CASES[RL.GRAPH_FAR]["far"] is not None


def test_mpmath_sim3_log_agrees_with_scipy_logm():
    """the new reference against an implementation it shares nothing with: log of the 4 x 4 matrix [s R t; 0 1] is [sigma I + [omega]x, upsilon; 0 0] (sim3.h's W is
    the integral of exp(tau (sigma I + [omega]x)) over 0 .. 1).  On the large-angle points of the sweep, where logm is well conditioned"""
    from scipy.linalg import logm
    n = 0
    for pt in RL.sweep_points():
        if pt["theta"] < 1.0:
            continue
        C = pt["C"]
        q = RL.mp_sim3(C)[0]
        R = np.array([[float(x) for x in row] for row in RL.mp_R(q).tolist()])
        M = np.eye(4); M[:3, :3] = C[7] * R; M[:3, 3] = C[4:7]
        L = np.real(logm(M))
        ref = np.r_[L[2, 1], L[0, 2], L[1, 0], L[:3, 3], (L[0, 0] + L[1, 1] + L[2, 2]) / 3]
        mine = np.array([float(x) for x in RL.mp_log(RL.mp_sim3(C))])
        assert np.abs(mine - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), (pt["theta"], pt["sigma"], mine, ref)
        n += 1
    assert n >= 20


def test_sim3_log_sweep_reaches_all_four_branches_and_measures_the_oracle(pyorc):
    """the sweep holds theta and |sigma| on both sides of each threshold, all four branch combinations of s3_log, and the oracle's own distance from mpmath (the
    baseline of tests/test_gpu_random_loop.py::test_sim3_log_against_mpmath) is what that test's docstring says"""
    pts = RL.sweep_points()
    assert {(pt["theta"], abs(pt["sigma"])) for pt in pts} == {(a, b) for a in RL.SWEEP_VALUES for b in RL.SWEEP_VALUES}
    assert {0, 1e-9, 0.99e-5, 1.01e-5, 1e-3, 1, 3.0} == set(RL.SWEEP_VALUES)
    assert max(np.abs(pt["C"][4:7]).max() for pt in pts) > 40 and max(np.abs(pt["Si"][4:7]).max() for pt in pts) > 40
    base = RL.oracle_log_errors(pyorc)
    worst = {}
    for b, _, e in base:
        worst[b] = max(worst.get(b, 0.0), e)
    print({b: "%.3g" % e for b, e in worst.items()})
    assert set(worst) == {"sigma<eps/d<=1-eps", "sigma<eps/d>1-eps", "sigma>=eps/d<=1-eps", "sigma>=eps/d>1-eps"}
    # the general closed form is a float64 evaluation of exact formulas; |sigma| < 1e-5 is read as sigma = 0 (C = 1 for (s - 1) / sigma = 1 + sigma / 2 + ...: up to
    # 5e-6 in upsilon, 1e-5 in chi2); sigma >= eps with d > 1 - eps carries sim3.h:199's B and is off by order 1 (see the GPU test's docstring)
    assert worst["sigma>=eps/d<=1-eps"] < 1e-9 and worst["sigma<eps/d<=1-eps"] < 2e-5 and worst["sigma<eps/d>1-eps"] < 2e-5
    # the oracle's SE3 recovery and point map against the same reference (1 float32 ulp), so that the GPU test's reference is known to be right before it is used
    for pt in pts[::5]:
        g = RL.sweep_graph(pt)
        R = pyorc.optimize_essential_graph(g, 0, False)
        RL._check_apply(R, g["S"], g["S"], pt["p"])
        g1 = dict(g); g1["fixed"] = np.array([0, 1], np.uint8)
        R1 = pyorc.optimize_essential_graph(g1, 1, False)
        assert np.isfinite(R1["S"]).all()
        RL._check_apply(R1, g["S"], R1["S"], pt["p"])


# ---- the calls on device-resident records: tests/test_gpu_random_records.py, tests/records_reference.py ----
import records_reference as R  # noqa: E402
import test_gpu_random_records as RC  # noqa: E402

RC_LISTS = ("TRACK_POSE_CASES", "TRACK_LAST_CASES", "TRACK_LOCAL_CASES", "REC_RELOC_CASES", "REC_SCW_CASES", "REC_SIM3_CASES", "REC_FUSE_CASES", "REPLACE_CASES",
            "DISTINCTIVE_SIZES")


def test_record_case_lists_are_deterministic_and_reach_every_size_and_setting():
    global RC
    before = {k: _fingerprint(getattr(RC, k)) for k in RC_LISTS}
    RC = importlib.reload(RC)
    for k in RC_LISTS:
        assert _fingerprint(getattr(RC, k)) == before[k], k
    for k in RC_LISTS[:-1]:
        cs = getattr(RC, k)
        ids = [RC._id("x", c, sorted(set(c) - {"i", "seed"})) for c in cs]
        assert len(set(ids)) == len(ids) and [c["i"] for c in cs] == list(range(len(cs))), k
    P = RC.TRACK_POSE_CASES
    assert {0, 2, 3, 9, 10, 11} <= {c["edges"] for c in P} and {63, 64, 65, 1023, 1024, 1025, 2049, 3000} <= {c["n"] for c in P}
    assert all(0.4 * c["n"] <= c["edges"] <= 0.7 * c["n"] for c in P if c["n"] >= 1023 or c["i"] in (6, 7, 8))
    assert {0, 1, 37} == {c["F"] - c["n"] for c in P} and {True, False} == {c["discard"] for c in P} and sum(c["collide"] for c in P) == 1
    assert any(c["F"] % 64 for c in P)
    sizes = {40, 63, 64, 65, 700, 2100, 2900}
    for cs, other in ((RC.TRACK_LAST_CASES, "n_last"), (RC.TRACK_LOCAL_CASES, "n_local")):
        assert sizes <= {c["n_cur"] for c in cs} and sizes <= {c[other] for c in cs} and {c[other] for c in cs} <= sizes and all(c["n_cur"] != c[other] for c in cs)
        assert sum(c["collide"] for c in cs) == 1 and len({c["th"] for c in cs}) == 2 and len({c["nnratio"] for c in cs}) == 2
    assert {True, False} == {c["mono"] for c in RC.TRACK_LAST_CASES} == {c["ori"] for c in RC.TRACK_LAST_CASES}
    assert sum(c["only_bad"] for c in RC.TRACK_LOCAL_CASES) == 1
    assert {50, 64, 600, 2100} == {c["n"] for c in RC.REC_RELOC_CASES} and sum(c["cur_smaller"] for c in RC.REC_RELOC_CASES) * 2 == len(RC.REC_RELOC_CASES)
    for cs in (RC.REC_SCW_CASES, RC.REC_SIM3_CASES, RC.REC_FUSE_CASES):
        assert {40, 63, 65, 600, 2100} <= {c["n"] for c in cs} and {1.0, 0.3} == {c["span"] for c in cs}
    assert {True, False} == {c["apply"] for c in RC.REC_FUSE_CASES} and {2, 8} == {c["max_obs"] for c in RC.REC_FUSE_CASES}
    assert {True, False} == {c["later"] for c in RC.REC_FUSE_CASES if c["apply"] and c["max_obs"] == 2}
    assert [c["merged"] for c in RC.REPLACE_CASES] == [1, 2, 63, 64, 65, 80] and RC.REPLACE_O == 80 and RC.REPLACE_NKF == 96 and RC.REPLACE_F == 8
    D = RC.DISTINCTIVE_SIZES
    assert {1, 2, 3, 4, 63, 64, 65, 128, 1023, 1024} <= set(D) and any(D[k] == 0 and D[k - 1] > 0 and D[k + 1] > 0 for k in range(1, len(D) - 1))


def test_record_pose_cases_have_the_edges_they_name_and_outliers_in_the_oracle(synth, pyorc):
    for c in RC.TRACK_POSE_CASES:
        p = RC.track_pose_problem(synth, c)
        e, r = RC.track_pose_reference(pyorc, p)
        E = len(e["feat"])
        assert E == c["edges"] and e["klass"] == (0 if E < 3 else 1 if E < 10 else 4) and np.all(np.diff(e["feat"]) > 0), c
        fl = p["fr"]["flags"]
        assert (fl == 2).any() or E < 3
        assert E == 0 or c["n"] < 100 or ((fl == 4).any() and (fl == 6).any() and (p["fr"]["mp_id"] == R.NONE).any() and (p["rec"]["flags"] & 1).any())
        if E >= 3:
            assert e["mono"].any() and not e["mono"].all()
        if E >= 10:
            assert 0 < r["outlier"].sum() < E, c
        if c["n"] >= 1023:                           # every 1024-chunk and every wave of 64 features has edges and gaps
            has = np.zeros(-(-c["n"] // 64) * 64, bool); has[e["feat"]] = True
            per = has.reshape(-1, 64).sum(1)
            assert per[:-1].min() > 0 and per.max() < 64
        if c["collide"]:
            assert R.probe_chain(p["rec"]["id"], R.id_table_cells(c["n"]))[0] >= 8


def test_record_tracking_cases_match_and_see_something_in_the_oracle(synth, pyorc):
    for c in RC.TRACK_LAST_CASES:
        p = RC.track_last_problem(synth, c)
        m, n, lastp, claimed = RC.track_last_reference(pyorc, c, p)
        assert n > 0 and 0 < lastp["valid"].sum() < c["n_last"], c
        assert claimed.any() or c["n_cur"] < 100, c
    for c in RC.TRACK_LOCAL_CASES:
        p = RC.track_local_problem(synth, c)
        m, n, exp, after = RC.track_local_reference(pyorc, c, p)
        assert n > 0 and 0 < int(exp["valid"].sum()) < c["n_local"], c
        assert (after != p["cur"]["mp_id"]).any(), c                                          # a bad point left the frame
        if c["only_bad"]:
            assert (after == R.NONE).all()
        if c["collide"]:
            seen = sorted(R.seen_in_frame(p["cur"]["mp_id"], p["cur"]["flags"], p["rec"], p["slot_of"]))      # what the call's in-frame table holds
            for ids in (p["rec"]["id"], seen):
                longest, wrapped = R.probe_chain(ids, R.id_table_cells(c["n_cur"]))
                assert longest >= 8 and wrapped > 0


def test_record_keyframe_matcher_cases_match_in_the_oracle(synth, pyorc):
    for c in RC.REC_RELOC_CASES:
        p = RC.rec_reloc_problem(synth, c)
        m, n, v, claimed = RC.rec_reloc_reference(pyorc, c, p)
        assert n > 0 and 0 < v["valid"].sum() < c["n"] and claimed.any(), c
        assert (R.slots_of(p["cur"]["mp_id"][claimed != 0], p["slot_of"]) < 0).any()           # held ids the store does not know
    for c in RC.REC_SCW_CASES:
        assert RC.rec_scw_reference(pyorc, c, RC.rec_scw_problem(synth, c))[1] > 0, c
    for c in RC.REC_SIM3_CASES:
        p = RC.rec_sim3_problem(synth, c)
        m0, n0, _, _ = RC.rec_sim3_reference(pyorc, c, p, None)
        m1, n1, v1, v2 = RC.rec_sim3_reference(pyorc, c, p, p["matched"])
        assert n0 > 0 and n1 > 0 and not v1["valid"][p["pre"]].any() and not v2["valid"][p["at"][2:]].any(), c
        pos = {R.index_in_keyframe(p["lists"][s], RC.KF2_ID) >= 0 and [k for k, _ in p["lists"][s]].index(RC.KF2_ID) for s in R.slots_of(p["matched"][p["pre"]], p["slot_of"]) if s >= 0}
        assert {0, c["max_obs"] // 2, c["max_obs"] - 1} <= pos
    for c in RC.REC_FUSE_CASES:
        p = RC.rec_fuse_problem(synth, c)
        bi, bd, nf = RC.rec_fuse_reference(pyorc, c, p)
        mp, act, lists = R.fuse_writes(bi, p["held"], p["rec"]["id"], p["lists"], RC.KF2_ID)
        assert nf > 0 and (act == 1).any() and ((act == 2).any() or c["n"] < 100), c
        if c["max_obs"] == 2 and c["apply"]:                                                  # with a later observer the full-list error path is taken, without it never
            assert any(act[i] == 1 and len(p["lists"][i]) >= 2 for i in range(c["n"])) == c["later"]


def test_replace_and_distinctive_cases_tie_on_the_least_median(pyorc):
    bests = []
    for c in RC.REPLACE_CASES:
        p = RC.replace_problem(c)
        st, into, act, _ = pyorc.mappoint_replace(100, 200, p["this"], p["into"], RC.REPLACE_O)
        rows = RC.replace_rows(p, into)
        assert st == 0 and len(rows) == c["merged"] and len(into) <= RC.REPLACE_O and {1, 2} <= set(act.tolist()) | ({1, 2} if c["merged"] <= 2 else set()), c
        assert any(k == 0 for k, _ in into) or c["merged"] < 2
        if len(rows) >= 3:
            med = R.row_medians(np.stack(rows))
            assert (med == med.min()).sum() >= 2
            bests.append(int(pyorc.distinctive_descriptors(np.stack(rows), np.array([0, len(rows)], np.int32))[0]))
            assert bests[-1] == int(np.argmin(med))
    desc, offset = RC.distinctive_problem()
    r = pyorc.distinctive_descriptors(desc, offset)
    for k, N in enumerate(RC.DISTINCTIVE_SIZES):
        if N == 0:
            assert r[k] == -1
            continue
        med = R.row_medians(desc[offset[k]: offset[k + 1]])
        assert r[k] == int(np.argmin(med))                                                      # the first row with the least median
        if N >= 3:
            assert (med == med.min()).sum() >= 2
            bests.append(int(r[k]))
    assert any(b > 0 for b in bests) and any(b >= 64 for b in bests)                            # not always row 0, and past the first wave


def test_colliding_ids_collide_under_the_restated_hash():
    for cells in (256, 2048, 8192):
        ids = R.colliding_ids(cells // 2 - 3, cells, np.random.default_rng(cells))
        assert len(set(ids.tolist())) == len(ids) and 0 in ids.tolist() and (1 << 64) - 2 in ids.tolist() and R.NO_MAP_POINT not in ids.tolist()
        assert sum((R.id_hash(int(k)) & (cells - 1)) >= cells - 4 for k in ids) >= 16
        longest, wrapped = R.probe_chain(ids, cells)
        assert longest >= 8 and wrapped >= 8
        assert R.id_table_cells(len(ids)) == cells
    assert [R.id_table_cells(n) for n in (0, 1, 32, 33, 1024, 1025)] == [64, 64, 64, 128, 2048, 4096]


def test_records_reference_agrees_with_the_hand_built_views_of_the_record_tests(synth):
    """the scene of tests/test_gpu_kfproj_store.py::test_reloc_projection_on_records with its ids, bad flags and claimed array built by hand as that test builds them"""
    seed, n = 5312, 500
    rng = np.random.default_rng(seed)
    sc = synth.keyframe_scene(seed, n=n, span=1.0)
    pts = sc["pts1"]; has = pts["valid"] != 0
    cause = rng.integers(0, 3, n)
    ids1 = np.where(has | (cause != 0), np.uint64(1000) + np.arange(n, dtype=np.uint64), R.NONE)
    bad1 = ~has & (cause == 1); found = np.nonzero(~has & (cause == 2))[0]
    claimed = sc["claimed2"] != 0
    ids2 = np.where(claimed, np.uint64(700000) + np.arange(n, dtype=np.uint64), R.NONE)
    ci = np.nonzero(claimed)[0]; ids2[ci[: len(found)]] = np.uint64(1000) + found.astype(np.uint64)
    rec = np.zeros(n, R.MP_RECORD_DTYPE); rec["id"] = 1000 + np.arange(n); rec["descriptor"] = sc["desc1"]; rec["world_pos"] = pts["world"]; rec["normal"] = pts["normal"]
    rec["min_distance"] = pts["min_distance"]; rec["max_distance"] = pts["max_distance"]; rec["flags"] = np.where(bad1, R.MP_BAD, 0); rec["n_obs"] = 1
    v, d, cl = R.reloc_view(sc["kf1"]["keys_un"], ids1, ids2, np.zeros(n, np.uint8), rec, R.slot_dict(rec))
    assert np.array_equal(cl, sc["claimed2"]) and np.array_equal(v["valid"], pts["valid"])
    ok = has
    for k in ("world", "normal", "min_distance", "max_distance", "angle"):
        assert np.array_equal(v[k][ok], pts[k][ok]), k
    assert np.array_equal(d[ok], sc["desc1"][ok])
    # test_search_by_sim3_on_records' second round: a third of some pairs enter as matched, KF2's side through the observation (22, i) of KF2's point i
    lists = [[(11, i)] for i in range(n)] + [[(22, i)] for i in range(n)]
    rec2 = np.concatenate([rec, rec]); rec2["id"][n:] = 500000 + np.arange(n); rec2["flags"] = 0
    i1 = np.uint64(1000) + np.arange(n, dtype=np.uint64); i2 = np.uint64(500000) + np.arange(n, dtype=np.uint64)
    pre = np.arange(0, n, 7); to = (pre * 3) % n
    matched = np.full(n, R.NONE, np.uint64); matched[pre] = i2[to]
    (v1, _), (v2, _) = R.sim3_views(i1, i2, matched, rec2, R.slot_dict(rec2), lists, 22)
    w1 = np.ones(n, bool); w1[pre] = False; w2 = np.ones(n, bool); w2[to] = False
    assert np.array_equal(v1["valid"].astype(bool), w1) and np.array_equal(v2["valid"].astype(bool), w2)


def test_pointer_level_rules_on_hand_checked_examples():
    rec = np.zeros(4, R.MP_RECORD_DTYPE); rec["id"] = [10, 20, 30, 40]; rec["n_obs"] = [1, 0, 1, 1]; rec["flags"] = [0, 0, R.MP_BAD, 0]
    rec["world_pos"] = np.arange(12).reshape(4, 3); rec["descriptor"] = np.arange(4)[:, None] + 1
    so = R.slot_dict(rec)
    keys = np.zeros(4, R.KP_DTYPE); keys["angle"] = [1, 2, 3, 4]; keys["octave"] = [0, 1, 2, 3]; keys["x"] = [5, 6, 7, 8]
    U = np.uint64
    # last frame: a good point; an outlier; a bad point; an id nobody knows.  Current frame: holds the unobserved point 20 (not claimed), 10 discarded, 40, nothing
    lastp, ld, cl = R.last_frame_view(keys, [U(10), U(40), U(30), U(99)], [0, R.OUTLIER, 0, 0], [U(20), U(10), U(40), R.NONE], [0, R.DISCARDED, R.OUTLIER, 0], rec, so)
    assert lastp["valid"].tolist() == [1, 0, 0, 0] and lastp["claims"].tolist() == [1, 0, 0, 0] and lastp["world"][0].tolist() == [0, 1, 2] and not lastp["world"][1:].any()
    assert ld[0, 0] == 1 and not ld[1:].any() and cl.tolist() == [0, 0, 1, 0] and lastp["octave"].tolist() == [0, 1, 2, 3]
    ids, fl = R.matched_writes([U(20), U(10), U(40), R.NONE], [0, R.DISCARDED, R.OUTLIER, 0], [-1, 0, -1, 3], [U(10), U(40), U(30), U(99)])
    assert ids.tolist() == [20, 10, 40, 99] and fl.tolist() == [0, 0, R.OUTLIER, 0]
    # pose edges: held and outlier-marked points carry an edge, in index order; discarded, bad and unknown ones do not
    e = R.pose_edges(keys, np.array([-1, 3, -1, 2], np.float32), [U(40), U(10), U(30), U(10)], [R.OUTLIER, 0, 0, R.DISCARDED], rec, so, np.array([1, .5, .25, .125], np.float32))
    assert e["feat"].tolist() == [0, 1] and e["mono"].tolist() == [True, False] and e["w"].tolist() == [1, .5] and e["points"].tolist() == [[9, 10, 11], [0, 1, 2]] and e["klass"] == 0
    assert e["obs"].tolist() == [[5, 0, -1], [6, 0, 3]]
    assert R.pose_writes([R.OUTLIER, 0, R.OUTLIER | R.DISCARDED, 1], [0, 1], [False, True], False).tolist() == [0, R.OUTLIER, R.DISCARDED, 1]
    assert R.pose_writes([R.OUTLIER, 0, R.OUTLIER | R.DISCARDED, 1], [0, 1], [False, True], True).tolist() == [0, R.DISCARDED, R.DISCARDED, 1]
    # SearchLocalPoints: the bad point 30 leaves the frame; 10 (held) and 40 (discarded) are seen; candidates: 20 only (30 bad, 99 unknown)
    after, cand, cl = R.local_points_view([U(10), U(30), U(40), R.NONE], [0, 0, R.DISCARDED, 0], [U(40), U(20), U(30), U(99), U(10)], rec, so)
    assert after.tolist() == [10, R.NO_MAP_POINT, 40, R.NO_MAP_POINT] and cand.tolist() == [False, True, False, False, False] and cl.tolist() == [1, 0, 0, 0]
    # relocalisation: the frame holds 20 and the unknown 99 (both claimed), 10 only discarded; pKF's points 10 (candidate), 20 (already found), 30 (bad), none
    v, d, cl = R.reloc_view(keys, [U(10), U(20), U(30), R.NONE], [U(20), U(99), U(10), R.NONE], [0, 0, R.DISCARDED, 0], rec, so)
    assert v["valid"].tolist() == [1, 0, 0, 0] and v["angle"].tolist() == [1, 0, 0, 0] and cl.tolist() == [1, 1, 0, 0] and d[0, 0] == 1
    # Scw: vpMatched holds 20 and an unknown id; vpPoints in the order 40, 30, 20, 10
    v, d, cl = R.scw_view([R.NONE, U(20), U(99)], [3, 2, 1, 0], rec)
    assert v["valid"].tolist() == [1, 0, 0, 1] and cl.tolist() == [0, 1, 1] and d[:, 0].tolist() == [4, 0, 0, 1]
    # Sim3: feature 0 of KF1 enters matched to point 40, which KF2 (id 7) sees at feature 2; feature 1 to point 10, seen at feature 9 >= N2; GetIndexInKeyFrame
    lists = [[(3, 0), (7, 9)], [(7, 1)], [(7, 0)], [(3, 1), (5, 0), (7, 2)]]
    assert [R.index_in_keyframe(l, 7) for l in lists] == [9, 1, 0, 2] and R.index_in_keyframe(lists[1], 3) == -1
    (v1, _), (v2, _) = R.sim3_views([U(10), U(20), U(30)], [U(30), U(20), U(40)], [U(40), U(10), R.NONE], rec, so, lists, 7)
    assert v1["valid"].tolist() == [0, 0, 0] and v2["valid"].tolist() == [0, 1, 0]
    (v1, _), (v2, _) = R.sim3_views([U(10), U(20), U(30)], [U(30), U(20), U(40)], None, rec, so, lists, 7)
    assert v1["valid"].tolist() == [1, 1, 0] and v2["valid"].tolist() == [0, 1, 1]
    # Fuse: 10 is seen by keyframe 7 already, 30 is bad; the fused points 20 and 40 meet an empty feature and a held one
    v, d = R.fuse_view([0, 1, 2, 3], rec, [[(3, 0), (7, 9)], [(9, 1)], [], [(3, 1)]], 7)
    assert v["valid"].tolist() == [0, 1, 0, 1]
    mp, act, out = R.fuse_writes([-1, 2, -1, 2], [R.NONE, U(5), R.NONE], [10, 20, 30, 40], [[(3, 0), (7, 9)], [(9, 1)], [], [(3, 1)]], 7)
    assert mp.tolist() == [R.NO_MAP_POINT, 5, 20] and act.tolist() == [0, 1, 0, 2] and out[1] == [(7, 2), (9, 1)] and out[3] == [(3, 1)]

"""GPU parity on seeded random problems across the bundle adjustment's route boundaries: GlobalBundleAdjustemnt against pyorc.ba_solve, PoseOptimization,
local windows and custom stage lists against pyorc.ba_solve_staged.  Every case is drawn from its own numpy seed and is its own parametrize id, and every
case asserts that the route it was built for is the route that ran (corb_ba.cpp: the fused one-workgroup optimiser up to BA_SMALL_SP / BA_SMALL_EDGES,
the in-LDS dense solve up to a 128-row reduced system, the blocked dense Cholesky, PCG with the row-owner Schur kernel from BA_ROW_MIN_POSES free poses,
the coarse levels from BA_ML_AUTO_POSES; the fused single-pose kernel; the device route of a staged window).  tests/test_random_cases.py checks on the
CPU that the case lists are deterministic and reach both sides of every boundary."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-4

# route buckets of GlobalBundleAdjustemnt (what CorbBAResult reports: solver_used, nnz_blocks = 0 without a block pattern, pc_levels)
FUSED, LDS, DENSE, PCG, PCG_ROW, PCG_ML = "fused", "lds", "dense", "pcg", "pcg-row", "pcg-ml"


def _ba(i, solver, free, clients=1, ppk=8, window=4, edges=None, fix_kf=False, robust=None, ml=0, devflat=False, route=None):
    return dict(i=i, seed=41000 + i, solver=solver, free=free, clients=clients, ppk=ppk, window=window, edges=edges, fix_kf=fix_kf,
                robust=bool(i & 1) if robust is None else robust, ml=ml, devflat=devflat, route=route)


# free poses and edge counts on both sides of every boundary: 15 / 16 / 17 and 2047 / 2048 / 2049 (fused), 21 / 22 (in-LDS dense), 63 / 64 (row Schur),
# 256 / 257 (dense vs PCG and the coarse levels of the automatic choice)
BA_CASES = [
    _ba(0, 0, 15, fix_kf=True, ppk=40, window=6, edges=2047, route=FUSED),
    _ba(1, 0, 16, ppk=40, window=6, edges=2048, route=FUSED),
    _ba(2, 0, 16, ppk=40, window=6, edges=2049, route=LDS),
    _ba(3, 0, 15, clients=4, ppk=8, route=FUSED),
    _ba(4, 0, 17, clients=2, ppk=10, route=LDS),
    _ba(5, 1, 16, ppk=12, route=LDS),
    _ba(6, 0, 21, clients=2, ppk=10, devflat=True, route=LDS),
    _ba(7, 0, 22, ppk=10, route=DENSE),
    _ba(8, 1, 22, clients=3, fix_kf=True, ppk=8, route=DENSE),
    _ba(9, 2, 16, ppk=10, route=PCG),
    _ba(10, 2, 63, ppk=6, route=PCG),
    _ba(11, 2, 64, clients=5, ppk=6, route=PCG_ROW),
    _ba(12, 2, 64, clients=6, fix_kf=True, ppk=6, ml=1, route=PCG_ROW),
    _ba(13, 1, 63, clients=4, ppk=6, devflat=True, route=DENSE),
    _ba(14, 2, 64, ppk=6, route=PCG_ROW),
    _ba(15, 0, 256, ppk=5, route=DENSE),
    _ba(16, 0, 257, ppk=5, route=PCG_ML),
    _ba(17, 2, 256, clients=2, fix_kf=True, ppk=5, route=PCG_ML),
    _ba(18, 2, 255, clients=4, ppk=5, route=PCG_ROW),
    _ba(19, 2, 257, ppk=5, ml=1, route=PCG_ROW),
    _ba(20, 0, 257, clients=6, ppk=5, devflat=True, route=PCG_ML),
]


def ba_case_id(c):
    return "ba-%03d-solver%d-free%d%s-%s%s%s" % (c["i"], c["solver"], c["free"], "-e%d" % c["edges"] if c["edges"] else "", "robust" if c["robust"] else "plain",
                                               "-ml%d" % c["ml"] if c["ml"] else "", "-devflat" if c["devflat"] else "")


def active_edges(p):
    e = p["edges"]
    return int((~((p["pose_fixed"][e["pose"]] != 0) & (p["point_fixed"][e["point"]] != 0))).sum())


def thin_edges(edges, keep_active, target, rng):
    """drop observations until `target` of the edges with keep_active[i] remain, the rest in the generator's order: single observations of points that keep
    at least two, or both observations of a point that has two (it leaves the problem)"""
    e = edges
    alive = np.ones(len(e), bool)
    cnt = np.bincount(e["point"], minlength=int(e["point"].max()) + 1)
    n = int(keep_active.sum())
    assert n >= target, (n, target)
    for i in rng.permutation(len(e)):
        if n == target:
            break
        j = e["point"][i]
        if not alive[i] or not keep_active[i]:
            continue
        if cnt[j] > 2:
            alive[i] = False; cnt[j] -= 1; n -= 1
        elif cnt[j] == 2 and n - target >= 2:
            both = np.nonzero((e["point"] == j) & alive)[0]
            if keep_active[both].all():
                alive[both] = False; cnt[j] = 0; n -= 2
    assert n == target
    return e[alive]


def ba_case_problem(synth, c):
    rng = np.random.default_rng(c["seed"])
    K = c["free"] + 1 + (1 if c["fix_kf"] else 0)
    assert K % c["clients"] == 0, c
    p = synth.ba_problem(n_clients=c["clients"], kf_per_client=K // c["clients"], pts_per_kf=c["ppk"], seed=c["seed"], window=c["window"])
    nfix = int(rng.integers(0, 4))
    if nfix:
        p["point_fixed"][rng.choice(len(p["points"]), size=nfix, replace=False)] = 1
    if c["fix_kf"]:
        p["pose_fixed"][int(rng.integers(1, K))] = 1
    if c["edges"]:
        e = p["edges"]
        p["edges"] = thin_edges(e, ~((p["pose_fixed"][e["pose"]] != 0) & (p["point_fixed"][e["point"]] != 0)), c["edges"], rng)
    return p


def _args(p, edges=None, points=None, point_fixed=None):
    return (p["poses"], p["pose_fixed"], p["points"] if points is None else points, p["point_fixed"] if point_fixed is None else point_fixed,
            p["edges"] if edges is None else edges, p["fx"], p["fy"], p["cx"], p["cy"], p["bf"])


def _near(g, r):
    """the estimates' bars of tests/test_gpu_ba.py::_check: rotations at 1e-4 absolute, translations and points at 1e-4 relative"""
    gp, rp = np.asarray(g["poses"]).reshape(-1, 4, 4), np.asarray(r["poses"]).reshape(-1, 4, 4)
    return (np.abs(gp[:, :3, :3] - rp[:, :3, :3]).max() <= RTOL and
            np.abs(gp[:, :3, 3] - rp[:, :3, 3]).max() <= RTOL * max(1.0, np.abs(rp[:, :3, 3]).max()) and
            np.abs(g["points"] - r["points"]).max() <= RTOL * max(1.0, np.abs(r["points"]).max()))


def _route(g):
    """the bucket of a result.  What the result itself tells apart: the solver, the fused optimiser (no block pattern: nnz_blocks = 0) and the coarse levels
    (pc_levels > 0).  The in-LDS solve vs the blocked dense Cholesky and the row-owner Schur kernel vs the plain PCG build are not reported in CorbBAResult: those
    splits follow the reported free_poses (checked against the case's) at the sizes ba_lm.cpp keys them on, 6 free_poses <= 128 and BA_ROW_MIN_POSES"""
    s = g["structure"]
    if g["solver"] == 1:
        return FUSED if s["nnz_blocks"] == 0 else LDS if 6 * s["free_poses"] <= 128 else DENSE
    if g["solver"] == 2:
        return PCG_ML if s["pc_levels"] > 0 else PCG_ROW if s["free_poses"] >= 64 else PCG
    return "solver%d" % g["solver"]


# ba-014 (seed 41014; solver 2, 64 free keyframes in one loop, non-robust): 17 LM trials against the oracle's 10.  The default PCG tolerance of a map below the forcing
# policy's size is a 1e-8 residual; on this ill-conditioned reduced system that step moves the ninth iteration's rho across the steep part of the lambda schedule (lambda
# 1.96e-2 against 2.94e-2) without the policy's doubt tests firing, and the tenth iteration then rejects 7 trials.  The same call with pcg_tol 1e-10 or 1e-13 gives
# 10 trials and the oracle's lambdas; the dense solver gives the oracle's bits.  Solving such maps to 1e-12 by default fixes this case but moves the plateau
# decisions of test_gpu_ba.py::test_rejected_trials_match_oracle[1.0-12-2] outside its point bar, so the tolerance policy is left as it is here.  Open.
BA_OPEN = {14: "PCG at the default 1e-8 tolerance: the ninth iteration's lambda and the tenth iteration's trials differ from the exact solve's (open)"}


@pytest.mark.parametrize("c", [pytest.param(c, id=ba_case_id(c), marks=pytest.mark.xfail(strict=True, reason=BA_OPEN[c["i"]])) if c["i"] in BA_OPEN else
                               pytest.param(c, id=ba_case_id(c)) for c in BA_CASES])
def test_global_ba_random_case(corb, pyorc, synth, c):
    p = ba_case_problem(synth, c)
    g = corb.Optimizer.GlobalBundleAdjustemnt(*_args(p), nIterations=10, bRobust=c["robust"], solver=c["solver"], pc_multilevel=c["ml"], devflat=c["devflat"])
    assert _route(g) == c["route"], g["structure"]
    assert g["structure"]["free_poses"] == c["free"]
    if c["edges"]:
        assert g["structure"]["active_edges"] == c["edges"]
    r = pyorc.ba_solve(*_args(p), iters=10, robust=c["robust"])
    assert g["iters_done"] == r["iters_done"] and g["trials"] == r["trials"], (g["iters_done"], r["iters_done"], g["trials"], r["trials"])
    assert np.allclose(g["chi2"], r["chi2"], rtol=RTOL), (g["chi2"], r["chi2"])
    assert _near(g, r)


# ---- PoseOptimization: sizes at wave (64) and workgroup (256 / 512) edges and on both sides of the register-resident limit (2 048); solver 0 = the fused
# single-pose kernel, 1 = the general staged path
POSE_SIZES = [60, 63, 64, 65, 255, 256, 257, 511, 512, 2049, 3000]
POSE_CASES = [dict(i=i, seed=43000 + i, n=n, solver=0) for i, n in enumerate(POSE_SIZES)] + \
             [dict(i=len(POSE_SIZES) + j, seed=43000 + len(POSE_SIZES) + j, n=n, solver=1) for j, n in enumerate([60, 64, 65, 256, 512, 2049, 3000])]


def pose_case_id(c):
    return "pose-%03d-solver%d-n%d" % (c["i"], c["solver"], c["n"])


def pose_case_problem(synth, c):
    rng = np.random.default_rng(c["seed"])
    return synth.pose_opt_problem(seed=c["seed"], n=c["n"], outlier_frac=float(rng.uniform(0.05, 0.3)))


def pose_edges(pyorc, q):
    n = len(q["points"])
    e = np.zeros(n, pyorc.EDGE_DTYPE)
    e["pose"] = 0; e["point"] = np.arange(n); e["u"] = q["obs"][:, 0]; e["v"] = q["obs"][:, 1]; e["ur"] = q["obs"][:, 2]; e["inv_sigma2"] = q["inv_sigma2"]
    return e


@pytest.mark.parametrize("c", POSE_CASES, ids=[pose_case_id(c) for c in POSE_CASES])
def test_pose_optimization_random_case(corb, pyorc, synth, c):
    q = pose_case_problem(synth, c)
    n = c["n"]
    a = (q["Tcw0"].reshape(1, 16), np.zeros(1, np.uint8), q["points"], np.ones(n, np.uint8), pose_edges(pyorc, q), q["fx"], q["fy"], q["cx"], q["cy"], q["bf"])
    g = corb.Optimizer._staged(corb.POSE_OPT_STAGES, *a, solver=c["solver"])          # (what Optimizer.PoseOptimization calls, with the route it took)
    assert (g["solver"] == 3) == (c["solver"] == 0), g["solver"]
    r = pyorc.ba_solve_staged(*a, pyorc.POSE_OPT_STAGES)
    assert np.array_equal(g["outlier"], r["outlier"]), int((g["outlier"] != r["outlier"]).sum())
    assert r["outlier"].sum() > 0
    assert np.abs(g["poses"][0] - r["poses"][0]).max() <= RTOL * max(1.0, np.abs(r["poses"][0]).max())
    T, outl, ninl = corb.Optimizer.PoseOptimization(q["Tcw0"], q["points"], q["obs"], q["inv_sigma2"], q["fx"], q["fy"], q["cx"], q["cy"], q["bf"], solver=c["solver"])
    assert np.array_equal(T, g["poses"][0]) and np.array_equal(outl, g["outlier"].astype(bool)) and ninl == n - int(r["outlier"].sum())


# ---- local windows on both sides of E = 2 048: grouped by point (the device route above it) and the same window with one point's edges moved to the end (host route)
# edges: the window's edge count (raw) or its count without the edges between a fixed keyframe and a fixed point (active: what the fused optimiser's
# BA_SMALL_EDGES limit sees)
WINDOW_CASES = [dict(i=0, seed=44000, n_local=6, n_fixed=4, ppk=120, edges=2047, count="raw"),
                dict(i=1, seed=44001, n_local=6, n_fixed=4, ppk=120, edges=2048, count="raw"),
                dict(i=2, seed=44002, n_local=6, n_fixed=4, ppk=120, edges=2049, count="active"),
                dict(i=3, seed=44003, n_local=8, n_fixed=3, ppk=110, edges=2050, count="active"),
                dict(i=4, seed=44004, n_local=12, n_fixed=6, ppk=90, edges=None, count="raw"),
                dict(i=5, seed=44005, n_local=4, n_fixed=0, ppk=160, edges=None, count="raw"),
                dict(i=6, seed=44006, n_local=24, n_fixed=2, ppk=40, edges=None, count="raw"),
                dict(i=7, seed=44007, n_local=10, n_fixed=5, ppk=30, edges=None, count="raw")]


def window_case_problem(synth, c):
    rng = np.random.default_rng(c["seed"])
    p = synth.local_ba_problem(seed=c["seed"], n_local=c["n_local"], n_fixed=c["n_fixed"], pts_per_kf=c["ppk"], outlier_frac=float(rng.uniform(0.04, 0.14)))
    pf = p["point_fixed"]; pf[rng.random(len(pf)) < rng.uniform(0.0, 0.06)] = 1
    if c["edges"]:
        e = p["edges"]
        keep = np.ones(len(e), bool) if c["count"] == "raw" else ~((p["pose_fixed"][e["pose"]] != 0) & (pf[e["point"]] != 0))
        p["edges"] = thin_edges(e, keep, c["edges"], rng)
    return p


def window_expects_device(p):
    """corb_ba_staged.cpp: ba_staged_window_host takes a window grouped by point with more than BA_SMALL_EDGES edges and 1 .. 64 free keyframes, and declines one
    that the fused one-workgroup optimiser takes (at most 16 free keyframes and BA_SMALL_EDGES active edges)"""
    e = p["edges"]
    free = int((p["pose_fixed"] == 0).sum())
    fused = 6 * free <= 96 and active_edges(p) <= 2048
    return bool(np.all(np.diff(e["point"]) >= 0)) and len(e) > 2048 and 1 <= free <= 64 and not fused


def moved_order(e):
    moved = e["point"] == e["point"][len(e) // 2]
    return np.r_[np.nonzero(~moved)[0], np.nonzero(moved)[0]]


def window_case_id(c):
    return "window-%03d-local%d-fixed%d-%s" % (c["i"], c["n_local"], c["n_fixed"], "%s%d" % ("e" if c["count"] == "raw" else "active", c["edges"]) if c["edges"] else "ppk%d" % c["ppk"])


def _staged_pair(corb, pyorc, stages, a, order, expect_device, bit_equal=True):
    """the grouped window and the moved one through corb_ba_solve_staged, both against the oracle; the two routes bit for bit when the grouped one took the device"""
    e = a[4]
    g = corb.Optimizer._staged(stages, *a)
    h = corb.Optimizer._staged(stages, *(a[:4] + (e[order],) + a[5:]))
    assert g["device_route"] == expect_device and not h["device_route"]
    r = pyorc.ba_solve_staged(*a, stages)
    for x, outl in ((g, r["outlier"]), (h, r["outlier"][order])):
        assert x["iters_done"] == r["iters_done"] and x["trials"] == r["trials"], (x["iters_done"], r["iters_done"], x["trials"], r["trials"])
        assert np.array_equal(x["outlier"], outl), int((x["outlier"] != outl).sum())
        assert _near(x, r)
    if expect_device and bit_equal:
        assert np.array_equal(g["poses"], h["poses"]) and np.array_equal(g["points"], h["points"]) and np.array_equal(g["outlier"][order], h["outlier"])
    return g, r


# window-006 (seed 44006, 24 local keyframes: 23 free, the blocked dense solve): both routes match the oracle (flags, counts, estimates), but their estimates differ in the
# last bits.  The difference appears only beyond ~10 LM iterations of one optimize() -- one stage of 15 iterations differs, 10 robust iterations or 5 + 2 stay
# bit-equal, and it does not depend on the classification (no edge removed: still different) or on fixed points -- while the 29-free-keyframe window of
# test_gpu_staged.py stays bit-equal through 15.  Open: pinned as a strict xfail so that it fails loudly once the routes agree again.
# Its oracle comparison runs with the others; the bit-for-bit comparison of its two routes is the strict xfail below.
# Recorded with tests/test_gpu_ba_switches.py: CORB_BA_NO_CHAIN=1, CORB_BA_CHAIN=1 and CORB_BA_HOST_STAGES=1 change no byte of either route and none makes them agree (poses
# differ by 9.3e-10, points by 1.9e-9); the chains are not on this window's path (6 * 23 > 128 rows).  What does separate the routes: ba_schur_mfma_launch takes the split form
# of the Schur kernel up to BA_SMALL_SPLIT_MAX_UNITS = 128 units, the device window lays out the full pattern (23 * 24 / 2 = 276 units: one wavefront per block), the host
# flattening the 126 blocks with a shared map point (16 wavefronts per block) -- another summation order.  With the split form compiled out, in an experiment, the two routes of
# this window are bit-equal; a 16-keyframe window (seed 44008) then still differs, so the kernel's form is not the only cause among windows of this size.
WINDOW_OPEN = {6: "device and host routes of a 23-free-keyframe window differ in the last bits beyond ~10 LM iterations (open)"}


@pytest.mark.parametrize("c", WINDOW_CASES, ids=[window_case_id(c) for c in WINDOW_CASES])
def test_local_window_random_case(corb, pyorc, synth, c):
    p = window_case_problem(synth, c)
    g, r = _staged_pair(corb, pyorc, corb.LOCAL_BA_STAGES, _args(p), moved_order(p["edges"]), window_expects_device(p), bit_equal=c["i"] not in WINDOW_OPEN)
    assert r["outlier"].sum() > 0


@pytest.mark.xfail(strict=True, reason=WINDOW_OPEN[6])
@pytest.mark.parametrize("c", [c for c in WINDOW_CASES if c["i"] in WINDOW_OPEN], ids=[window_case_id(c) for c in WINDOW_CASES if c["i"] in WINDOW_OPEN])
def test_local_window_routes_bit_equal_open(corb, synth, c):
    p = window_case_problem(synth, c)
    e = p["edges"]; order = moved_order(e)
    g = corb.Optimizer._staged(corb.LOCAL_BA_STAGES, *_args(p))
    h = corb.Optimizer._staged(corb.LOCAL_BA_STAGES, *_args(p, edges=e[order]))
    assert g["device_route"] and not h["device_route"]
    assert np.array_equal(g["poses"], h["poses"]) and np.array_equal(g["points"], h["points"]) and np.array_equal(g["outlier"][order], h["outlier"])


# ---- custom stage lists of 1 .. 15 stages (corb_ba_staged_device_wanted admits up to 15) on a window with a fixed point behind a fixed camera that observes it
STAGE_COUNTS = [1, 4, 8, 9, 12, 15]
STAGE_CASES = [dict(i=i, seed=45000 + i, n_stages=n, late_depth=False) for i, n in enumerate(STAGE_COUNTS)] + \
              [dict(i=len(STAGE_COUNTS) + j, seed=45000 + len(STAGE_COUNTS) + j, n_stages=n, late_depth=True) for j, n in enumerate([9, 15])]


def stage_case_id(c):
    return "stages-%03d-n%d%s" % (c["i"], c["n_stages"], "-depth-after-8" if c["late_depth"] else "")


def stage_list(c):
    """random stages (Optimizer.cc's stage fields); reset_estimates only on the first stage is never set, so that the device route stays eligible.
    late_depth: the first 8 stages skip the depth test and every later one applies it, so only stages 9+ can flag the edge behind the fixed camera"""
    rng = np.random.default_rng(c["seed"])
    st = []
    for k in range(c["n_stages"]):
        cm = float(np.float32(rng.uniform(3.0, 9.0))); cs = float(np.float32(rng.uniform(5.0, 12.0)))
        depth = (k >= 8) if c["late_depth"] else int(rng.random() < 0.6)
        st.append((int(rng.integers(1, 5)), int(rng.random() < 0.5), cm, cs, int(depth), 0, int(rng.random() < 0.5), 0, 0,
                   float(np.float32(np.sqrt(cm))), float(np.float32(np.sqrt(cs)))))
    return st


def stage_case_problem(synth, c):
    """the window of test_gpu_staged.py's fixed-point test: fixed map points, and one of them moved behind a fixed camera that observes it.
    Returns (problem, point_fixed, points, index of that observation)"""
    p = synth.local_ba_problem(seed=c["seed"], n_local=7, n_fixed=4, pts_per_kf=120, outlier_frac=0.08)
    rng = np.random.default_rng(c["seed"])
    e = p["edges"]
    point_fixed = p["point_fixed"].copy(); point_fixed[rng.random(len(point_fixed)) < 0.05] = 1
    ff = np.nonzero((p["pose_fixed"][e["pose"]] != 0) & (point_fixed[e["point"]] != 0))[0]
    assert len(ff) > 0
    j, k = int(e["point"][ff[0]]), int(e["pose"][ff[0]])
    pts = p["points"].copy(); T = p["poses"][k].reshape(4, 4).astype(np.float64)
    pts[j] = (T[:3, :3].T @ (np.array([0.3, -0.2, -4.0]) - T[:3, 3])).astype(np.float32)
    return p, point_fixed, pts, int(ff[0])


def stage_flags_behind(stages, e_idx, r):
    """what the staged classification must leave on the edge behind the fixed camera (chi2 0, depth < 0): replayed stage by stage"""
    active = 1
    for s in stages:
        if not active and not s[6]:
            continue
        active = 0 if s[4] else 1
    return 1 - active


@pytest.mark.parametrize("c", STAGE_CASES, ids=[stage_case_id(c) for c in STAGE_CASES])
def test_custom_stage_list_random_case(corb, pyorc, synth, c):
    p, point_fixed, pts, ff = stage_case_problem(synth, c)
    stages = stage_list(c)
    a = _args(p, points=pts, point_fixed=point_fixed)
    g, r = _staged_pair(corb, pyorc, stages, a, moved_order(p["edges"]), True)
    assert g["outlier"][ff] == r["outlier"][ff] == stage_flags_behind(stages, ff, r)
    if c["late_depth"]:
        assert r["outlier"][ff] == 1


def _store_window(corb, synth, c):
    """the stage-list case's window as store records (tests/test_gpu_local_ba_store.py's construction) with the same fixed point behind a fixed camera"""
    from test_gpu_local_ba_store import _build, _objects
    n_local = 7
    prob, cm, KF, MP = _build(corb, synth, c["seed"], n_local=n_local, n_fixed=4, ppk=120, outlier_frac=0.08)
    K, M = len(cm["kf"]), len(cm["mp_records"])
    off = cm["obs_off"]
    kf_ids = [int(k["id"]) for k in cm["kf"]]
    j, s = next((j, kf_ids.index(int(cm["obs_kf"][t]))) for j in range(M) for t in range(off[j], off[j + 1]) if kf_ids.index(int(cm["obs_kf"][t])) >= n_local)
    rec, _, _ = MP.get(0, M)
    rec["flags"][j] |= corb.MP_FIXED
    T = cm["kf"][s]["Tcw"].reshape(4, 4).astype(np.float64)
    rec["world_pos"][j] = (T[:3, :3].T @ (np.array([0.3, -0.2, -4.0]) - T[:3, 3])).astype(np.float32)
    MP.put(0, rec, cm["obs_off"], cm["obs_kf"], cm["obs_idx"])
    cm["mp_records"] = rec
    kfs, mps = _objects(cm)
    return KF, MP, kfs, mps, n_local, (s, j)


@pytest.mark.parametrize("c", [c for c in STAGE_CASES if c["n_stages"] in (4, 9, 15)], ids=[stage_case_id(c) for c in STAGE_CASES if c["n_stages"] in (4, 9, 15)])
def test_local_ba_store_custom_stage_list(corb, pyorc, synth, c):
    """the same stage lists through LocalBundleAdjustmentStore: the device route's classification of the window's edges, the erased observations as the oracle's"""
    KF, MP, kfs, mps, n_local, behind = _store_window(corb, synth, c)
    stages = stage_list(c)
    o = pyorc.local_bundle_adjustment(kfs[:n_local], kfs[n_local:], mps, scale_factor=1.2, stages=stages)
    g = corb.LocalBundleAdjustmentStore(KF, np.arange(len(kfs)), n_local, MP, np.arange(len(mps)), scale_factor=1.2, stages=stages)
    assert g["device_route"]
    assert sorted(map(tuple, g["erase"].tolist())) == sorted(o["erase"])
    assert _near(g, o)
    ff = next(i for i, (kid, j) in enumerate(zip(o["edges"]["pose"], o["edges"]["point"])) if (kid, j) == behind)
    assert (behind in set(map(tuple, g["erase"].tolist()))) == bool(stage_flags_behind(stages, ff, o))
    if c["late_depth"]:
        assert behind in set(map(tuple, g["erase"].tolist()))
    KF.close(); MP.close()

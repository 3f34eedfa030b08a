"""GPU parity tests for global bundle adjustment: chi2 per LM iteration, poses and landmarks within
1e-4 relative of the CPU oracle (BASELINE.json north_star tolerance; FP64 inside, FP32 at the boundary)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-4
PCG_LOOSE = 1e-6          # ba_host.h: BA_PCG_TOL_LOOSE, the cap of the default policy's forcing sequence (the certificate of a call stays within 10x of it)


def _args(prob):
    return (prob["poses"], prob["pose_fixed"], prob["points"], prob["point_fixed"], prob["edges"], prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"])


def _run_both(corb, pyorc, prob, iters, robust, solver=1, pc_block=0, intr=None, pcg_tol=0.0):
    g = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=iters, bRobust=robust, solver=solver, pc_block=pc_block, intr=intr, pcg_tol=pcg_tol)
    r = pyorc.ba_solve(*_args(prob), iters=iters, robust=robust, intr=intr)
    return g, r


def test_warmup(corb):
    """corb_warmup: creates the per-device workspace lanes (the library links no rocBLAS / rocSOLVER any more); idempotent"""
    corb.warmup(0)
    corb.warmup(0)


def _check(g, r):
    assert g["iters_done"] == r["iters_done"] and g["trials"] == r["trials"]
    assert np.allclose(g["chi2"], r["chi2"], rtol=RTOL), (g["chi2"], r["chi2"])
    assert np.allclose(g["lam"], r["lam"], rtol=1e-3)
    scale_t = max(1.0, np.abs(r["poses"][:, :3, 3]).max())
    assert np.abs(g["poses"][:, :3, 3] - r["poses"][:, :3, 3]).max() <= RTOL * scale_t
    assert np.abs(g["poses"][:, :3, :3] - r["poses"][:, :3, :3]).max() <= RTOL
    scale_p = max(1.0, np.abs(r["points"]).max())
    assert np.abs(g["points"] - r["points"]).max() <= RTOL * scale_p


@pytest.mark.parametrize("robust", [False, True])
def test_small_mixed_problem(corb, pyorc, synth, robust):
    prob = synth.ba_problem(n_clients=2, kf_per_client=4, pts_per_kf=6, seed=1001, window=2)
    prob["point_fixed"][3] = 1
    g, r = _run_both(corb, pyorc, prob, 10, robust)
    _check(g, r)
    assert np.array_equal(g["poses"][0], prob["poses"][0]) and np.array_equal(g["points"][3], prob["points"][3])


@pytest.mark.parametrize("cfg", [dict(n_clients=1, kf_per_client=12, pts_per_kf=20, seed=1003),
                                 dict(n_clients=4, kf_per_client=25, pts_per_kf=30, seed=1004),
                                 dict(n_clients=8, kf_per_client=20, pts_per_kf=40, seed=1005, max_obs=16, window=10)])
def test_server_setting_10_iterations_nonrobust(corb, pyorc, synth, cfg):
    """corbslam_server/src/GlobalOptimize.cpp:444: GlobalBundleAdjustemnt(cache, 10, &stop, nLoopKF, false)"""
    prob = synth.ba_problem(**cfg)
    g, r = _run_both(corb, pyorc, prob, 10, False)
    _check(g, r)
    assert g["chi2"][-1] < 0.25 * g["chi2"][0]


def test_edge_cases(corb, pyorc, synth):
    prob = synth.ba_problem(n_clients=1, kf_per_client=6, pts_per_kf=8, seed=1006)
    # zero iterations: estimates come back converted float->double->float (identity on fixed, ~1e-7 on free)
    g, r = _run_both(corb, pyorc, prob, 0, False)
    assert g["iters_done"] == 0 and np.allclose(g["poses"], r["poses"], atol=1e-6) and np.allclose(g["points"], prob["points"])
    # every pose fixed: pure landmark refinement (structure-only), reduced system is empty
    prob2 = dict(prob); prob2["pose_fixed"] = np.ones_like(prob["pose_fixed"])
    g, r = _run_both(corb, pyorc, prob2, 5, False)
    _check(g, r)
    assert np.array_equal(g["poses"], prob["poses"])
    # every landmark fixed: pose-only refinement, no Schur terms
    prob3 = dict(prob); prob3["point_fixed"] = np.ones_like(prob["point_fixed"])
    g, r = _run_both(corb, pyorc, prob3, 5, True)
    _check(g, r)
    # no edges at all
    prob4 = dict(prob); prob4["edges"] = prob["edges"][:0]
    g, r = _run_both(corb, pyorc, prob4, 3, False)
    assert np.allclose(g["points"], prob["points"])
    with pytest.raises(corb.CorbError):
        bad = prob["edges"].copy(); bad["pose"][0] = 10 ** 6
        corb.Optimizer.GlobalBundleAdjustemnt(prob["poses"], prob["pose_fixed"], prob["points"], prob["point_fixed"], bad,
                                              prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"])


def test_larger_problem_properties(corb, synth):
    """Too large for the dense CPU oracle in seconds: check size-independent properties instead --
    chi2 is non-increasing over LM iterations, noise-free data converge to ~0 cost and to the truth."""
    prob = synth.ba_problem(n_clients=8, kf_per_client=60, pts_per_kf=40, seed=1007, pix_noise=0.0)
    g = corb.Optimizer.GlobalBundleAdjustemnt(prob["poses"], prob["pose_fixed"], prob["points"], prob["point_fixed"], prob["edges"],
                                              prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"], nIterations=10, bRobust=False)
    assert np.all(np.diff(g["chi2"]) <= 1e-6 * g["chi2"][0])
    assert g["chi2"][-1] < 1e-3 * g["chi2"][0]
    err0 = np.abs(prob["poses"][:, :3, 3] - prob["poses_true"][:, :3, 3]).max()
    err1 = np.abs(g["poses"][:, :3, 3] - prob["poses_true"][:, :3, 3]).max()
    assert err1 < 0.25 * err0


@pytest.mark.parametrize("robust", [False, True])
def test_fused_small_problem_optimiser_matches_oracle_and_the_multi_kernel_path(corb, pyorc, synth, robust):
    """solver 0 (auto) sends small problems (<= 16 free poses, <= 2048 observations) through ba_small_optimize_kernel: the whole LM run in one workgroup;
    solver 1 forces the multi-kernel path with rocSOLVER.  Same iterations / trials / chi2 trajectory as the oracle, and both paths agree."""
    for prob in (synth.ba_problem(n_clients=2, kf_per_client=4, pts_per_kf=30, seed=1011, window=3),
                 synth.ba_problem(n_clients=1, kf_per_client=14, pts_per_kf=28, seed=1012, window=5),      # 13 free poses (78 unknowns), < 2048 observations
                 synth.ba_problem(n_clients=2, kf_per_client=4, pts_per_kf=6, seed=1001, window=2)):
        g0, r = _run_both(corb, pyorc, prob, 10, robust, solver=0)
        assert g0["solver"] == 1
        _check(g0, r)
        g1, _ = _run_both(corb, pyorc, prob, 10, robust, solver=1)
        assert g0["iters_done"] == g1["iters_done"] and g0["trials"] == g1["trials"]
        assert np.allclose(g0["chi2"], g1["chi2"], rtol=1e-4) and np.abs(g0["poses"] - g1["poses"]).max() < 1e-4     # two summation orders of an ill-conditioned robust problem: the parity bar


@pytest.mark.parametrize("robust", [False, True])
def test_block_sparse_pcg_solver_matches_oracle(corb, pyorc, synth, robust):
    """solver 2 (BSR reduced camera system + block-Jacobi PCG, default tolerance 1e-8) against the oracle's exact LDLT."""
    prob = synth.ba_problem(n_clients=4, kf_per_client=25, pts_per_kf=30, seed=1004)
    g, r = _run_both(corb, pyorc, prob, 10, robust, solver=2)
    assert g["solver"] == 2 and g["pcg_iterations"] > 0
    _check(g, r)
    prob2 = synth.ba_problem(n_clients=2, kf_per_client=4, pts_per_kf=6, seed=1001, window=2); prob2["point_fixed"][3] = 1
    g, r = _run_both(corb, pyorc, prob2, 10, robust, solver=2)
    _check(g, r)


@pytest.mark.parametrize("solver", [0, 1, 2])
@pytest.mark.parametrize("point_noise,trials", [(0.3, 17), (1.0, 12)])
def test_rejected_trials_match_oracle(corb, pyorc, synth, solver, point_noise, trials):
    """Large initial errors: several LM trials are rejected (lambda grows, the estimates are restored, the retry uses the linearisation of the
    iteration's start).  The multi-kernel path enqueues the next iteration's linearisation before it knows the trial's outcome and redoes it after a
    rejection; solver 0 = the one-workgroup optimiser, 1 = multi-kernel dense, 2 = PCG."""
    prob = synth.ba_problem(n_clients=1, kf_per_client=10, pts_per_kf=15, seed=3001, pose_noise=(0.6, 0.1), point_noise=point_noise)
    g, r = _run_both(corb, pyorc, prob, 10, True, solver=solver)
    assert r["trials"] == trials and r["iters_done"] == 10
    if solver == 2:
        # at the plateau (chi2 flat to 1e-9) the sign of a trial's gain is decided by the PCG residual: the accept / reject pattern of the last
        # iterations may differ from the exact solve's, the cost and the estimates may not
        assert g["iters_done"] == 10 and g["trials"] > 10
        assert np.allclose(g["chi2"], r["chi2"], rtol=RTOL)
        assert np.abs(g["poses"] - r["poses"]).max() <= RTOL * max(1.0, np.abs(r["poses"][:, :3, 3]).max())
        assert np.abs(g["points"] - r["points"]).max() <= RTOL * max(1.0, np.abs(r["points"]).max())
    else:
        _check(g, r)


@pytest.mark.parametrize("threads", [3, 8])
def test_threaded_host_flattening_equals_the_serial_one(corb, pyorc, synth, threads, monkeypatch):
    """The host-side graph flattening (active-edge filter, stable sort by landmark, per-pose lists, block pattern) runs on worker threads from
    ~260 k observations on; forced on for a map the oracle can solve, it must reproduce the serial lists: bit-identical results, oracle parity.
    Fixed landmarks / poses and an `active` subset exercise every branch of the filter."""
    prob = synth.ba_problem(n_clients=4, kf_per_client=25, pts_per_kf=30, seed=1031)
    prob["point_fixed"][5] = 1; prob["point_fixed"][77] = 1; prob["pose_fixed"][30] = 1
    for solver in (1, 2):
        monkeypatch.setenv("CORB_BA_HOST_THREADS", "1")
        g1 = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=6, bRobust=True, solver=solver)
        monkeypatch.setenv("CORB_BA_HOST_THREADS", str(threads))
        g2 = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=6, bRobust=True, solver=solver)
        # (this generator repeats some (keyframe, point) pairs: round 2 sent such inputs to fp64-atomic Schur kernels, which were not reproducible; the pair
        # lists now carry all cross products of a repeated observation, so the deterministic kernel serves them too -- bit for bit)
        assert np.array_equal(g1["chi2"], g2["chi2"]) and np.array_equal(g1["poses"], g2["poses"]) and np.array_equal(g1["points"], g2["points"])
        assert g1["structure"] == g2["structure"]
    fast = synth.ba_problem_fast(n_clients=2, kf_per_client=40, pts_per_kf=40, seed=1032)       # no repeated pairs: the deterministic kernels, bit for bit
    monkeypatch.setenv("CORB_BA_HOST_THREADS", "1")
    f1 = corb.Optimizer.GlobalBundleAdjustemnt(*_args(fast), nIterations=5, bRobust=False, solver=2, intr=fast["intr"])
    monkeypatch.setenv("CORB_BA_HOST_THREADS", str(threads))
    f2 = corb.Optimizer.GlobalBundleAdjustemnt(*_args(fast), nIterations=5, bRobust=False, solver=2, intr=fast["intr"])
    assert f1["structure"] == f2["structure"] and f1["structure"]["schur_pairs"] > 0
    assert np.array_equal(f1["chi2"], f2["chi2"]) and np.array_equal(f1["poses"], f2["poses"]) and np.array_equal(f1["points"], f2["points"])
    r = pyorc.ba_solve(*_args(prob), iters=6, robust=True)
    _check(g2, r)


@pytest.mark.parametrize("pc_block", [8, 16])
def test_pcg_with_large_jacobi_blocks_matches_oracle(corb, pyorc, synth, pc_block):
    """block-Jacobi blocks of pc_block poses (block inverses by ba_pc_invert_kernel in LDS; dense mat-vec in the CG step): same LM trajectory as the oracle's exact
    solve; 99 free poses are not a multiple of any block size (padded last block), and the tiny map has fewer poses than one block."""
    prob = synth.ba_problem(n_clients=4, kf_per_client=25, pts_per_kf=30, seed=1004)
    g, r = _run_both(corb, pyorc, prob, 10, False, solver=2, pc_block=pc_block)
    assert g["solver"] == 2 and g["pcg_iterations"] > 0
    _check(g, r)
    g1, _ = _run_both(corb, pyorc, prob, 10, False, solver=2, pc_block=1)
    assert g["pcg_iterations"] < g1["pcg_iterations"]                 # the larger blocks pay: fewer CG iterations for the same trajectory
    prob2 = synth.ba_problem(n_clients=2, kf_per_client=4, pts_per_kf=6, seed=1001, window=2); prob2["point_fixed"][3] = 1
    g, r = _run_both(corb, pyorc, prob2, 10, True, solver=2, pc_block=pc_block)
    _check(g, r)


def test_pcg_multilevel_preconditioner_matches_oracle(corb, pyorc, synth):
    """coarse levels next to the 16-pose blocks (csrc/ba_multilevel.h: linear hats over the keyframe order, Galerkin matrices, block Jacobi per level), forced on
    maps far below the size where they are the default: the LM trajectory of the oracle's exact solve, with fewer CG iterations than the blocks alone; 799 free
    poses give two coarse levels (100 and 25 nodes -> 13 nodes is not reached: the top level has two blocks), 99 give one (13 nodes, exact)."""
    for cfg, levels in ((dict(n_clients=4, kf_per_client=25, pts_per_kf=30, seed=1004), 1), (dict(n_clients=2, kf_per_client=400, pts_per_kf=30, seed=1011), 3)):
        prob = synth.ba_problem_fast(**cfg) if cfg["kf_per_client"] > 100 else synth.ba_problem(**cfg)
        intr = prob.get("intr")
        g = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=10, bRobust=False, solver=2, pc_block=16, pc_multilevel=2, intr=intr)
        g0 = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=10, bRobust=False, solver=2, pc_block=16, pc_multilevel=1, intr=intr)
        r = pyorc.ba_solve(*_args(prob), iters=10, robust=False, intr=intr)
        assert g["solver"] == 2 and g["structure"]["pc_levels"] == levels and g0["structure"]["pc_levels"] == 0
        _check(g, r)
        _check(g0, r)
        if levels > 1:
            assert g["pcg_iterations"] < 0.7 * g0["pcg_iterations"], (g["pcg_iterations"], g0["pcg_iterations"])
        g2 = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=10, bRobust=False, solver=2, pc_block=16, pc_multilevel=2, intr=intr)
        assert np.array_equal(g["chi2"], g2["chi2"]) and g["pcg_iterations"] == g2["pcg_iterations"]          # every sum in a fixed order


def test_row_schur_kernel_with_many_observations_per_keyframe(corb, pyorc, synth):
    """the row-owner Schur kernel's work decomposition: keyframes with ~1 650 observations (five ranges of 352, blocks cut into many work units, partial blocks
    added by ba_schur_combine_kernel) next to the PCG solve, against the oracle; two runs are bit-identical."""
    prob = synth.ba_problem_fast(n_clients=2, kf_per_client=40, pts_per_kf=300, seed=1021, obs_range=(3, 8), window=6)
    a = _args(prob)
    g = corb.Optimizer.GlobalBundleAdjustemnt(*a, nIterations=10, bRobust=False, solver=2, pc_block=16, intr=prob["intr"])
    r = pyorc.ba_solve(*a, iters=10, robust=False, intr=prob["intr"])
    per_kf = np.bincount(prob["edges"]["pose"], minlength=len(prob["poses"]))
    assert per_kf.max() > 4 * 352 and g["solver"] == 2 and g["structure"]["free_poses"] >= 64
    _check(g, r)
    g2 = corb.Optimizer.GlobalBundleAdjustemnt(*a, nIterations=10, bRobust=False, solver=2, pc_block=16, intr=prob["intr"])
    assert np.array_equal(g["chi2"], g2["chi2"]) and np.array_equal(g["poses"], g2["poses"])


def test_pair_lists_by_hash_probe_and_hub_rows(corb, synth):
    """the pair lists of a map (ba_pairs_row_kernel: a block row's landmarks in an LDS hash table, hub rows with more than 2 048 observations merged serially) against
    the dense solver's, which builds them block by block with the serial merge: the same Schur complement, so the same chi2 trajectory to the CG tolerance."""
    prob = synth.ba_problem_fast(n_clients=1, kf_per_client=1300, pts_per_kf=372, seed=1033, obs_range=(3, 8), window=6)
    a = _args(prob)
    per_kf = np.bincount(prob["edges"]["pose"], minlength=len(prob["poses"]))
    assert per_kf.max() > 2048 and per_kf.min() < 2048                     # both kinds of rows
    g2 = corb.Optimizer.GlobalBundleAdjustemnt(*a, nIterations=3, bRobust=False, solver=2, pcg_tol=1e-8, intr=prob["intr"])      # (a fixed tight tolerance: the subject is the pair lists)
    g1 = corb.Optimizer.GlobalBundleAdjustemnt(*a, nIterations=3, bRobust=False, solver=1, intr=prob["intr"])
    assert g2["solver"] == 2 and g1["solver"] == 1 and g2["structure"]["schur_pairs"] == g1["structure"]["schur_pairs"] and g2["structure"]["nnz_blocks"] > 2 * 8192
    assert np.allclose(g2["chi2"], g1["chi2"], rtol=1e-6), (g2["chi2"], g1["chi2"])
    assert np.abs(g2["poses"] - g1["poses"]).max() < 1e-4


@pytest.mark.parametrize("pc_block", [1, 16])
def test_pcg_two_level_partial_reduction(corb, pyorc, synth, pc_block, monkeypatch):
    """the large-system form of the CG scalars (one-workgroup reduction kernels between the CG kernels; default above 4096 partials) on a small map"""
    monkeypatch.setenv("CORB_BA_TWO_LEVEL", "1")
    prob = synth.ba_problem(n_clients=4, kf_per_client=25, pts_per_kf=30, seed=1004)
    g, r = _run_both(corb, pyorc, prob, 10, False, solver=2, pc_block=pc_block, pcg_tol=1e-8)
    assert g["solver"] == 2 and g["pcg_iterations"] > 0
    _check(g, r)
    monkeypatch.delenv("CORB_BA_TWO_LEVEL")
    g0, _ = _run_both(corb, pyorc, prob, 10, False, solver=2, pc_block=pc_block, pcg_tol=1e-8)
    # Same algorithm, same Schur complement bit for bit (no floating-point atomic is left in the BA kernels: every sum has a fixed order, and each form is
    # bit-identical from run to run).  The two forms differ in ONE place: the order in which the CG scalars r.z, r.r, p.q are summed (per-workgroup partials
    # added by every consumer vs the three-level tree of cg_tree_reduce), i.e. alpha / beta differ in the last bits, and so do the iterates -- by far less
    # than the CG tolerance, which bounds how far either is from the exact solve.
    assert abs(g0["pcg_iterations"] - g["pcg_iterations"]) <= 0.02 * g0["pcg_iterations"] and np.allclose(g0["chi2"], g["chi2"], rtol=1e-7)


@pytest.mark.parametrize("kf", [60, 66])        # 479 / 527 free poses: below / above the size from which the 16-pose preconditioner blocks are the default
def test_pcg_and_dense_agree_on_a_larger_map(corb, synth, kf):
    prob = synth.ba_problem(n_clients=8, kf_per_client=kf, pts_per_kf=40, seed=1007)
    args = (prob["poses"], prob["pose_fixed"], prob["points"], prob["point_fixed"], prob["edges"], prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"])
    a = corb.Optimizer.GlobalBundleAdjustemnt(*args, nIterations=10, bRobust=False, solver=1)
    b = corb.Optimizer.GlobalBundleAdjustemnt(*args, nIterations=10, bRobust=False, solver=2, pcg_tol=1e-8)
    assert a["solver"] == 1 and b["solver"] == 2
    assert a["iters_done"] == b["iters_done"] and a["trials"] == b["trials"]
    assert np.allclose(a["chi2"], b["chi2"], rtol=1e-6)
    assert np.abs(a["poses"] - b["poses"]).max() < 1e-4 and np.abs(a["points"] - b["points"]).max() < 1e-3


@pytest.mark.parametrize("kf", [60, 66])
def test_default_pcg_policy_agrees_with_dense_on_a_larger_map(corb, synth, kf):
    """ the PRODUCTION default above 256 free keyframes -- pcg_tol = 0: the forcing sequence 1e-6 / clamp(1e-2 x the last relative gain, 1e-8, 1e-6) with the
    decision-safe continuation to 1e-8 -- against the dense Cholesky solve on the maps of the test above: the same accept / reject history, chi2 per LM iteration within the
    documented 1e-6, lambda within 1e-3, estimates inside the parity bar, and the solve certifies itself (true residual of every reduced solve at the tolerance's order)."""
    prob = synth.ba_problem(n_clients=8, kf_per_client=kf, pts_per_kf=40, seed=1007)
    args = (prob["poses"], prob["pose_fixed"], prob["points"], prob["point_fixed"], prob["edges"], prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"])
    a = corb.Optimizer.GlobalBundleAdjustemnt(*args, nIterations=10, bRobust=False, solver=1)
    b = corb.Optimizer.GlobalBundleAdjustemnt(*args, nIterations=10, bRobust=False, solver=2)          # pcg_tol = 0: the default policy
    assert a["solver"] == 1 and b["solver"] == 2 and b["structure"]["free_poses"] > 256
    assert a["iters_done"] == b["iters_done"] and a["trials"] == b["trials"]
    assert np.allclose(a["chi2"], b["chi2"], rtol=1e-6) and np.allclose(a["lam"], b["lam"], rtol=1e-3)
    assert np.abs(a["poses"] - b["poses"]).max() < 1e-4 and np.abs(a["points"] - b["points"]).max() < 1e-3
    c = b["certificate"]
    assert 0 < c["pcg_residual_max"] < 10 * PCG_LOOSE and c["pcg_refined_trials"] >= 0
    t = corb.Optimizer.GlobalBundleAdjustemnt(*args, nIterations=10, bRobust=False, solver=2, pcg_tol=1e-8)
    assert b["pcg_iterations"] < t["pcg_iterations"]                          # the policy is what saves iterations ...
    assert np.allclose(b["chi2"], t["chi2"], rtol=1e-6)                       # ... at the same chi2 history


# ---- BASELINE configs[3]: 4 clients on KITTI 00/02/05/07 -- two camera models in one fused map ----
def _cams4(synth):
    a, b = synth.KITTI_CAMS["00-02"], synth.KITTI_CAMS["04-12"]
    return [a, a, b, b]                  # sequences 00, 02 (KITTI00-02.yaml) and 05, 07 (KITTI04-12.yaml)


@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("robust", [False, True])
def test_four_clients_two_camera_models_match_oracle(corb, pyorc, synth, solver, robust):
    """e->fx = pKF->fx ... e->bf = pKF->mbf (Optimizer.cc:160-163, 189-193): the intrinsics travel per keyframe (CorbBAProblem.intr)"""
    prob = synth.ba_problem_fast(n_clients=4, kf_per_client=40, pts_per_kf=30, seed=1020, cams=_cams4(synth))
    assert len(np.unique(prob["intr"], axis=0)) == 2
    g, r = _run_both(corb, pyorc, prob, 10, robust, solver=solver, intr=prob["intr"])
    _check(g, r)
    shared = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=10, bRobust=robust, solver=solver)     # one camera for every keyframe: another problem
    assert abs(shared["chi2"][-1] - g["chi2"][-1]) > 0.05 * g["chi2"][-1]


def test_small_and_staged_paths_read_the_keyframes_camera(corb, pyorc, synth):
    """the one-workgroup optimiser (<= 16 free poses), LocalBundleAdjustment's staged form and the fused single-pose kernel with per-keyframe intrinsics"""
    cams = [synth.KITTI_CAMS["00-02"], synth.KITTI_CAMS["04-12"]]
    prob = synth.ba_problem_fast(n_clients=2, kf_per_client=6, pts_per_kf=20, seed=1021, cams=cams, window=3)
    g, r = _run_both(corb, pyorc, prob, 10, True, solver=0, intr=prob["intr"])
    assert g["solver"] == 1
    _check(g, r)
    gs = corb.Optimizer.LocalBundleAdjustment(*_args(prob), intr=prob["intr"])
    rs = pyorc.ba_solve_staged(*_args(prob), stages=corb.LOCAL_BA_STAGES, intr=prob["intr"])
    assert np.array_equal(gs["outlier"], rs["outlier"]) and gs["iters_done"] == rs["iters_done"]
    assert np.abs(gs["poses"] - rs["poses"]).max() < 1e-4 and np.abs(gs["points"] - rs["points"]).max() < 1e-3
    # one free keyframe of the SECOND camera, all points fixed: the fused pose kernel must use that keyframe's row, not the shared camera
    k = 8
    pf = np.ones_like(prob["pose_fixed"]); pf[k] = 0
    sel = prob["edges"][prob["edges"]["pose"] == k]
    a = (prob["poses"], pf, prob["points"], np.ones_like(prob["point_fixed"]), sel, prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"])
    g1 = corb.Optimizer._staged(corb.POSE_OPT_STAGES, *a, intr=prob["intr"])
    r1 = pyorc.ba_solve_staged(*a, stages=corb.POSE_OPT_STAGES, intr=prob["intr"])
    assert np.array_equal(g1["outlier"], r1["outlier"]) and np.abs(g1["poses"][k] - r1["poses"][k]).max() < 1e-4


@pytest.mark.parametrize("tag", ["nonrobust", "huber"])
def test_config3_size_matches_the_oracle_golden(corb, synth, tag):
    """BASELINE configs[3] size (4 clients x 1 200 keyframes, two camera models, 480 000 points, pixel noise): the PCG path -- the only reduced solver used at
    this size, with the multilevel preconditioner -- against the trajectory of the oracle's exact sparse LDL^T (tests/golden/ba_config3.json, generated in the
    build container by tools/gen_ba_golden.py: the oracle needs ~40 minutes per run at this size).  chi2 after every iteration, iteration and trial counts, lambda,
    64 sampled poses / points at 1e-4."""
    import json, os, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gold = json.load(open(os.path.join(root, "tests", "golden", "ba_config3.json")))
    if tag not in gold["runs"]:
        pytest.skip("tests/golden/ba_config3.json holds no %s run" % tag)
    sys.path.insert(0, os.path.join(root, "tools"))
    import gen_ba_golden
    prob = gen_ba_golden.make_problem(synth)
    assert gen_ba_golden.checksum(prob) == gold["checksum"], "synth.ba_problem_fast changed: regenerate the fixture (tools/gen_ba_golden.py)"
    run = gold["runs"][tag]
    g = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=10, bRobust=run["robust"], intr=prob["intr"])
    assert g["solver"] == 2 and g["structure"]["pc_levels"] >= 2
    assert g["iters_done"] == run["iters_done"] and g["trials"] == run["trials"]
    assert np.allclose(g["chi2"], run["chi2"], rtol=RTOL), (g["chi2"], run["chi2"])
    assert np.allclose(g["lam"], run["lam"], rtol=1e-3)
    pi = np.asarray(gold["pose_sample"]); xi = np.asarray(gold["point_sample"])
    rp = np.asarray(run["poses"]).reshape(-1, 4, 4); rx = np.asarray(run["points"])
    scale_t = max(1.0, np.abs(rp[:, :3, 3]).max())
    assert np.abs(g["poses"][pi][:, :3, 3] - rp[:, :3, 3]).max() <= RTOL * scale_t
    assert np.abs(g["poses"][pi][:, :3, :3] - rp[:, :3, :3]).max() <= RTOL
    assert np.abs(g["points"][xi] - rx).max() <= RTOL * max(1.0, np.abs(rx).max())


def test_twelve_thousand_keyframes_match_the_oracle_golden(corb, synth):
    """8 clients x 1 500 keyframes (12 000 keyframes, 1.2 M points, 6.6 M observations): the default PCG policy -- forcing-sequence tolerance, multilevel preconditioner --
    against the oracle's exact sparse LDL^T above the 4 800 keyframes of configs[3] (tests/golden/ba_12k.json: `python tools/gen_ba_golden.py 12k`, 3.5 hours of one core
    in the build container).  chi2 after every iteration, iteration and trial counts, lambda, 64 sampled poses / points at 1e-4."""
    import json, os, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "tests", "golden", "ba_12k.json")
    if not os.path.exists(path):
        pytest.skip("tests/golden/ba_12k.json not generated")
    gold = json.load(open(path))
    sys.path.insert(0, os.path.join(root, "tools"))
    import gen_ba_golden
    kw = dict(gold["problem"]); kw["obs_range"] = tuple(kw["obs_range"]); kw["cams"] = [synth.KITTI_CAMS[c] for c in gold["cams"]]
    prob = synth.ba_problem_fast(**kw)
    assert len(prob["poses"]) == gold["n_poses"] == 12000 and len(prob["edges"]) == gold["n_edges"]
    assert gen_ba_golden.checksum(prob) == gold["checksum"], "synth.ba_problem_fast changed: regenerate the fixture (tools/gen_ba_golden.py 12k)"
    run = gold["runs"]["nonrobust"]
    g = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=10, bRobust=False, intr=prob["intr"])
    assert g["solver"] == 2 and g["structure"]["pc_levels"] >= 3
    assert g["iters_done"] == run["iters_done"] and g["trials"] == run["trials"]
    assert np.allclose(g["chi2"], run["chi2"], rtol=RTOL), (g["chi2"], run["chi2"])
    assert np.allclose(g["lam"], run["lam"], rtol=1e-3)
    pi = np.asarray(gold["pose_sample"]); xi = np.asarray(gold["point_sample"])
    rp = np.asarray(run["poses"]).reshape(-1, 4, 4); rx = np.asarray(run["points"])
    scale_t = max(1.0, np.abs(rp[:, :3, 3]).max())
    assert np.abs(g["poses"][pi][:, :3, 3] - rp[:, :3, 3]).max() <= RTOL * scale_t
    assert np.abs(g["poses"][pi][:, :3, :3] - rp[:, :3, :3]).max() <= RTOL
    assert np.abs(g["points"][xi] - rx).max() <= RTOL * max(1.0, np.abs(rx).max())
    assert g["certificate"]["pcg_residual_max"] <= 10 * PCG_LOOSE


def test_config3_size_four_clients_properties(corb, synth):
    """BASELINE configs[3] at full size: 4 x 1 200 keyframes, 480 k points, two camera models.  Too large for the oracle: noise-free data must
    converge to ~0 cost and towards the truth, chi2 never increases, and repeated runs are bit-identical."""
    prob = synth.ba_problem_fast(n_clients=4, kf_per_client=1200, pts_per_kf=100, seed=1022, cams=_cams4(synth), pix_noise=0.0)
    assert len(prob["poses"]) == 4800
    g = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=10, bRobust=False, intr=prob["intr"])
    assert g["solver"] == 2
    assert np.all(np.diff(g["chi2"]) <= 1e-6 * g["chi2"][0]) and g["chi2"][-1] < 1e-3 * g["chi2"][0]
    err0 = np.abs(prob["poses"][:, :3, 3] - prob["poses_true"][:, :3, 3]).max()
    err1 = np.abs(g["poses"][:, :3, 3] - prob["poses_true"][:, :3, 3]).max()
    assert err1 < 0.25 * err0
    g2 = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=10, bRobust=False, intr=prob["intr"])
    assert np.array_equal(g["chi2"], g2["chi2"]) and np.array_equal(g["poses"], g2["poses"]) and np.array_equal(g["points"], g2["points"])


def test_config4_size_fifty_thousand_keyframes_properties(corb, synth):
    """BASELINE configs[4], BA half: 8 clients x 6 250 keyframes = 50 000 keyframes, 5 000 000 map points (~27 M observations), server setting
    (10 iterations, non-robust).  Properties: chi2 never increases, the noisy problem's cost drops by > 10x, every output is finite, the fixed
    keyframe is untouched."""
    prob = synth.ba_problem_fast(n_clients=8, kf_per_client=6250, pts_per_kf=100, seed=1023)
    assert len(prob["poses"]) == 50000 and len(prob["points"]) == 5000000
    g = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=10, bRobust=False, intr=prob["intr"])
    assert g["solver"] == 2 and g["iters_done"] >= 3
    assert np.all(np.diff(g["chi2"]) <= 1e-6 * g["chi2"][0]) and g["chi2"][-1] < 0.1 * g["chi2"][0]
    assert np.isfinite(g["poses"]).all() and np.isfinite(g["points"]).all()
    assert np.array_equal(g["poses"][0], prob["poses"][0].reshape(4, 4))
    err0 = np.abs(prob["poses"][:, :3, 3] - prob["poses_true"][:, :3, 3]).mean()
    err1 = np.abs(g["poses"][:, :3, 3] - prob["poses_true"][:, :3, 3]).mean()
    assert err1 < err0
    # The oracle's exact factorisation cannot run at this size (hours); the call certifies itself instead (CorbBAResult.pcg_residual_* / grad_inf):
    # the TRUE residual |b - S x| / |b| of every reduced solve, recomputed in FP64 by a kernel independent of the CG kernels, stays within 10x the
    # stop tolerance of the recurrence (default policy: at most PCG_LOOSE, G/solvers/linear_solver_eigen.h:94-124 is exact), and the
    # gradient J' Omega r at the returned estimates has dropped far below the initial one's.
    cert = g["certificate"]
    assert 0 < cert["pcg_residual_max"] <= 10 * PCG_LOOSE and 0 < cert["pcg_residual_last"] <= cert["pcg_residual_max"], cert
    g0 = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=0, bRobust=False, intr=prob["intr"], solver=2)
    assert np.isfinite(cert["grad_inf"]) and 0 <= cert["grad_inf"] < 1e-2 * g0["certificate"]["grad_inf"], (cert, g0["certificate"])
    # a tight solve certifies tighter, and moves chi2 by far less than the parity bar
    gt = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=10, bRobust=False, intr=prob["intr"], pcg_tol=1e-8)
    assert gt["certificate"]["pcg_residual_max"] <= 10 * 1e-8 and gt["pcg_iterations"] > g["pcg_iterations"]
    assert np.allclose(gt["chi2"], g["chi2"], rtol=1e-6), (gt["chi2"], g["chi2"])
    # bit-identical repeat at this size: every sum of the path has a fixed order
    g2 = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=10, bRobust=False, intr=prob["intr"])
    assert np.array_equal(g["chi2"], g2["chi2"]) and g["pcg_iterations"] == g2["pcg_iterations"] and g["certificate"] == g2["certificate"]
    assert g["poses"].tobytes() == g2["poses"].tobytes() and g["points"].tobytes() == g2["points"].tobytes()


@pytest.mark.parametrize("cfg,solver", [(dict(n_clients=2, kf_per_client=4, pts_per_kf=6, seed=1001, window=2), 0),          # fused one-workgroup optimiser
                                        (dict(n_clients=4, kf_per_client=25, pts_per_kf=30, seed=1004), 1),                  # dense reduced system
                                        (dict(n_clients=4, kf_per_client=25, pts_per_kf=30, seed=1004), 2),                  # block-sparse PCG
                                        (dict(n_clients=8, kf_per_client=60, pts_per_kf=40, seed=1009, window=6, max_obs=8), 0)])
def test_device_flattening_equals_host_flattening(corb, synth, cfg, solver):
    """corb_ba_solve_devflat (ba_flatten.hip: index mapping, landmark sort, per-keyframe lists, block pattern built by kernels -- the path of
    corb_ba_solve_store) returns what the host flattening returns: the lists are the same element for element, so chi2 histories and estimates are
    bit-identical when no map point is fixed (edges of fixed map points keep their input order on the host and the map-point order on the device)."""
    prob = synth.ba_problem(**cfg)
    a = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=10, bRobust=False, solver=solver)
    b = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=10, bRobust=False, solver=solver, devflat=True)
    assert a["structure"] == b["structure"] and a["solver"] == b["solver"] and a["iters_done"] == b["iters_done"] and a["trials"] == b["trials"]
    assert np.array_equal(a["chi2"], b["chi2"]) and np.array_equal(a["poses"], b["poses"]) and np.array_equal(a["points"], b["points"])
    # fixed map points and a second fixed keyframe, robust kernel: equal within rounding
    prob["point_fixed"][::7] = 1; prob["pose_fixed"][3] = 1
    a = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=6, bRobust=True, solver=solver, pcg_tol=1e-8)
    b = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=6, bRobust=True, solver=solver, devflat=True, pcg_tol=1e-8)
    assert a["structure"] == b["structure"] and a["iters_done"] == b["iters_done"]
    assert np.allclose(a["chi2"], b["chi2"], rtol=1e-9) and np.allclose(a["poses"], b["poses"], atol=1e-5) and np.allclose(a["points"], b["points"], atol=1e-5)
    assert np.array_equal(b["points"][::7], prob["points"][::7]) and np.array_equal(b["poses"][3], prob["poses"][3])


def test_large_host_array_call_takes_the_device_flattening_and_equals_the_host_one(corb, synth, monkeypatch):
    """corb_ba_solve_ex on a map of more than 2^20 observations whose edges arrive grouped by map point (as OptimizerT::BundleAdjustment builds them): the raw arrays
    travel through the page-locked double buffer and the graph is flattened on the device.  The same call with CORB_BA_HOST_FLATTEN=1 (host flattening): equal element
    for element.  Edges NOT grouped by point fall back to the host path (same result); an out-of-range index is refused by either."""
    prob = synth.ba_problem_fast(n_clients=4, kf_per_client=500, pts_per_kf=100, seed=1041, obs_range=(3, 8), window=6)
    assert len(prob["edges"]) > (1 << 20) and np.all(np.diff(prob["edges"]["point"].astype(np.int64)) >= 0)
    a = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=6, bRobust=False, intr=prob["intr"])
    monkeypatch.setenv("CORB_BA_HOST_FLATTEN", "1")
    b = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=6, bRobust=False, intr=prob["intr"])
    monkeypatch.delenv("CORB_BA_HOST_FLATTEN")
    assert a["structure"] == b["structure"] and a["iters_done"] == b["iters_done"] == 6 and a["trials"] == b["trials"]
    assert np.array_equal(a["chi2"], b["chi2"]) and a["poses"].tobytes() == b["poses"].tobytes() and a["points"].tobytes() == b["points"].tobytes()
    # fixed map points and further fixed keyframes at this size (the thread-per-edge placement and the workgroup-aggregated keyframe lists of the maps' flattening:
    # an edge's rank among the free-keyframe / fixed-keyframe edges of its point, edges between two fixed vertices dropped)
    fx = dict(prob); fx["point_fixed"] = prob["point_fixed"].copy(); fx["point_fixed"][::7] = 1; fx["pose_fixed"] = prob["pose_fixed"].copy(); fx["pose_fixed"][[3, 700, 1999]] = 1
    a2 = corb.Optimizer.GlobalBundleAdjustemnt(*_args(fx), nIterations=3, bRobust=False, intr=prob["intr"])
    monkeypatch.setenv("CORB_BA_HOST_FLATTEN", "1")
    b2 = corb.Optimizer.GlobalBundleAdjustemnt(*_args(fx), nIterations=3, bRobust=False, intr=prob["intr"])
    monkeypatch.delenv("CORB_BA_HOST_FLATTEN")
    assert a2["structure"] == b2["structure"] and a2["trials"] == b2["trials"] and np.array_equal(a2["chi2"], b2["chi2"])
    assert a2["poses"].tobytes() == b2["poses"].tobytes() and a2["points"].tobytes() == b2["points"].tobytes()
    assert np.array_equal(a2["points"][::7], prob["points"][::7]) and np.array_equal(a2["poses"][700], prob["poses"][700])
    # shuffled edges: not grouped by point -> the host path, whose stable sort by landmark restores the order inside a landmark only up to the shuffle: chi2 at rounding
    sh = dict(prob); rng = np.random.default_rng(3); sh["edges"] = prob["edges"][rng.permutation(len(prob["edges"]))]
    c = corb.Optimizer.GlobalBundleAdjustemnt(*_args(sh), nIterations=6, bRobust=False, intr=prob["intr"])
    assert c["iters_done"] == 6 and np.allclose(c["chi2"], a["chi2"], rtol=1e-9)
    bad = dict(prob); bad["edges"] = prob["edges"].copy(); bad["edges"]["pose"][12345] = len(prob["poses"])
    with pytest.raises(corb.CorbError, match="out of range"):
        corb.Optimizer.GlobalBundleAdjustemnt(*_args(bad), nIterations=2, bRobust=False, intr=prob["intr"])


@pytest.mark.parametrize("solver", [1, 2])
def test_repeated_observations_are_deterministic_and_match_the_oracle(corb, pyorc, synth, solver):
    """A (keyframe, map point) pair that occurs twice (the reference cannot produce one -- MapPoint::mObservations is a std::map keyed by the keyframe -- but
    the C-ABI accepts it): the pair lists of the Schur kernel hold every cross product of such a pair, i.e. the summed Hpl block of g2o.  Oracle parity
    and bit-identical runs; no atomic fallback exists any more."""
    prob = synth.ba_problem(n_clients=3, kf_per_client=12, pts_per_kf=20, seed=1041, window=4)
    e = prob["edges"]
    dup = e[::9].copy(); dup["u"] += 0.5; dup["v"] -= 0.25                       # every 9th observation a second time, with another measurement
    trip = e[::31].copy(); trip["u"] -= 0.3
    prob["edges"] = np.concatenate([e, dup, trip])
    prob["point_fixed"][4] = 1
    runs = [corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=10, bRobust=False, solver=solver, devflat=df) for df in (False, False, True)]
    r = pyorc.ba_solve(*_args(prob), iters=10, robust=False)
    for g in runs:
        _check(g, r)
    assert np.array_equal(runs[0]["chi2"], runs[1]["chi2"]) and np.array_equal(runs[0]["poses"], runs[1]["poses"]) and np.array_equal(runs[0]["points"], runs[1]["points"])
    assert runs[0]["structure"] == runs[2]["structure"]


def test_dense_spd_solver(corb):
    """csrc/dense_chol.hip (blocked Cholesky, FP64 MFMA trailing updates, the right-hand side carried as an extra row, backward substitution by one workgroup)
    against numpy on sizes around the panel (32) and tile (64) edges, a reduced-camera-system size, an ill-conditioned matrix and a non-SPD one."""
    rng = np.random.default_rng(77)
    for n in (1, 5, 31, 32, 33, 63, 64, 65, 96, 97, 130, 200, 402, 1536):
        M = rng.normal(size=(n, n + 8)); A = M @ M.T + 0.5 * np.eye(n); b = rng.normal(size=n)
        Au = A.copy(); Au[np.triu_indices(n, 1)] = np.nan                     # only the lower triangle may be read
        x, info = corb.spd_solve(Au, b)
        ref = np.linalg.solve(A, b)
        assert info == 0 and np.abs(x - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), (n, np.abs(x - ref).max())
        x2, _ = corb.spd_solve(Au, b)
        assert np.array_equal(x, x2)                                          # no atomics: bit-identical runs
    n = 300
    Q, _ = np.linalg.qr(rng.normal(size=(n, n))); A = (Q * np.logspace(0, -10, n)) @ Q.T; A = 0.5 * (A + A.T); b = A @ rng.normal(size=n)
    x, info = corb.spd_solve(A, b)
    assert info == 0 and np.linalg.norm(A @ x - b) <= 1e-8 * np.linalg.norm(b)          # cond 1e10: the residual is what a backward-stable solve bounds
    A = np.eye(70); A[40, 40] = -1.0
    _, info = corb.spd_solve(A, np.ones(70))
    assert info == 41
    A = np.eye(10); A[3, 3] = np.nan
    _, info = corb.spd_solve(A, np.ones(10))
    assert info == 4



def test_release_scratch_gives_the_arenas_back_and_the_next_call_rebuilds_them(corb, synth):
    """corb_release_scratch: the workspace arenas (and, after a large host-array call, its staging) return to the runtime; the same call afterwards allocates them again
    and returns the same bits"""
    prob = synth.ba_problem_fast(n_clients=2, kf_per_client=200, pts_per_kf=60, seed=1077, obs_range=(3, 6), window=5)
    a = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=4, bRobust=False, intr=prob["intr"])
    freed = corb.release_scratch(0)
    assert freed >= (8 << 20)                                     # at least the smallest arena chunk
    assert corb.release_scratch(0) == 0                           # nothing left to give back
    b = corb.Optimizer.GlobalBundleAdjustemnt(*_args(prob), nIterations=4, bRobust=False, intr=prob["intr"])
    assert np.array_equal(a["chi2"], b["chi2"]) and a["poses"].tobytes() == b["poses"].tobytes() and a["points"].tobytes() == b["points"].tobytes()

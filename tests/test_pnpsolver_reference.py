"""CPU tests that pin tests/pnpsolver_reference.py, the definition the PnPsolver RANSAC on the device is held to bit for bit: the draw rule, SetRansacParameters, the two
Jacobi decompositions against LAPACK, compute_pose against ground truth, the replay rule against a literal emulation of iterate(), and that the seeded cases of the
GPU suite are what they claim to be.

Measured here (seeds below): jacobi_eig's eigenvalues differ from numpy.linalg.eigvalsh by at most 1.9e-15 max|lambda| and hestenes' singular values from
numpy.linalg.svd by at most 9.2e-16 max w; the bars are 16 times that (other seeds), 3.0e-14 and 1.5e-14.  compute_pose on 200 noise-free scenes each: max|R - R_true| =
4.9e-7 / 3.4e-7 / 1.9e-7 and |t - t_true|_inf = 1.3e-5 / 3.7e-6 / 1.1e-6 at n = 6 / 12 / 50, against bars of 2e-5 and 2e-4.  n = 4 is excluded by design: MtM of four
points has an exact four-dimensional null space whose basis is the decomposition's rounding, so the pose is not a well-posed function of the input (a LAPACK prototype
recovers it in 37 % of trials)."""
import os
import re
import numpy as np
import pytest
import pnpsolver_reference as R
import gpu_pnp_cases as G

EIG_BAR, SVD_BAR = 16 * 1.9e-15, 16 * 9.2e-16
R_BAR, T_BAR = 2e-5, 2e-4


def test_draw_rule_equals_the_literal_emulation():
    rng = np.random.RandomState(3)
    for min_set in range(4, 9):
        for N in (min_set, min_set + 1, 9, 10, 17, 64, 300):
            for _ in range(60):
                r = rng.randint(0, R.RAND_RANGE, min_set)
                if rng.rand() < 0.3:                                     # provoke picks of the back and of swapped positions
                    r[rng.randint(min_set)] = R.RAND_RANGE - 1
                if rng.rand() < 0.3:
                    r[:] = r[0]
                assert R.draw_set(r, min_set, N) == R.draw_set_literal(r, min_set, N)
    rv = np.zeros((1, 4), np.int32); G.force(rv, 0, [3, 5, 8, 13], 40)


def test_ransac_parameters():
    assert R.ransac_parameters(200, 0.99, 10, 300, 4, 0.5) == (35, 100)           # the cap is 35 at epsilon 0.5: ceil(log(0.01) / log(1 - 0.5^3)), whatever minSet is
    assert R.ransac_parameters(200, 0.99, 10, 300, 6, 0.5) == (35, 100)
    assert R.ransac_parameters(10, 0.99, 10, 300, 4, 0.5) == (1, 10)              # N == m
    assert R.ransac_parameters(9, 0.99, 10, 300, 4, 0.5) == (0, 10)               # N < m: no iterations
    assert R.ransac_parameters(11, 0.99, 10, 300, 4, 0.5) == (4, 10)              # epsilon raised to 10 / 11
    assert R.ransac_parameters(300, 0.99, 10, 300, 4, 0.2) == (300, 60)           # 574 capped by maxIterations
    assert R.ransac_parameters(300, 0.99, 10, 20, 4, 0.5)[0] == 20
    assert R.ransac_parameters(5, 0.99, 2, 300, 4, 0.4) == (7, 4)                 # raised to minSet; epsilon raised to 0.8: ceil(4.605 / 0.717)
    assert R.max_errors([np.float32(1.44)])[0] == np.float32(1.44) * np.float32(5.991)


def test_jacobi_routines_agree_with_lapack():
    rng = np.random.default_rng(5)
    worst_e = worst_s = 0.0
    for n in (3, 12):
        B = rng.normal(size=(50, n, n)); full = B + B.transpose(0, 2, 1)
        Bd = rng.normal(size=(50, n, max(n - 4, 1))); deficient = Bd @ Bd.transpose(0, 2, 1)
        for M in (full, deficient):
            lam, V = R.jacobi_eig(M)
            for i in range(len(M)):
                e = np.linalg.eigvalsh(M[i])
                worst_e = max(worst_e, np.abs(np.sort(lam[i]) - e).max() / np.abs(e).max())
                assert np.abs(V[i].T @ V[i] - np.eye(n)).max() < 1e-13 and np.abs(M[i] @ V[i] - V[i] * lam[i]).max() < 1e-12 * np.abs(e).max()
    for m, n in ((3, 3), (6, 4), (6, 3), (6, 5)):
        full = rng.normal(size=(50, m, n)); deficient = rng.normal(size=(50, m, n - 1)) @ rng.normal(size=(50, n - 1, n))
        for M in (full, deficient):
            UW, V, w, order = R.hestenes(M)
            for i in range(len(M)):
                e = np.linalg.svd(M[i], compute_uv=False)
                worst_s = max(worst_s, np.abs(w[i][order[i]] - e).max() / e.max())
                assert np.abs(UW[i] @ V[i].T - M[i]).max() < 1e-13 * e.max()
        x = R.sv_solve(R.hestenes(full), np.ones((50, m)))
        for i in range(50):
            assert np.abs(x[i] - np.linalg.lstsq(full[i], np.ones(m), rcond=None)[0]).max() < 1e-10
    print("jacobi_eig vs eigvalsh: %.3g (bar %.3g); hestenes vs svd: %.3g (bar %.3g)" % (worst_e, EIG_BAR, worst_s, SVD_BAR))
    assert worst_e <= EIG_BAR and worst_s <= SVD_BAR
    # NaN rotates nothing; ties keep the lower index first
    lam, V = R.jacobi_eig(np.full((1, 3, 3), np.nan))
    assert np.isnan(lam).all() and np.array_equal(V[0], np.eye(3))
    assert R.order_desc([1.0, 2.0, 2.0, 0.5, 2.0]) == [1, 2, 4, 0, 3] and R.order_desc([np.nan, 1.0, 2.0]) == [0, 2, 1]


@pytest.mark.parametrize("n", [6, 12, 50])
def test_compute_pose_recovers_the_ground_truth(n):
    P, U, T = [], [], []
    for s in range(200):
        pr, tr = R.scene(1000 + s, n, 1.0, 0.0)
        P.append(pr["p3dw"]); U.append(pr["p2d"]); T.append(tr)
    h = R.compute_pose(np.array(P), np.array(U), R.KITTI)
    dR = max(np.abs(h["R"][i] - T[i]["R"]).max() for i in range(200)); dt = max(np.abs(h["t"][i] - T[i]["t"]).max() for i in range(200))
    print("n = %d: max|R - R_true| = %.3g (bar %.3g), |t - t_true|_inf = %.3g (bar %.3g)" % (n, dR, R_BAR, dt, T_BAR))
    assert dR <= R_BAR and dt <= T_BAR


def test_first_event_of_a_half_outlier_scene():
    seed = next(s for s in range(70, 90) if R.scene(s, 200, 0.5, 0.0)[1]["inlier"].sum() > 103)       # a 50 % draw that leaves more than m = 100 true ones
    pr, tr = R.scene(seed, 200, 0.5, 0.0)
    out = R.ransac(pr, R.draws(seed, 1, 300)[0], **G.PARAMS)
    assert out["cap"] == 35 and out["m"] == 100 and out["records"]
    rec = out["records"][0]
    assert rec["i"] + 1 < out["cap"] and rec["refine_ok"] and rec["n_inliers"] == int(tr["inlier"].sum())
    ok = {r["i"]: r["refine_ok"] for r in out["records"]}
    first = R.replay(list(out["counts"]), ok, out["m"], out["cap"], [5])[0]
    assert first[0] == "refined" and first[1] == rec["i"] and first[2] < out["cap"]                 # the event occurs before the cap
    dR = np.abs(rec["pose"][:9].reshape(3, 3) - tr["R"]).max(); dt = np.abs(rec["pose"][9:12] - tr["t"]).max()
    print("refined pose of the first event: max|dR| = %.3g, |dt|_inf = %.3g" % (dR, dt))
    assert dR <= R_BAR and dt <= T_BAR


def test_replay_rule_equals_the_stateful_emulation():
    rng = np.random.RandomState(11)
    kinds = set(); straddled = 0; multi = 0
    for trial in range(400):
        m = int(rng.randint(4, 12)); cap = int(rng.randint(1, 40)); n = cap + 60
        counts = rng.randint(0, m + 6, n) * (rng.rand(n) < rng.choice([0.05, 0.2, 0.6]))       # ties and runs of equal counts included
        counts = [int(c) for c in counts]
        recs = R.records_of(counts, m); multi += len(recs) > 1
        ok = {i: bool(rng.rand() < rng.choice([0.0, 0.5, 1.0])) for i in recs}
        calls = [int(rng.choice([1, 3, 5, 5, 5, 7])) for _ in range(8)]
        lit = R.iterate_literal(counts, ok, m, cap, calls); rule = R.replay(counts, ok, m, cap, calls)
        assert lit == rule, (trial, counts, ok, m, cap, calls, lit, rule)
        kinds |= {x[0] for x in lit}
        s = 0
        for c, x in zip(calls, lit):
            straddled += s < cap < x[2] or (s < cap and s + c > cap)
            s = x[2]
    assert kinds == {"refined", "best", None} and straddled > 20 and multi > 50
    # records: c_i >= m and c_i > every earlier c_j >= m
    assert R.records_of([3, 9, 12, 12, 11, 13, 2, 13], 10) == [2, 5]


def test_constructor_filter():
    pts = {5: dict(pos=[1, 2, 3], bad=False), 6: dict(pos=[4, 5, 6], bad=True), 7: dict(pos=[7, 8, 9], bad=False)}
    kp = np.arange(10, dtype=np.float32).reshape(5, 2); octave = np.array([0, 1, 2, 9, -1])
    ids = np.array([5, 6, R.NO_MAP_POINT, 7, 12345], np.uint64)
    pr, idx = R.constructor(kp, octave, ids, pts, (np.float32(1.2) ** np.arange(4)).astype(np.float32), R.KITTI)
    assert idx.tolist() == [0, 3] and pr["n"] == 2 and np.array_equal(pr["p2d"], kp[[0, 3]]) and np.array_equal(pr["p3dw"], np.array([[1, 2, 3], [7, 8, 9]], np.float32))
    s3 = np.float32(1.2) ** np.float32(3)
    assert pr["sigma2"].tolist() == [1.0, float(np.float32(s3 * s3))]


def test_special_case_takes_the_special_branches():
    """the forced draws of the GPU suite's special case really reach the pseudo-inverse's drop branch, the cross-product branch, the NaN rotation and qr_solve's singular
    return; otherwise the case would test nothing"""
    pr, sets, rv = G.special()
    assert [R.draw_set(rv[0][i], 4, pr["n"]) for i in range(4)] == sets
    assert np.array_equal(pr["p3dw"][4], pr["p3dw"][5]) and (pr["p3dw"][:4, 2] == 2.0).all()
    taken = {}
    for k, s in enumerate(sets):
        before = dict(R.BRANCHES)
        h = R.compute_pose(*[x[None] for x in R.gather_sets(pr, s)], pr["K"])
        taken[k] = {b: R.BRANCHES[b] - before[b] for b in before}
        if k == 2:
            Zc = h["R"][0, 2] @ pr["p3dw"][20].astype(np.float64) + h["t"][0, 2]
            assert abs(Zc) < 1e-5 and not R.check_inliers(pr, h["R"], h["t"])[0, 20]
        if k == 3:
            assert not np.isfinite(h["R"]).all()
    print(taken)
    # coplanar: an exactly zero eigenvalue, so CC has a zero column that the pseudo-inverse drops; the duplicated point: a rank-two ABt completed by the cross product; the
    # four equal correspondences: everything dropped, a NaN rotation; the clean sample: none of them
    assert taken[0]["sv_drop"] > 0 and taken[0]["cross"] > 0 and taken[1]["cross"] > 0 and taken[3]["sv_drop"] > 0 and taken[3]["nan_R"] > 0 and taken[0]["qr_singular"] > 0
    assert not any(taken[2].values())


def test_epsilon_case_has_several_records():
    case = G.host_cases()["epsilon_02"]
    outs = [R.ransac(pr, rv, tail_iterations=case["tail"], **case["params"]) for pr, rv in zip(case["problems"], case["rand"])]
    assert [o["cap"] for o in outs] == [300, 300] and [len(o["records"]) for o in outs] == [4, 5]


def test_refine_set_sizes():
    sizes = []
    for pr, rv, n_in in G.refine_scenes():
        out = R.ransac(pr, rv[0], **G.PARAMS)
        assert out["records"] and out["records"][0]["i"] == 0
        sizes.append(len(out["records"][0]["set"]))
    assert sizes == [10, 64, 65]


def test_new_symbols_are_declared_and_exported(corb):
    import ctypes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "corb_accel.h")).read(), flags=re.S)
    L = ctypes.CDLL(corb.LIB_PATH)
    assert re.search(r"\bint\s+corb_pnp_ransac\s*\(", src) and hasattr(L, "corb_pnp_ransac") and "corb_pnp_ransac" in corb.EXPORTS
    assert "CorbPnPRansacProblem" in src and "CorbPnPRansacRecord" in src and "#define CORB_ABI_VERSION 6" in src
    assert ctypes.sizeof(corb._PnPRansacProblem) == 48 and corb.PNP_RECORD_DTYPE.itemsize == 112

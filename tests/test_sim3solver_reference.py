"""CPU tests of the numpy restatement of Sim3Solver (tests/sim3solver_reference.py): a known similarity, the integer thresholds, SetRansacParameters' cap, the draw
mapping against a literal list-with-pop emulation, the event rule against a literal transcription of iterate(), the identity-rotation triple, and the exports of the
built library.  The GPU tests (test_gpu_sim3_ransac.py) compare the device against this restatement."""
import ctypes
import os
import re
import numpy as np
import sim3solver_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _triangle():
    """three points 5-10 m apart, 8-20 m in front of the camera"""
    return np.array([[-4.0, 1.0, 8.0], [5.0, -1.5, 12.0], [0.5, 2.0, 20.0]])


def test_known_similarity_is_recovered():
    """noise-free X1 = s R X2 + t: coordinates round at 20 * 2^-24 = 1.2e-6 and the centred triangle spans 5 m or more, so R, s are right to a few 1e-6 and t (which
    multiplies the rotation error by the centroid's 13 m) to a few 1e-5; the bounds are 1e-4 and 1e-3"""
    rng = np.random.default_rng(3)
    for s_true, fix in ((1.0, False), (1.0, True), (1.7, False), (0.6, False)):
        Rt = R._rot(rng, 1.2); t = rng.uniform(-2, 2, 3)
        X2 = _triangle(); X1 = s_true * X2 @ Rt.T + t
        h = R.compute_sim3(X1.astype(np.float32), X2.astype(np.float32), fix)
        assert h["ok"] and np.abs(h["R"] - Rt).max() < 1e-4 and abs(float(h["s"]) - s_true) < 1e-4 and np.abs(h["t"] - t).max() < 1e-3
        assert abs(np.linalg.det(h["R"].astype(np.float64)) - 1) < 1e-5
        if fix:
            assert h["s"] == np.float32(1.0)
        # every correspondence of the same similarity is an inlier of it, in both directions
        pr, _ = R.scene(8, 50, outlier_share=0.0, noise=0.0)
        X2n = pr["x2"].astype(np.float64); X1n = s_true * X2n @ Rt.T + t
        ok = X1n[:, 2] > 1
        pr = R.problem(X1n[ok], X2n[ok], pr["sigma2_1"][ok], pr["sigma2_2"][ok], R.KITTI, R.KITTI)
        assert R.check_inliers(pr, h).all()


def test_sign_of_the_quaternion_cancels_exactly():
    q = np.array([0.83, -0.31, 0.22, 0.4], np.float32)
    assert np.array_equal(R.rotation(q).view(np.uint32), R.rotation(-q).view(np.uint32))
    ang = 2 * np.arctan2(np.linalg.norm(q[1:].astype(np.float64)), np.float64(q[0])); ax = q[1:].astype(np.float64) / np.linalg.norm(q[1:].astype(np.float64))
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    assert np.abs(R.rotation(q) - (np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K)).max() <= 2.0 ** -23      # the same function as atan2 + Rodrigues


def test_thresholds_are_truncated_integers():
    assert R.thresholds(np.array([1.0, 1.44], np.float32)).tolist() == [9.0, 13.0]
    assert R.thresholds(np.array([np.float32(1.2) ** 2 * np.float32(1.2) ** 2], np.float32)).tolist() == [19.0]      # 9.21 * 2.0736 = 19.09


def test_cap():
    assert [R.ransac_cap(n, 0.99, 20, 300) for n in (19, 20, 40, 200)] == [0, 1, 35, 300]
    assert R.ransac_cap(21, 0.99, 20, 300) == 3 and R.ransac_cap(200, 0.99, 20, 50) == 50


def test_draw_mapping_matches_the_list_emulation():
    rng = np.random.RandomState(4)
    for N in (3, 4, 5, 6, 20, 65):
        for r in rng.randint(0, R.RAND_RANGE, (3000, 3)):
            assert R.draw_triple(r, N) == R.draw_triple_literal(r, N)
    # forced collisions of the drawn positions: r1 == r0, r2 on either earlier position, the back itself
    for N in (3, 4, 5, 9):
        pos = lambda p, size: int((p + 0.5) / size * R.RAND_RANGE)
        for p0 in range(N):
            for p1 in range(N - 1):
                for p2 in range(N - 2):
                    r = (pos(p0, N), pos(p1, N - 1), pos(p2, N - 2))
                    got = R.draw_triple(r, N)
                    assert got == R.draw_triple_literal(r, N) and len(set(got)) == 3 and all(0 <= g < N for g in got)
    assert R.draw_triple((R.RAND_RANGE - 1,) * 3, 3) == R.draw_triple_literal((R.RAND_RANGE - 1,) * 3, 3) == (2, 1, 0)


def test_event_rule_matches_the_iterate_loop():
    rng = np.random.RandomState(9)
    for trial in range(400):
        cap = int(rng.randint(1, 40)); mn = int(rng.randint(3, 12))
        counts = rng.randint(max(mn - 3, 0), mn + 4, cap)                    # few distinct values: ties, and counts equal to min_inliers
        ev = [i + 1 for i in R.events_of(counts, mn)]
        for chunk in (1, 5, cap, 300):
            assert R.iterate_literal(counts, cap, mn, chunk) == ev
    assert R.events_of([20, 20, 21, 21, 20, 22], 20) == [2, 3, 5] and R.events_of([20, 19], 20) == []


def test_identity_rotation_triple_has_no_inliers():
    """p1c == p2c without noise: M is symmetric, N's first row is (trace, 0, 0, 0), the quaternion is (1, 0, 0, 0) and the reference divides 0 by 0 (:280)"""
    X = _triangle().astype(np.float32)
    h = R.compute_sim3(X, X)
    assert not h["N"][0, 1:].any() and h["q"].tolist() == [1.0, 0.0, 0.0, 0.0] and not h["ok"] and np.isnan(h["R"]).all() and np.isnan(h["t"]).all() and np.isnan(h["s"])
    pr = R.problem(X, X, np.ones(3, np.float32), np.ones(3, np.float32), R.KITTI, R.KITTI)
    assert not R.check_inliers(pr, h).any()
    out = R.ransac(pr, R.draws(1, 1, 5)[0], 0.99, 3, 5)
    assert out["cap"] == 1 and out["counts"].tolist() == [0] and out["events"] == []


def test_gpu_cases_are_well_conditioned():
    """the seeds test_gpu_sim3_ransac.py runs: at most 5 % of a case's hypotheses have a relative eigen-gap below 2^-10, and without a device the restatement's own
    Jacobi quaternion is within 2^-23 of float64 eigh's eigenvector wherever the gap holds"""
    import gpu_sim3_cases as G
    worst = 0.0
    for name, case in G.host_cases().items():
        for pr, rv in zip(case["problems"], case["rand"]):
            out = R.ransac(pr, rv, 0.99, case["min_inliers"], case["max_iterations"], case["fix_scale"])
            low = 0
            for q, N, ok in zip(out["q"], out["N"], out["ok"]):
                v, gap = R.eigen_gap(N)
                if gap < 2.0 ** -10:
                    low += 1
                    continue
                worst = max(worst, min(np.abs(q - v).max(), np.abs(q + v).max()))
            assert low <= 0.05 * max(out["cap"], 1), name
    assert worst <= 2.0 ** -23


def test_new_symbols_are_declared_and_exported(corb):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "corb_accel.h")).read(), flags=re.S)
    L = ctypes.CDLL(corb.LIB_PATH)
    for name in ("corb_sim3_ransac", "corb_sim3_ransac_store"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src) and hasattr(L, name) and name in corb.EXPORTS
    assert "CorbSim3RansacProblem" in src and "CorbSim3RansacEvent" in src
    assert ctypes.sizeof(corb._Sim3RansacProblem) == 72 and corb.SIM3_EVENT_DTYPE.itemsize == 60

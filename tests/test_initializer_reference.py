"""CPU tests that pin tests/initializer_reference.py, the definition the device is held to (tests/test_gpu_initializer.py): the draw rule against a literal emulation,
Normalize against a literal loop, the Jacobi decompositions against numpy.linalg.svd, ground truth on noise-free scenes, the sign invariance of H and F, every status,
the quirks of the source, and the declaration of the C-ABI.

Measured on the seeds below (the worst case of each; every bar is 16 x it, as in test_pnpsolver_reference.py):
  null vectors of the 16 x 9 / 8 x 9 / 4 x 4 systems: singular values against LAPACK 2.2e-15 of the largest (bar 3.5e-14); |A v| - sigma_min 4.1e-16 of the largest
    singular value in double (bar 6.6e-15), and 2.3e-8 after the rounding of v to float (bar 3.6e-7);
  3 x 3 decompositions (float results): singular values 4.6e-8 of the largest (bar 7.4e-7); |U diag(w) Vt - M| 5.7e-8 of |M| (bar 9.2e-7);
  H21 against the plane-induced homography, both of unit Frobenius norm: 7.1e-7 (bar 1.14e-5);
  F21: distance of a key to the epipolar line of its match 1.95e-4 px (bar 3.1e-3 px);
  R21 against the true rotation 1.77e-4 rad (BAR_ROTATION 2.8e-3); t21 against the true direction 2.1e-5 rad (BAR_DIRECTION 3.4e-4);
  triangulated points against truth / baseline 7.4e-5 relative (BAR_POINTS 1.19e-3)."""
import os
import re
import numpy as np
import pytest
import initializer_reference as R
import pnpsolver_reference as P
import gpu_init_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_NULL_SV, BAR_NULL_RES, BAR_NULL_RES_F32 = 3.5e-14, 6.6e-15, 3.6e-7
BAR_SVD3_SV, BAR_SVD3_REC = 7.4e-7, 9.2e-7
BAR_H, BAR_F_PX = 1.14e-5, 3.1e-3
BAR_ROTATION, BAR_DIRECTION, BAR_POINTS = 2.8e-3, 3.4e-4, 1.19e-3
TRUTH_SCENES = [("general", 105, 129), ("general", 106, 200), ("planar", 210, 65), ("planar", 210, 129)]           # the definition returns true on each


def test_draw_rule_against_a_literal_emulation():
    rng = np.random.default_rng(1)
    for N in (8, 9, 10, 15, 16, 63, 200):
        for r in rng.integers(0, R.RAND_RANGE, size=(40, 8)):
            s = R.draw_sets(r[None], N)[0].tolist()
            assert s == P.draw_set_literal(r, 8, N) and len(set(s)) == 8 and min(s) >= 0 and max(s) < N
    assert sorted(R.draw_sets(rng.integers(0, R.RAND_RANGE, size=(1, 8)), 8)[0].tolist()) == list(range(8))         # N = 8: a permutation
    edge = np.array([[0, R.RAND_RANGE - 1] * 4], np.int64)
    assert R.draw_sets(edge, 9)[0].tolist() == P.draw_set_literal(edge[0], 8, 9)


def test_normalize_against_a_literal_loop():
    f32 = np.float32
    for seed, n in ((1, 1), (2, 7), (3, 500), (4, 2000)):
        xy = np.random.default_rng(seed).uniform(0, 1241, (n, 2)).astype(f32)
        mx = my = f32(0)
        for x, y in xy:
            mx = f32(mx + x); my = f32(my + y)
        mx = f32(mx / f32(n)); my = f32(my / f32(n))
        dx = dy = f32(0)
        for x, y in xy:
            dx = f32(dx + abs(f32(x - mx))); dy = f32(dy + abs(f32(y - my)))
        with np.errstate(all="ignore"):
            dx = f32(dx / f32(n)); dy = f32(dy / f32(n))
            want = np.array([mx, my, f32(1.0 / np.float64(dx)), f32(1.0 / np.float64(dy))], f32)
        assert R.normalize(xy).tobytes() == want.tobytes()
    T = R.T_of(np.array([3, 5, 0.5, 0.25], f32))
    assert T.tolist() == [[0.5, 0, -1.5], [0, 0.25, -1.25], [0, 0, 1]]


def _systems(seed):
    pr, _ = G.scene(seed, 40, "general", 0.5)
    m, i1, i2 = R.pack_matches(pr["keys1"], pr["keys2"], pr["matches12"])
    sets = R.draw_sets(R.draws(seed, 1, 30)[0], 40)
    n1, n2 = R.normalize(pr["keys1"]), R.normalize(pr["keys2"])
    p1 = ((pr["keys1"][i1] - n1[:2]) * n1[2:])[sets]; p2 = ((pr["keys2"][i2] - n2[:2]) * n2[2:])[sets]
    u1, v1, u2, v2 = p1[:, :, 0], p1[:, :, 1], p2[:, :, 0], p2[:, :, 1]
    A8 = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], axis=2)
    A16 = np.zeros((len(sets), 16, 9), np.float32); z = np.zeros_like(u1); o = np.ones_like(u1)
    A16[:, 0::2] = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], axis=2); A16[:, 1::2] = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], axis=2)
    A4 = np.random.default_rng(seed).normal(size=(30, 4, 4)).astype(np.float32)
    return [A16, A8, A4], R.compute_F21(p1, p2)


def decomposition_errors(seeds=(1, 2, 3)):
    sv = res = res32 = sv3 = rec3 = 0.0
    for seed in seeds:
        systems, F = _systems(seed)
        for A in systems:
            Ad = A.astype(np.float64)
            UW, V, w, order = P.hestenes(Ad)
            for k in range(len(A)):
                s = np.linalg.svd(Ad[k], compute_uv=False); s = np.concatenate([s, np.zeros(A.shape[2] - len(s))])
                sv = max(sv, np.abs(np.sort(w[k])[::-1] - s).max() / s[0])
                v = V[k, :, order[k, -1]]
                res = max(res, abs(np.linalg.norm(Ad[k] @ v) - s[-1]) / s[0])
                res32 = max(res32, abs(np.linalg.norm(Ad[k] @ R.svd_null(A[k:k + 1])[0].astype(np.float64)) - s[-1]) / s[0])
        M = np.concatenate([F, np.random.default_rng(seed).normal(size=(20, 3, 3)).astype(np.float32)])
        U, w, Vt = R.svd3(M)
        for k in range(len(M)):
            s = np.linalg.svd(M[k].astype(np.float64), compute_uv=False)
            sv3 = max(sv3, np.abs(w[k] - s).max() / s[0])
            rec3 = max(rec3, np.abs((U[k].astype(np.float64) * w[k]) @ Vt[k] - M[k]).max() / np.linalg.norm(M[k]))
            assert w[k][0] >= w[k][1] >= w[k][2]
    return sv, res, res32, sv3, rec3


def test_jacobi_decompositions_against_lapack():
    sv, res, res32, sv3, rec3 = decomposition_errors()
    print("null: sv %.3g residual %.3g float %.3g; 3x3: sv %.3g reconstruction %.3g" % (sv, res, res32, sv3, rec3))
    assert sv <= BAR_NULL_SV and res <= BAR_NULL_RES and res32 <= BAR_NULL_RES_F32 and sv3 <= BAR_SVD3_SV and rec3 <= BAR_SVD3_REC


def truth_errors(R21, t21, p3d, tri, truth):
    """-> (rotation error [rad], direction error [rad], worst relative error of a triangulated point against truth times the one free scale 1 / baseline)"""
    R21 = np.asarray(R21, np.float64).reshape(3, 3); t21 = np.asarray(t21, np.float64)
    rot = np.arccos(np.clip((np.trace(R21 @ truth["R"].T) - 1) / 2, -1, 1))
    direction = np.arccos(np.clip(t21 @ truth["t"] / (np.linalg.norm(t21) * np.linalg.norm(truth["t"])), -1, 1))
    X = truth["X"] / np.linalg.norm(truth["t"]); got = np.asarray(p3d, np.float64)[truth["i1"]]; sel = np.asarray(tri)[truth["i1"]]
    points = (np.linalg.norm(got[sel] - X[sel], axis=1) / np.linalg.norm(X[sel], axis=1)).max()
    return float(rot), float(direction), float(points)


def model_errors(e, pr, truth):
    K = np.array([[G.KITTI[0], 0, G.KITTI[2]], [0, G.KITTI[1], G.KITTI[3]], [0, 0, 1]])
    if truth["plane"] is not None:
        n, d = truth["plane"]
        Ht = K @ (truth["R"] + np.outer(truth["t"], n) / d) @ np.linalg.inv(K); Ht /= np.linalg.norm(Ht)
        H = e["H21"].astype(np.float64).reshape(3, 3); H /= np.linalg.norm(H)
        return "H", min(np.abs(H - Ht).max(), np.abs(H + Ht).max())
    F = e["F21"].astype(np.float64).reshape(3, 3)
    m, i1, i2 = R.pack_matches(pr["keys1"], pr["keys2"], pr["matches12"])
    x1 = np.stack([m[0], m[1], np.ones(len(i1))], axis=1).astype(np.float64); x2 = np.stack([m[2], m[3], np.ones(len(i1))], axis=1).astype(np.float64)
    l2 = x1 @ F.T; l1 = x2 @ F
    d2 = np.abs((l2 * x2).sum(1)) / np.hypot(l2[:, 0], l2[:, 1]); d1 = np.abs((l1 * x1).sum(1)) / np.hypot(l1[:, 0], l1[:, 1])
    return "F", max(d1.max(), d2.max())


def ground_truth_errors():
    out = dict(H=0.0, F=0.0, rot=0.0, direction=0.0, points=0.0)
    for kind, seed, N in TRUTH_SCENES:
        pr, truth = G.scene(seed, N, kind)
        e = R.initialize(pr["keys1"], pr["keys2"], pr["matches12"], pr["K"], R.draws(seed, 1, 200)[0], **G.PARAMS)
        assert e["status"] == R.OK and e["model"] == (0 if kind == "planar" else 1), (kind, seed, N, R.STATUS_NAMES[e["status"]])
        which, err = model_errors(e, pr, truth); out[which] = max(out[which], err)
        rot, direction, points = truth_errors(e["R21"], e["t21"], e["p3d"], e["triangulated"], truth)
        out["rot"] = max(out["rot"], rot); out["direction"] = max(out["direction"], direction); out["points"] = max(out["points"], points)
        assert e["n_triangulated"] > 50
    return out


def test_ground_truth_on_noise_free_scenes():
    g = ground_truth_errors()
    print(g)
    assert g["H"] <= BAR_H and g["F"] <= BAR_F_PX and g["rot"] <= BAR_ROTATION and g["direction"] <= BAR_DIRECTION and g["points"] <= BAR_POINTS


@pytest.mark.parametrize("name", ["general129", "planar65_ok", "general64_ok", "rotation129", "planar65"])
def test_negated_model_gives_the_same_outcome(name):
    c = G.cases()[name]; pr = c["problem"]
    a = G.expected(name)
    b = R.initialize(pr["keys1"], pr["keys2"], pr["matches12"], pr["K"], c["rand"], negate=True, **c["params"])
    # (-E swaps t and -t in DecomposeE, so the winner may sit at another index of the source's order: the counts are compared as a multiset)
    assert a["status"] == b["status"] and sorted(a["n_good"]) == sorted(b["n_good"]) and a["n_good"][a["best_hypothesis"]] == b["n_good"][b["best_hypothesis"]]
    assert np.array_equal(a["triangulated"], b["triangulated"])
    # the decision, R21, t21 and the points do not depend on the sign; their last bits may (the decompositions start from another matrix)
    assert np.abs(a["R21"] - b["R21"]).max() <= 1e-5 and np.abs(a["t21"] - b["t21"]).max() <= 1e-4
    sel = a["triangulated"]
    if sel.any():
        assert (np.linalg.norm(a["p3d"][sel] - b["p3d"][sel], axis=1) / np.linalg.norm(a["p3d"][sel], axis=1)).max() <= 1e-3


def test_every_status_is_reached_by_a_constructed_case():
    want = dict(rotation129=R.LOW_PARALLAX, identity64=R.H_DEGENERATE, rotation65_exact=R.H_DEGENERATE, few40=R.FEW_POINTS, planar65=R.AMBIGUOUS, coincident20=R.NO_MODEL,
                general129=R.OK, planar65_ok=R.OK, general64_ok=R.OK, general65=R.LOW_PARALLAX)
    for name, st in want.items():
        assert G.expected(name)["status"] == st, (name, R.STATUS_NAMES[G.expected(name)["status"]])
    assert G.expected("rotation129")["model"] == 0 and G.expected("few40")["model"] == 1 and G.expected("few40")["n_matches"] == 40
    e = G.expected("coincident20")
    assert np.isnan(e["rh"]) and np.isnan(e["scores"]).all() and e["best_it_h"] == -1 and not e["H21"].any()
    # the scene choice: general scenes are far below the 0.40 switch, planar and rotating ones far above
    for name in G.cases():
        e = G.expected(name)
        if name.startswith("general") or name.startswith("few"):
            assert e["rh"] < 0.32, (name, e["rh"])
        elif not name.startswith(("coincident", "tie")):
            assert e["rh"] > 0.44, (name, e["rh"])
    # :517 nsimilar > 1 as well
    assert R.decide(1, [60, 50, 0, 0], np.zeros(8, np.float32), 62, 1.0, 50)[0] == R.AMBIGUOUS
    assert R.decide(1, [60, 42, 0, 0], np.full(8, 0.5, np.float32), 62, 1.0, 50)[0] == R.OK


def test_decision_rules_and_quirks():
    f32 = np.float32
    # the else-if chain of :523-567: the first hypothesis that equals maxGood fails the parallax test and no other is tried (reachable where maxGood = 0 passes :517)
    cos = np.array([1.0, 0.5, 0.5, 0.5, 0, 0, 0, 0], f32)
    assert R.decide(1, [0, 0, 0, 0], cos, 1, 1.0, 0) == (R.LOW_PARALLAX, 0, 0)
    assert R.decide(1, [0, 0, 0, 0], cos, 1, -1.0, 0)[0] == R.OK
    # nGood > 0.7 * maxGood and 0.9 * N are double comparisons; static_cast<int>(0.9 * N) truncates
    assert R.decide(1, [10, 7, 0, 0], np.full(8, 0.5, f32), 11, 1.0, 9)[0] == R.OK                                    # 7 > 7.0 is false; int(9.9) = 9
    assert R.decide(1, [10, 8, 0, 0], np.full(8, 0.5, f32), 11, 1.0, 9)[0] == R.AMBIGUOUS
    assert R.decide(1, [9, 0, 0, 0], np.full(8, 0.5, f32), 12, 1.0, 5)[0] == R.FEW_POINTS                            # int(10.8) = 10 > 9
    # ReconstructH: strict > for bestGood (the first of equals stays), secondBestGood < 0.75 * bestGood, bestGood > 0.9 * N, >= for the parallax
    assert R.decide(0, [60, 60, 0, 0, 0, 0, 0, 0], np.full(8, 0.5, f32), 60, 1.0, 50) == (R.AMBIGUOUS, 0, 60)
    assert R.decide(0, [60, 45, 0, 0, 0, 0, 0, 0], np.full(8, 0.5, f32), 60, 1.0, 50)[0] == R.AMBIGUOUS               # 45 < 45.0 is false
    assert R.decide(0, [60, 44, 0, 0, 0, 0, 0, 0], np.full(8, 0.5, f32), 60, 1.0, 50) == (R.OK, 0, 44)
    assert R.decide(0, [54, 0, 0, 0, 0, 0, 0, 0], np.full(8, 0.5, f32), 60, 1.0, 50)[0] == R.FEW_POINTS              # 54 > 54.0 is false
    assert R.decide(0, [50, 0, 0, 0, 0, 0, 0, 0], np.full(8, 0.5, f32), 50, 1.0, 50)[0] == R.FEW_POINTS              # bestGood > minTriangulated
    assert R.decide(0, [0] * 8, np.ones(8, f32), 60, 1.0, 50) == (R.LOW_PARALLAX, -1, 0)
    # several failing tests of :721 at once: parallax first, then the second best
    assert R.decide(0, [60, 60, 0, 0, 0, 0, 0, 0], np.ones(8, f32), 60, 1.0, 50)[0] == R.LOW_PARALLAX
    # parallax: > for F, >= for H, at a cosine whose parallax is exactly minParallax
    c = f32(0.5); p = float(R.parallax_of(c))
    assert R.decide(1, [60, 0, 0, 0], np.full(8, c, f32), 60, p, 50)[0] == R.LOW_PARALLAX and R.decide(0, [60] + [0] * 7, np.full(8, c, f32), 60, p, 50)[0] == R.OK
    # 0.99998 is a double literal compared with a float; a NaN cosine ranks last; the order statistic by (value, position)
    assert np.isnan(R.order_statistic([f32(0.3), f32(np.nan), f32(0.1)])) and R.order_statistic([f32(np.nan)] + [f32(k) / 64 for k in range(64)]) == f32(50) / 64
    assert R.order_statistic([f32(0.5)] * 3 + [f32(0.25)]) == f32(0.5) and R.cos_before(f32(0.5), 0, f32(0.5), 1) and not R.cos_before(f32(0.5), 1, f32(0.5), 0)
    assert R.parallax_of(f32(1)) == 0 and np.isnan(R.parallax_of(f32(1.0000001)))


@pytest.mark.parametrize("size", [1, 50, 51, 52, 60])
def test_order_statistic_on_either_side_of_50(size):
    """vCosParallax of sizes 50, 51 and 52 through CheckRT: min(50, size - 1) is 49, 50 and 50"""
    pr, truth = G.scene(105, 129, "general")
    m, i1, i2 = R.pack_matches(pr["keys1"], pr["keys2"], pr["matches12"])
    inl = np.zeros(129, bool); inl[np.random.default_rng(size).permutation(129)[:size]] = True
    n_good, c, p3d, good, cos = R.check_rt(truth["R"], truth["t"] / np.linalg.norm(truth["t"]), m, i1, inl, pr["K"], len(pr["keys1"]), 1.0)
    assert n_good == size == len(cos)
    assert c == sorted(cos)[min(50, size - 1)]
    # quirks: vP3D and vbGood are indexed by the key-1 index and sized n1; vP3D is written wherever nGood counts
    assert p3d.shape == (len(pr["keys1"]), 3) and set(np.nonzero(p3d.any(axis=1))[0]) == set(i1[inl]) and not good[np.setdiff1d(np.arange(len(good)), i1[inl])].any()


def test_p3d_is_written_where_low_parallax_leaves_good_false():
    pr, truth = G.scene(130, 129, "rotation", 0.5)
    e = G.expected("rotation129")
    m, i1, i2 = R.pack_matches(pr["keys1"], pr["keys2"], pr["matches12"])
    hyps = R.faugeras(R.mul3(R.mul3(R.inv3(np.array([[G.KITTI[0], 0, G.KITTI[2]], [0, G.KITTI[1], G.KITTI[3]], [0, 0, 1]], np.float32)), e["H21"].reshape(3, 3)),
                             np.array([[G.KITTI[0], 0, G.KITTI[2]], [0, G.KITTI[1], G.KITTI[3]], [0, 0, 1]], np.float32)))
    n_good, c, p3d, good, cos = R.check_rt(hyps[0][0], hyps[0][1], m, i1, e["inliers_h"], pr["K"], len(pr["keys1"]), 1.0)
    assert n_good == e["n_good"][0] and n_good > good.sum() and p3d.any(axis=1).sum() == n_good


def test_forced_equal_draws_tie_and_the_earlier_iteration_wins():
    e = G.expected("tie65"); sc = e["scores"]
    assert sc[2].tobytes() == sc[0].tobytes() and sc[3].tobytes() == sc[1].tobytes() and (sc > 0).all()
    assert e["best_it_h"] == int(np.argmax(sc[:2, 0])) and e["best_it_f"] == int(np.argmax(sc[:2, 1]))
    assert R.first_best(np.array([1, 3, 3, 2], np.float32)) == (3, 1) and R.first_best(np.array([np.nan, 0, -1], np.float32))[1] == -1


def test_symbol_is_declared_exported_and_abi_version_stays_6():
    hdr = open(os.path.join(ROOT, "include", "corb_accel.h")).read()
    assert re.search(r"#define CORB_ABI_VERSION 6\b", hdr)
    assert re.search(r"\bint corb_mono_initialize\(const CorbInitProblem\* problems, int n_problems, float sigma, int max_iterations, float min_parallax, int min_triangulated,", hdr)
    for k, name in enumerate(("OK", "NO_MODEL", "H_DEGENERATE", "AMBIGUOUS", "FEW_POINTS", "LOW_PARALLAX")):
        assert re.search(r"#define CORB_INIT_%s\s+%d\b" % (name, k), hdr) and getattr(R, name) == k
    import corbload
    corb = corbload.load_pkg()
    assert "corb_mono_initialize" in corb.EXPORTS
    assert corb.INIT_RESULT_DTYPE == R.RESULT_DTYPE and R.RESULT_DTYPE.itemsize == 264 and C_sizeof(corb._InitProblem) == 56
    fields = re.search(r"typedef struct CorbInitResult \{(.*?)\} CorbInitResult;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n).strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    assert names == list(R.RESULT_DTYPE.names)
    lib = os.path.join(ROOT, "corb-slam_amd", "libcorb_accel.so")
    if os.path.exists(lib):
        import ctypes
        assert hasattr(ctypes.CDLL(lib), "corb_mono_initialize")


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)

"""GPU tests: the Sim3Solver RANSAC on the device (corb_sim3_ransac, corb_sim3_ransac_store, the Sim3Solver class) against tests/sim3solver_reference.py.
(a) every quaternion q_out of a hypothesis whose matrix N has a relative eigen-gap (l1 - l2) / max|l| of at least 2^-10 is within 4 * 2^-23 per component of the top
eigenvector of numpy's float64 eigh of the same float N, up to sign (half a float ulp of a unit vector's component for the rounding, the rest for the conditioning: at
that gap the float64 Jacobi's own 2^-52 / gap stays below 2^-42); at most 5 % of a case's hypotheses may fall under the gap.  (b) counts, R, t, s, flags,
ransac_max_its, the events and their iterations, n_corr / index1 and the scattered vbInliers are bit-equal to the restatement evaluated with the device's q.
(c) the record route equals the host-array route on the same data and changes no record.  (d) the constructor's filter cases."""
import ctypes as C
import numpy as np
import pytest
import sim3solver_reference as R
import gpu_sim3_cases as G

pytestmark = pytest.mark.gpu
BOUND = 4 * 2.0 ** -23


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_q(pr, rv, res, name):
    """bar (a) for the hypotheses of one problem; returns the largest deviation"""
    worst, low = 0.0, 0
    for it in range(res["ransac_max_its"]):
        idx = list(R.draw_triple(rv[it], pr["n"]))
        v, gap = R.eigen_gap(R.horn_N(pr["x1"][idx], pr["x2"][idx])[0])
        if gap < 2.0 ** -10:
            low += 1
            continue
        q = res["q"][it].astype(np.float64)
        worst = max(worst, min(np.abs(q - v).max(), np.abs(q + v).max()))
    assert low <= 0.05 * max(res["ransac_max_its"], 1), name
    return worst


def check_against_restatement(pr, rv, res, case, flags_of=None):
    """(b): everything downstream of the device's q, bit for bit"""
    ref = R.ransac(pr, rv, 0.99, case["min_inliers"], case["max_iterations"], case["fix_scale"], q_dev=res["q"])
    assert res["ransac_max_its"] == ref["cap"]
    assert np.array_equal(res["counts"][: ref["cap"]], ref["counts"]) and not res["counts"][ref["cap"]:].any() and not res["q"][ref["cap"]:].any()
    assert res["n_events"] == len(ref["events"]) and [int(e["iteration"]) for e in res["events"]] == [e["iteration"] for e in ref["events"]][: len(res["events"])]
    for k, (g, e) in enumerate(zip(res["events"], ref["events"])):
        assert g["n_inliers"] == e["n_inliers"]
        assert np.array_equal(_bits(g["R12"]), _bits(e["R"]).reshape(-1)) and np.array_equal(_bits(g["t12"]), _bits(e["t"])) and _bits(g["s12"]) == _bits(e["s"])
        want = e["flags"] if flags_of is None else flags_of(e["flags"])
        assert np.array_equal(res["inliers"][k], want)
    return ref


@pytest.mark.parametrize("name", ["seven", "seven_fix_scale", "three", "n3", "single_iteration", "one_special"])
def test_sim3_ransac_host_arrays(corb, name):
    case = G.host_cases()[name]
    out = corb.Sim3Ransac(case["problems"], case["rand"], 0.99, case["min_inliers"], case["max_iterations"], case["fix_scale"])
    worst = 0.0
    n_ev = []
    for pr, rv, res in zip(case["problems"], case["rand"], out):
        worst = max(worst, check_q(pr, rv, res, name))
        ref = check_against_restatement(pr, rv, res, case)
        n_ev.append(res["n_events"])
    print("%s: largest |q_out -+ eigh| = %.3g (bound %.3g)" % (name, worst, BOUND))
    assert worst <= BOUND
    if name == "seven":            # N = 19 < min: bNoMore at once; N = 20 clean: every count equals min_inliers, no event; N = 21 clean: cap 3, three tied events
        assert [r["ransac_max_its"] for r in out[:3]] == [0, 1, 3] and n_ev[:3] == [0, 0, 3] and out[2]["counts"][:3].tolist() == [21, 21, 21]
    if name == "three":
        assert [r["ransac_max_its"] for r in out] == [35, 300, 300]
    if name == "n3":
        assert out[0]["ransac_max_its"] == 1 and out[0]["counts"][0] == 3 and n_ev == [0]
    if name == "single_iteration":
        assert n_ev == [1] and out[0]["events"][0]["iteration"] == 1
    if name == "one_special":
        r = out[0]
        assert r["counts"][:3].tolist() == [0, 0, 0] and r["n_events"] > 1               # the p1c == p2c triple; z == 0 inside a triple, on either side
        assert np.isnan(ref["events"][0]["R"]).sum() == 0 and not r["inliers"][:, 5].any() and not r["inliers"][:, 9].any()      # z == 0 outside a triple: never an inlier


def test_max_events_and_arguments(corb):
    case = G.host_cases()["seven"]
    full = corb.Sim3Ransac(case["problems"], case["rand"], 0.99, 20, 300, False)
    cut = corb.Sim3Ransac(case["problems"], case["rand"], 0.99, 20, 300, False, max_events=2)
    for f, c in zip(full, cut):
        assert c["n_events"] == f["n_events"] and len(c["events"]) == min(2, f["n_events"])
        assert c["events"].tobytes() == f["events"][:2].tobytes() and np.array_equal(c["inliers"], f["inliers"][:2])
    assert cut[2]["n_events"] == 3
    bad = case["rand"].copy(); bad[3, 17, 1] = -5
    for kw in (dict(rand_values=bad), dict(min_inliers=2), dict(probability=1.0)):
        a = dict(rand_values=case["rand"], probability=0.99, min_inliers=20); a.update(kw)
        with pytest.raises(corb.CorbError, match=r"\(-1\)"):
            corb.Sim3Ransac(case["problems"], a["rand_values"], a["probability"], a["min_inliers"], 300)
    # CORB_ERR_ARG writes nothing
    L = corb.load(); pr = case["problems"][3]
    arr = (corb._Sim3RansacProblem * 1)(corb._Sim3RansacProblem(pr["n"], corb._p(pr["x1"]), corb._p(pr["x2"]), corb._p(pr["sigma2_1"]), corb._p(pr["sigma2_2"]), *[float(k) for k in pr["K1"] + pr["K2"]]))
    rv = np.ascontiguousarray(bad[3]); cap = np.full(1, -7, np.int32); ne = np.full(1, -7, np.int32); ev = np.zeros(4, corb.SIM3_EVENT_DTYPE); fl = np.full((4, pr["n"]), 9, np.uint8)
    assert L.corb_sim3_ransac(C.cast(arr, C.c_void_p), 1, 0.99, 20, 300, 0, corb._p(rv), 4, pr["n"], corb._p(cap), corb._p(ne), corb._p(ev), corb._p(fl), None, None, 0) == -1
    assert cap[0] == -7 and ne[0] == -7 and (fl == 9).all()


def test_sim3solver_class_replays_iterate(corb):
    case = G.host_cases()["seven"]; pr = case["problems"][5]; rv = case["rand"][5]
    res = corb.Sim3Ransac([pr], rv[None], 0.99, 20, 300, False)[0]
    idx1 = np.arange(pr["n"]) * 2 + 1
    for chunk in (5, 1, 300):
        s = corb.Sim3Solver(pr["x1"], pr["x2"], pr["sigma2_1"], pr["sigma2_2"], pr["K1"], pr["K2"], indices1=idx1, n1=2 * pr["n"] + 3, rand_values=rv)
        s.SetRansacParameters(0.99, 20, 300)
        returns = []
        for _ in range(400):
            T, bNoMore, vb, n = s.iterate(chunk)
            if T is not None:
                k = len(returns); e = res["events"][k]; returns.append(s.mnIterations)
                assert n == e["n_inliers"] == vb.sum() and len(vb) == 2 * pr["n"] + 3 and np.array_equal(np.nonzero(vb)[0], idx1[res["inliers"][k]])
                assert np.array_equal(_bits(T[:3, :3]), _bits(e["s12"] * e["R12"].reshape(3, 3))) and np.array_equal(_bits(T[:3, 3]), _bits(e["t12"])) and T[3].tolist() == [0, 0, 0, 1]
                assert np.array_equal(s.GetEstimatedRotation(), e["R12"].reshape(3, 3)) and s.GetEstimatedScale() == e["s12"] and np.array_equal(s.GetEstimatedTranslation(), e["t12"])
            if bNoMore or s.mnIterations >= res["ransac_max_its"]:
                break
        assert returns == R.iterate_literal(res["counts"], res["ransac_max_its"], 20, chunk) == [int(e["iteration"]) for e in res["events"]]
    T, vb, n = corb.Sim3Solver(pr["x1"], pr["x2"], pr["sigma2_1"], pr["sigma2_2"], pr["K1"], pr["K2"], rand_values=rv).find()      # default parameters: (0.99, 6, 300)
    assert T is not None and n == vb.sum() > 6
    small = corb.Sim3Solver(pr["x1"][:5], pr["x2"][:5], pr["sigma2_1"][:5], pr["sigma2_2"][:5], pr["K1"], pr["K2"])
    assert small.iterate(5)[:2] == (None, True)                                  # N < minInliers: bNoMore at once
    seeded = [corb.Sim3Solver(pr["x1"], pr["x2"], pr["sigma2_1"], pr["sigma2_2"], pr["K1"], pr["K2"], seed=3).find()[2] for _ in range(2)]
    assert seeded[0] == seeded[1] > 6


# ---- the record route ----
def _stores(corb, sc):
    kf1, kfs2 = sc["kf1"], sc["kfs2"]
    F = max(len(k["mp_id"]) for k in [kf1] + kfs2) + 3
    KF = corb.KeyFrameStore(len(kfs2) + 2, F); ids = sorted(sc["points"]); MP = corb.MapPointStore(len(ids) + 4, 4)
    for slot, k in enumerate([kf1] + kfs2):
        n = len(k["mp_id"]); kp = np.zeros(n, corb.KP_DTYPE); kp["octave"] = k["octave"]; kp["x"] = np.arange(n); kp["y"] = 7
        KF.put(slot, kp, np.zeros((n, 32), np.uint8), None, None, keyframe_id=k["id"])
        KF.set_meta(slot, id=k["id"], client_id=1, flags=0, fx=k["K"][0], fy=k["K"][1], cx=k["K"][2], cy=k["K"][3], bf=386.0, nlevels=8, Tcw=np.asarray(k["Tcw"], np.float32).reshape(16))
        KF.set_map_points(slot, k["mp_id"])
    rec = np.zeros(len(ids), corb.MP_RECORD_DTYPE); okf, oidx, off = [], [], [0]
    for r, i in zip(rec, ids):
        p = sc["points"][i]
        r["id"] = i; r["world_pos"] = p["pos"]; r["flags"] = corb.MP_BAD if p["bad"] else 0; r["n_obs"] = len(p["obs"]); r["client_id"] = 1
        for k in sorted(p["obs"]):
            okf.append(k); oidx.append(p["obs"][k])
        off.append(len(okf))
    MP.put(0, rec, np.array(off, np.int32), np.array(okf, np.uint64), np.array(oidx, np.uint32))
    MP.build_index(0, len(ids))
    cam = corb.TrackCamera.make(718.856, 718.856, 607.1928, 185.2157, 386.0, 0.537, 0.0, 1241.0, 0.0, 376.0, sc["scale"])
    return KF, MP, cam


def _state(KF, MP, n_slots):
    recs, okf, oi = MP.get(0, MP.capacity)
    return [(KF.get(s)["kp"].tobytes(), KF.get(s)["flags"].tobytes(), KF.get_map_points(s).tobytes(), KF.get_meta(s).tobytes()) for s in range(n_slots)], recs.tobytes(), okf.tobytes(), oi.tobytes()


@pytest.mark.parametrize("n_cand", [1, 3])
def test_sim3_ransac_on_records(corb, n_cand):
    sc = G.record_scene(); KF, MP, cam = _stores(corb, sc)
    case = dict(min_inliers=20, max_iterations=300, fix_scale=False)
    before = _state(KF, MP, 4)
    out = KF.Sim3Ransac(0, list(range(1, n_cand + 1)), MP, cam, [cam] * n_cand, sc["matched"][:n_cand], sc["rand"][:n_cand])
    assert _state(KF, MP, 4) == before                                       # (c) no record changes
    n1 = len(sc["kf1"]["mp_id"]); cs = sc["cases"]; host = []
    for c in range(n_cand):
        pr, idx1 = R.constructor(sc["kf1"], sc["kfs2"][c], sc["points"], sc["matched"][c], sc["scale"], sc["scale"])
        res = out[c]
        assert res["n_corr"] == pr["n"] and np.array_equal(res["index1"], idx1)                         # (d) the filter
        for k in ("bad1", "bad2", "unknown_id", "no_mp1", "not_matched", "not_observing1", "not_observing2"):
            assert cs[k] not in idx1
        k40 = int(np.nonzero(idx1 == cs["other_index"])[0][0])
        assert pr["th1"][k40] == np.floor(9.21 * np.float64(sc["scale"][3] * sc["scale"][3]))            # indexKF1 != i1: the keypoint at the observation's index (octave 3, not 0)
        assert check_q(pr, sc["rand"][c], res, "records") <= BOUND

        def scatter(f, idx1=idx1):
            vb = np.zeros(n1, bool); vb[idx1[f]] = True
            return vb
        ref = check_against_restatement(pr, sc["rand"][c], res, case, flags_of=scatter)
        assert res["n_events"] > 1 and len(res["inliers"][0]) == n1
        host.append(pr)
    # (c) the host-array route on the same data
    hres = corb.Sim3Ransac(host, sc["rand"][:n_cand], 0.99, 20, 300, False)
    for c, (h, r) in enumerate(zip(hres, out)):
        idx1 = r["index1"]
        assert h["ransac_max_its"] == r["ransac_max_its"] and h["n_events"] == r["n_events"] and np.array_equal(h["counts"], r["counts"]) and np.array_equal(_bits(h["q"]), _bits(r["q"]))
        assert h["events"].tobytes() == r["events"].tobytes()
        assert all(np.array_equal(np.nonzero(vb)[0], idx1[f]) for vb, f in zip(r["inliers"], h["inliers"]))
    with pytest.raises(corb.CorbError, match=r"\(-1\)"):
        KF.Sim3Ransac(0, [0], MP, cam, [cam], sc["matched"][:1], sc["rand"][:1])                         # keyframe 1 as its own candidate
    with pytest.raises(corb.CorbError, match=r"\(-1\)"):
        KF.Sim3Ransac(0, [4], MP, cam, [cam], sc["matched"][:1], sc["rand"][:1])                         # an empty slot
    KF.close(); MP.close()

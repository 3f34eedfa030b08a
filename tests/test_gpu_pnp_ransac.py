"""GPU tests: the PnPsolver RANSAC on the device (corb_pnp_ransac, the PnPsolver class) against tests/pnpsolver_reference.py, with no tolerance anywhere.
(a) pose_out and refine_pose_out -- R, t, the three reprojection errors and the chosen N of every hypothesis and of every record's Refine() -- are bit-equal to the
restatement's (any NaN equal to any NaN: payloads are not part of a reading).  (b) independently, counts, both flag sets, n_records and every CorbPnPRansacRecord field,
ransac_max_its and ransac_min_inliers, and on records n_corr, index and the scattered flags, are bit-equal to the restatement evaluated with the device's R and t: a decomposition mismatch shows in (a), a mistake in
CheckInliers or the rule in (b).  (c) max_records, the argument errors, the Python class against the stateful emulation of iterate().  (d) the record route: the constructor's filter cases, equality with
the host-array route on the same data, and stores that are byte-identical before and after."""
import ctypes as C
import numpy as np
import pytest
import pnpsolver_reference as R
import gpu_pnp_cases as G

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(corb, case, **kw):
    p = dict(case["params"]); p.update(kw)
    return corb.PnPRansac(case["problems"], case["rand"], tail_iterations=case["tail"], **p)


def check_problem(pr, rv, res, case, name, flags_of=lambda f: f):
    p = case["params"]
    own = R.ransac(pr, rv, tail_iterations=case["tail"], **p)
    its = own["its"]
    # (a) the device's poses against the restatement's own
    assert res["ransac_max_its"] == own["cap"] and res["ransac_min_inliers"] == own["m"], name
    bad = [i for i in range(its) if not R.same_bits(res["pose"][i], own["pose"][i])]
    assert not bad, (name, pr["n"], bad[:5], res["pose"][bad[0]], own["pose"][bad[0]])
    assert not res["pose"][its:].any() and not res["counts"][its:].any()
    # (b) everything downstream of the device's poses
    dev_ref = {int(e["iteration"]) - 1: res["refine_pose"][k] for k, e in enumerate(res["records"])}
    first = R.ransac(pr, rv, tail_iterations=case["tail"], pose_dev=res["pose"][:its], **p)
    assert np.array_equal(res["counts"][:its], first["counts"]), name
    assert res["n_records"] == len(first["records"]) and [int(e["iteration"]) - 1 for e in res["records"]] == [r["i"] for r in first["records"]], name
    ref = R.ransac(pr, rv, tail_iterations=case["tail"], pose_dev=res["pose"][:its], refine_dev=dev_ref, **p)
    for k, (g, e) in enumerate(zip(res["records"], ref["records"])):
        assert R.same_bits(res["refine_pose"][k], e["pose"]), (name, pr["n"], k, res["refine_pose"][k], e["pose"])             # (a) for Refine()
        assert g["n_inliers"] == e["n_inliers"] and g["n_refined"] == e["n_refined"] and bool(g["refine_ok"]) == e["refine_ok"], (name, k)
        for got, want in ((g["Tcw_best"], e["Tcw_best"]), (g["Tcw_refined"], e["Tcw_refined"])):
            assert np.array_equal(_bits(got)[~np.isnan(got)], _bits(want)[~np.isnan(want)]) and np.array_equal(np.isnan(got), np.isnan(want)), (name, k)
        assert np.array_equal(res["best_inliers"][k], flags_of(e["flags"])) and np.array_equal(res["refined_inliers"][k], flags_of(e["refined_flags"])), (name, k)
    return ref


@pytest.mark.parametrize("name", ["eight", "eight_tail", "single_iteration", "min_set_6", "epsilon_02", "special", "refine_sets"])
def test_pnp_ransac_host_arrays(corb, name):
    case = G.host_cases()[name]
    out = run(corb, case)
    refs = [check_problem(pr, rv, res, case, name) for pr, rv, res in zip(case["problems"], case["rand"], out)]
    caps = [r["ransac_max_its"] for r in out]
    if name in ("eight", "eight_tail"):          # N = 9 < m: bNoMore with no hypothesis; N = 10 == m: cap 1; epsilon 0.5: cap 35
        assert caps == [0, 1, 4, 35, 35, 35, 35, 35] and out[0]["n_records"] == 0 and not out[0]["counts"].any()
        assert [r["ransac_min_inliers"] for r in out] == [10, 10, 10, 31, 32, 32, 64, 150]
        assert sum(r["n_records"] for r in out) >= 3
    if name == "single_iteration":
        assert caps == [1, 1]
    if name == "epsilon_02":
        assert caps == [300, 300] and [r["n_records"] for r in out] == [4, 5]                              # the cap exceeds 35 and several records occur
    if name == "special":
        r = out[0]
        assert np.isnan(r["pose"][3, :12]).any() and r["counts"][3] == 0 and r["counts"][1] == 0          # the four equal correspondences; the duplicated point
        assert not r["best_inliers"][:, 20].any() and not r["refined_inliers"][:, 20].any()                # the correspondence on sample 2's camera plane
    if name == "refine_sets":
        assert [int(r["records"][0]["n_inliers"]) for r in out] == [10, 64, 65] and [int(r["records"][0]["iteration"]) for r in out] == [1, 1, 1]
        assert [bool(r["records"][0]["refine_ok"]) for r in out] == [False, False, True]


def test_max_records_and_arguments(corb):
    case = G.host_cases()["eight"]
    full = run(corb, case)
    cut = run(corb, case, max_records=1)
    assert max(f["n_records"] for f in full) > 1
    for f, c in zip(full, cut):
        assert c["n_records"] == f["n_records"] and len(c["records"]) == min(1, f["n_records"])
        assert c["records"].tobytes() == f["records"][:1].tobytes() and np.array_equal(c["best_inliers"], f["best_inliers"][:1]) and np.array_equal(c["counts"], f["counts"])
    # every CORB_ERR_ARG case leaves the outputs untouched
    L = corb.load(); pr = case["problems"][3]; n = pr["n"]
    prob = corb._PnPRansacProblem(n, *[corb._p(pr[k]) for k in ("p3dw", "p2d", "sigma2")], *[float(k) for k in pr["K"]])
    rv = np.ascontiguousarray(case["rand"][3], np.int32).copy()
    bad_rv = rv.copy(); bad_rv[7, 1] = -1
    good = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, tail=0, rv=rv)
    for change in (dict(min_set=3), dict(min_set=9), dict(min_inliers=3), dict(probability=0.0), dict(probability=1.0), dict(epsilon=0.0), dict(epsilon=1.5),
                   dict(max_iterations=0), dict(max_iterations=65536), dict(tail=-1), dict(tail=65536), dict(rv=bad_rv)):
        a = dict(good); a.update(change)
        total = max(a["max_iterations"], 1) + max(a["tail"], 0)
        rvx = a["rv"] if total * a["min_set"] <= a["rv"].size else np.zeros((total, max(a["min_set"], 1)), np.int32)
        outs = [np.full(1, 77, np.int32) for _ in range(3)] + [np.full(2 * corb.PNP_RECORD_DTYPE.itemsize, 0x55, np.uint8), np.full((2, n), 0x55, np.uint8),
                                                                 np.full((2, n), 0x55, np.uint8), np.full(min(total, 70000), 77, np.int32)]
        before = [o.tobytes() for o in outs]
        rc = L.corb_pnp_ransac(C.byref(prob), 1, a["probability"], a["min_inliers"], a["max_iterations"], a["min_set"], a["epsilon"], 5.991, a["tail"], corb._p(rvx), 2, n,
                               *[corb._p(o) for o in outs[:6]], None if total > 70000 else corb._p(outs[6]), None, None, 0)
        assert rc != 0 and [o.tobytes() for o in outs] == before, change


def test_pnpsolver_class_replays_iterate(corb):
    """PnPsolver.iterate(5) called repeatedly equals the stateful emulation of iterate() call by call, on sequences with several records, a failing Refine() and calls that
    straddle the cap"""
    seen = set()
    for name, k in (("eight", 4), ("eight_tail", 3), ("refine_sets", 0), ("refine_sets", 2), ("min_set_6", 1), ("eight", 6)):
        case = G.host_cases()[name]; pr = case["problems"][k]; p = case["params"]; tail = 12
        rv = np.concatenate([case["rand"][k], R.draws(31, 1, tail, p["min_set"])[0]])[: p["max_iterations"] + tail]
        s = corb.PnPsolver(pr["p3dw"], pr["p2d"], pr["sigma2"], pr["K"], rand_values=rv, tail_iterations=tail)
        s.SetRansacParameters(p["probability"], p["min_inliers"], p["max_iterations"], p["min_set"], p["epsilon"], p["th2"])
        res = s._run(); cap, m = res["ransac_max_its"], res["ransac_min_inliers"]
        counts = res["counts"][: cap + tail]
        ok = {int(e["iteration"]) - 1: bool(e["refine_ok"]) for e in res["records"]}
        calls = [5] * 9                                                  # 35 = 7 x 5: call 7 straddles nothing, the calls behind it run into the tail
        want = R.iterate_literal(list(counts) + [0] * 64, ok, m, cap, calls)          # (what lies behind the evaluated hypotheses is never compared)
        for n_it, (kind, rec, mn, no_more) in zip(calls, want):
            if mn > cap + tail:
                break
            T, bNoMore, vb, nInl = s.iterate(n_it)
            seen.add(kind)
            assert s.mnIterations == mn and bNoMore == no_more, (name, k, kind, mn)
            if kind is None:
                assert T is None and nInl == 0 and not vb.any()
                continue
            e = [x for x in res["records"] if int(x["iteration"]) - 1 == rec][0]
            j = [int(x["iteration"]) - 1 for x in res["records"]].index(rec)
            key = "Tcw_refined" if kind == "refined" else "Tcw_best"
            assert np.array_equal(_bits(T[:3]).reshape(-1), _bits(e[key])) and T[3].tolist() == [0, 0, 0, 1]
            assert nInl == int(e["n_refined" if kind == "refined" else "n_inliers"])
            assert np.array_equal(vb, res["refined_inliers" if kind == "refined" else "best_inliers"][j])
    assert seen == {"refined", "best", None}


# ---- the record route ----
def _stores(corb, sc):
    n = len(sc["kp"]); F = n + 3
    KF = corb.KeyFrameStore(2, F); ids = sorted(sc["points"]); MP = corb.MapPointStore(len(ids) + 4, 4)
    kp = np.zeros(n, corb.KP_DTYPE); kp["octave"] = sc["octave"]; kp["x"] = sc["kp"][:, 0]; kp["y"] = sc["kp"][:, 1]
    KF.put(0, kp, np.zeros((n, 32), np.uint8), None, None, keyframe_id=11)
    KF.set_meta(0, id=11, client_id=1, flags=0, fx=sc["K"][0], fy=sc["K"][1], cx=sc["K"][2], cy=sc["K"][3], bf=386.0, nlevels=8, Tcw=np.eye(4, dtype=np.float32).reshape(16))
    rec = np.zeros(len(ids), corb.MP_RECORD_DTYPE)
    for r, i in zip(rec, ids):
        p = sc["points"][i]
        r["id"] = i; r["world_pos"] = p["pos"]; r["flags"] = corb.MP_BAD if p["bad"] else 0; r["n_obs"] = 0; r["client_id"] = 1
    MP.put(0, rec, np.zeros(len(ids) + 1, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    MP.build_index(0, len(ids))
    cam = corb.TrackCamera.make(sc["K"][0], sc["K"][1], sc["K"][2], sc["K"][3], 386.0, 0.537, 0.0, 1241.0, 0.0, 376.0, sc["scale"])
    return KF, MP, cam


def _state(KF, MP):
    recs, okf, oi = MP.get(0, MP.capacity)
    return (KF.get(0)["kp"].tobytes(), KF.get(0)["flags"].tobytes(), KF.get_map_points(0).tobytes(), KF.get_meta(0).tobytes()), recs.tobytes(), okf.tobytes(), oi.tobytes()


@pytest.mark.parametrize("n_cand", [1, 3])
def test_pnp_ransac_on_records(corb, n_cand):
    sc = G.record_scene(); KF, MP, cam = _stores(corb, sc); p = sc["params"]
    n1 = len(sc["kp"]); cs = sc["cases"]
    before = _state(KF, MP)
    out = corb.PnPRansacStore(KF, 0, MP, cam, sc["matched"][:n_cand], sc["rand"][:n_cand], tail_iterations=sc["tail"], **p)
    assert _state(KF, MP) == before                                          # no record changes
    host = []
    for c in range(n_cand):
        pr, idx = R.constructor(sc["kp"], sc["octave"], sc["matched"][c], sc["points"], sc["scale"], sc["K"])
        res = out[c]
        assert res["n_corr"] == pr["n"] == n1 - 3 and np.array_equal(res["index"], idx)                      # the filter
        assert all(cs[k] not in idx for k in cs)

        def scatter(f, idx=idx):
            vb = np.zeros(n1, bool); vb[idx[f]] = True
            return vb
        check_problem(pr, sc["rand"][c], res, sc, "records", flags_of=scatter)
        assert len(res["best_inliers"][0]) == n1 if res["n_records"] else True
        host.append(pr)
    assert out[0]["n_records"] >= 1 and bool(out[0]["records"][0]["refine_ok"])
    # the host-array route on the same data
    hres = corb.PnPRansac(host, sc["rand"][:n_cand], tail_iterations=sc["tail"], **p)
    for h, r in zip(hres, out):
        assert h["ransac_max_its"] == r["ransac_max_its"] and h["ransac_min_inliers"] == r["ransac_min_inliers"] and h["n_records"] == r["n_records"]
        assert np.array_equal(h["counts"], r["counts"]) and h["records"].tobytes() == r["records"].tobytes()
        assert h["pose"].tobytes() == r["pose"].tobytes() and h["refine_pose"].tobytes() == r["refine_pose"].tobytes()
        assert all(np.array_equal(np.nonzero(vb)[0], r["index"][f]) for vb, f in zip(r["refined_inliers"], h["refined_inliers"]))
    with pytest.raises(corb.CorbError, match=r"\(-1\)"):
        corb.PnPRansacStore(KF, 1, MP, cam, sc["matched"][:1], sc["rand"][:1], tail_iterations=sc["tail"], **p)          # an empty slot
    KF.close(); MP.close()

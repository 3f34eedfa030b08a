"""The correspondence set the two record routes share (csrc/ransac_common.h: prepare -> scan -> compaction, the read-back, the scatter through the index) at the size
where it can go wrong: n1 = 65 features, so a hypothesis leaves two mask words and the second holds one bit; three candidates and 8 iterations.  Candidate 0 matches
every feature, candidate 1 none (N = 0: nothing runs for it), candidate 2 every other feature.  n_corr, index / index1 (-1 behind N, in arrays the caller did not
preset) and the scattered flags against the numpy definitions, through the record_scene builders and the checks of test_gpu_sim3_ransac / test_gpu_pnp_ransac, bit for
bit.  The CPU test holds that the definitions give N >= min_inliers and an event / a record for candidates 0 and 2: the GPU tests cannot pass by running nothing."""
import ctypes as C
import functools
import numpy as np
import pytest
import sim3solver_reference as RS
import pnpsolver_reference as RP
import gpu_sim3_cases as GS
import gpu_pnp_cases as GP

N1, ITS = 65, 8
SIM3_SEED, PNP_SEED = 702, 701
SIM3 = dict(min_inliers=12, max_iterations=ITS, fix_scale=False)
PNP = dict(GP.PARAMS, max_iterations=ITS, epsilon=0.4)                      # min_inliers 10: mRansacMinInliers = max(int(N * 0.4), 10) = 26 and 13


@functools.lru_cache(maxsize=None)
def sim3_scene():
    """the builder's scene with its filter cases undone, so that the constructor accepts every matched feature: N = 65, 0, 33"""
    sc = dict(GS.record_scene(SIM3_SEED, N1, 3)); cs = sc["cases"]
    pts = {i: dict(p) for i, p in sc["points"].items()}; kf1 = dict(sc["kf1"]); kf1["mp_id"] = kf1["mp_id"].copy(); m = sc["matched"].copy()
    pts[1000 + cs["bad1"]]["bad"] = False; pts[1000 + cs["not_observing1"]]["obs"] = {11: cs["not_observing1"]}; kf1["mp_id"][cs["no_mp1"]] = 1000 + cs["no_mp1"]
    for c in range(3):
        ids2 = sc["kfs2"][c]["mp_id"]
        m[c, cs["unknown_id"]] = ids2[0]; m[c, cs["not_matched"]] = ids2[1]
        for i in ids2:
            pts[int(i)]["bad"] = False; pts[int(i)]["obs"] = {22 + c: int(i) - 500000 - 1000 * c, 5: 1}
    m[1, :] = RS.NO_MAP_POINT
    m[2, 1::2] = RS.NO_MAP_POINT
    sc.update(points=pts, kf1=kf1, matched=m, rand=np.ascontiguousarray(sc["rand"][:, :ITS]))
    sc["expected"] = [RS.constructor(kf1, sc["kfs2"][c], pts, m[c], sc["scale"], sc["scale"]) for c in range(3)]
    return sc


@functools.lru_cache(maxsize=None)
def pnp_scene():
    """the builder's frame and its two rows of points (90 % and 60 % of them seen by the true pose) with the filter cases undone: N = 65, 0, 33"""
    sc = dict(GP.record_scene(PNP_SEED, N1, 2))
    pts = {i: dict(p, bad=False) for i, p in sc["points"].items()}
    m = np.stack([1000 + np.arange(N1), np.zeros(N1), 2000 + np.arange(N1)]).astype(np.uint64)
    m[1, :] = RP.NO_MAP_POINT
    m[2, 1::2] = RP.NO_MAP_POINT
    sc.update(points=pts, matched=m, rand=RP.draws(PNP_SEED, 3, ITS), tail=0, params=PNP)
    sc["expected"] = [RP.constructor(sc["kp"], sc["octave"], m[c], pts, sc["scale"], sc["K"]) for c in range(3)]
    return sc


def test_the_definitions_run_candidates_0_and_2():
    sc = sim3_scene()
    assert [pr["n"] for pr, _ in sc["expected"]] == [N1, 0, 33] and sc["expected"][2][1].max() == 64          # word 1's one bit belongs to feature 64
    for c in (0, 2):
        ref = RS.ransac(sc["expected"][c][0], sc["rand"][c], 0.99, **SIM3)
        assert ref["cap"] == ITS and len(ref["events"]) >= 1
    sc = pnp_scene()
    assert [pr["n"] for pr, _ in sc["expected"]] == [N1, 0, 33] and sc["expected"][2][1].max() == 64
    for c in (0, 2):
        ref = RP.ransac(sc["expected"][c][0], sc["rand"][c], **PNP)
        assert ref["cap"] == ITS and ref["m"] <= sc["expected"][c][0]["n"] and len(ref["records"]) >= 1


def _index_behind_n(ncorr, index, expected):
    for c, (pr, idx) in enumerate(expected):
        assert ncorr[c] == pr["n"] and np.array_equal(index[c, : pr["n"]], idx) and (index[c, pr["n"]:] == -1).all(), c


@pytest.mark.gpu
def test_sim3_record_route(corb):
    import test_gpu_sim3_ransac as T
    sc = sim3_scene(); KF, MP, cam = T._stores(corb, sc)
    out = KF.Sim3Ransac(0, [1, 2, 3], MP, cam, [cam] * 3, sc["matched"], sc["rand"], 0.99, **SIM3)
    for c, (res, (pr, idx1)) in enumerate(zip(out, sc["expected"])):
        assert res["n_corr"] == pr["n"] and np.array_equal(res["index1"], idx1), c
        if c == 1:
            assert res["ransac_max_its"] == 0 and res["n_events"] == 0 and not res["counts"].any() and not res["q"].any() and not res["inliers"].any()
            continue

        def scatter(f, idx1=idx1):
            vb = np.zeros(N1, bool); vb[idx1[f]] = True
            return vb
        T.check_against_restatement(pr, sc["rand"][c], res, SIM3, flags_of=scatter)
        assert res["ransac_max_its"] == ITS and res["counts"].any()
    assert out[0]["n_events"] >= 1 and out[0]["inliers"].shape[1:] == (N1,)
    # the same call into arrays that hold something else: the library presets n_corr and index itself
    p = corb._p; sl = np.array([1, 2, 3], np.int32); cams = (corb.TrackCamera * 3)(cam, cam, cam); ids = np.ascontiguousarray(sc["matched"]); rv = np.ascontiguousarray(sc["rand"], np.int32)
    cap = np.zeros(3, np.int32); n_ev = np.zeros(3, np.int32); ev = np.zeros((3, ITS), corb.SIM3_EVENT_DTYPE); fl = np.zeros((3, ITS, N1), np.uint8)
    nc = np.full(3, -7, np.int32); ix = np.full((3, N1), 9, np.int32)
    rc = corb.load().corb_sim3_ransac_store(KF.h, 0, p(sl), 3, MP.h, C.byref(cam), C.cast(cams, C.c_void_p), p(ids), 0.99, SIM3["min_inliers"], ITS, 0, p(rv), ITS, p(cap), p(n_ev), p(ev), p(fl), p(nc), p(ix),
                                            None, None)
    assert rc == 0
    _index_behind_n(nc, ix, sc["expected"])
    assert [int(x) for x in n_ev] == [r["n_events"] for r in out] and all(np.array_equal(fl[c, : len(r["inliers"])].astype(bool), r["inliers"]) for c, r in enumerate(out))
    KF.close(); MP.close()


@pytest.mark.gpu
def test_pnp_record_route(corb):
    import test_gpu_pnp_ransac as T
    sc = pnp_scene(); KF, MP, cam = T._stores(corb, sc)
    out = corb.PnPRansacStore(KF, 0, MP, cam, sc["matched"], sc["rand"], tail_iterations=0, **PNP)
    for c, (res, (pr, idx)) in enumerate(zip(out, sc["expected"])):
        assert res["n_corr"] == pr["n"] and np.array_equal(res["index"], idx), c
        if c == 1:
            assert res["ransac_max_its"] == 0 and res["n_records"] == 0 and not res["counts"].any() and not res["pose"].any()
            continue

        def scatter(f, idx=idx):
            vb = np.zeros(N1, bool); vb[idx[f]] = True
            return vb
        T.check_problem(pr, sc["rand"][c], res, sc, "corr set %d" % c, flags_of=scatter)
        assert res["ransac_max_its"] == ITS and res["counts"].any()
    assert out[0]["n_records"] >= 1 and out[0]["best_inliers"].shape[1:] == (N1,)
    p = corb._p; ids = np.ascontiguousarray(sc["matched"]); rv = np.ascontiguousarray(sc["rand"], np.int32)
    cap = np.zeros(3, np.int32); mi = np.zeros(3, np.int32); n_rec = np.zeros(3, np.int32); rec = np.zeros((3, ITS), corb.PNP_RECORD_DTYPE)
    bf = np.zeros((3, ITS, N1), np.uint8); rf = np.zeros((3, ITS, N1), np.uint8); nc = np.full(3, -7, np.int32); ix = np.full((3, N1), 9, np.int32)
    rc = corb.load().corb_pnp_ransac_store(KF.h, 0, MP.h, C.byref(cam), p(ids), 3, PNP["probability"], PNP["min_inliers"], ITS, PNP["min_set"], PNP["epsilon"], PNP["th2"], 0, p(rv), ITS,
                                           p(cap), p(mi), p(n_rec), p(rec), p(bf), p(rf), p(nc), p(ix), None, None, None)
    assert rc == 0
    _index_behind_n(nc, ix, sc["expected"])
    assert [int(x) for x in n_rec] == [r["n_records"] for r in out]
    assert all(np.array_equal(bf[c, : r["n_records"]].astype(bool), r["best_inliers"]) and np.array_equal(rf[c, : r["n_records"]].astype(bool), r["refined_inliers"]) for c, r in enumerate(out))
    KF.close(); MP.close()

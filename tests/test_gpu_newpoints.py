"""GPU tests: LocalMapping::CreateNewMapPoints on the device (corb_triangulate_pairs, corb_create_new_map_points_store) against tests/newpoints_reference.py.
(a) every SVD-branch point is within 4 * 2^-23 * |x3D|_inf per component of an independent float64 SVD of the same float32 A (one float ulp each for rounding v_i and
v_3, half for the division, rounded up; the FP64 Jacobi's own error is below 1e-12 at the scene's parallaxes); (b) status, source, n_new and the stereo-branch points are
bit-equal to the numpy restatement evaluated with the device's SVD points.  Together they pin every output."""
import ctypes as C
import numpy as np
import pytest
import newpoints_reference as R

pytestmark = pytest.mark.gpu
BOUND = 4 * 2.0 ** -23


@pytest.fixture(scope="module")
def mixed():
    return R.mixed_pairs(11, 257)


def check_points(kf1, kf2, pairs, x3d, status, source):
    """bound (a) for every pair with source 0 and a computed x3D"""
    worst = 0.0
    for (a, b), x, st, src in zip(pairs, x3d, status, source):
        if src != 0 or st in (R.NO_PARALLAX, R.W_ZERO):
            continue
        v = R.svd_point(R.matrix_A(kf1, kf2, int(a), int(b)))
        err = np.abs(x.astype(np.float64) - v[:3] / v[3]).max() / np.abs(x).max()
        worst = max(worst, err)
    print("largest |x3D - svd_point| / |x3D|_inf = %.3g (bound %.3g)" % (worst, BOUND))
    assert worst <= BOUND


@pytest.mark.parametrize("n_pairs", [0, 1, 63, 64, 65, 257])
def test_triangulate_pairs(corb, mixed, n_pairs):
    kf1, kf2, pairs = mixed
    pairs = pairs[:n_pairs]
    x3d, st, src, n_new = corb.TriangulatePairs(kf1, kf2, pairs)
    assert len(x3d) == n_pairs
    check_points(kf1, kf2, pairs, x3d, st, src)
    rx, rst, rsrc = R.decide(kf1, kf2, pairs, x3d_svd=x3d)
    assert np.array_equal(st, rst) and np.array_equal(src, rsrc) and n_new == int((rst == R.OK).sum())
    assert np.array_equal(x3d.view(np.uint32), rx.view(np.uint32))
    if n_pairs == 257:
        assert set(st.tolist()) == {0, 1, 3, 4, 5, 6, 7} and set(src.tolist()) == {0, 1, 2}


def test_w_zero_and_arguments(corb):
    """a degenerate `pose` whose first column is zero makes A's first column zero: v = e1, w == 0 (LocalMapping.cc:310)"""
    k1, k2, pairs, names = R.status_cases()
    T = np.zeros((4, 4), np.float32); T[1, 1] = T[2, 2] = T[3, 3] = 1
    for k in (k1, k2):
        k["Tcw"] = T.copy()
    k2["Tcw"][1, 3] = 0.5
    k1["kp"]["y"][0] = k1["cy"]; k2["kp"]["y"][0] = np.float32(k2["cy"]) + np.float32(0.5) * np.float32(k2["fy"])
    x3d, st, src, n_new = corb.TriangulatePairs(k1, k2, pairs[:1])
    assert st[0] == R.W_ZERO and src[0] == 0 and not x3d.any() and n_new == 0
    assert not R.matrix_A(k1, k2, 0, 0)[:, 0].any() and R.decide_pair(k1, k2, 0, 0)[1] == R.W_ZERO
    with pytest.raises(corb.CorbError):
        corb.TriangulatePairs(k1, k2, [[0, len(k2["kp"])]])


def _cam(corb, k):
    return corb.TrackCamera.make(float(k["fx"]), float(k["fy"]), float(k["cx"]), float(k["cy"]), float(k["bf"]), float(k["mb"]), 0.0, 1241.0, 0.0, 376.0, k["scale"])


def _fill(corb, cur, nbs, F=256):
    kf = corb.KeyFrameStore(len(nbs) + 2, F)
    for slot, k in enumerate([cur] + list(nbs)):
        m = np.zeros((), corb.KF_META_DTYPE)
        m["id"] = k["id"]; m["client_id"] = 1; m["nlevels"] = 8; m["Tcw"] = np.asarray(k["Tcw"], np.float32).reshape(16)
        for f in ("fx", "fy", "cx", "cy", "bf"):
            m[f] = k[f]
        m["inv_level_sigma2"][:8] = 1 / (k["scale"] * k["scale"])
        kf.put_frame(slot, k["kp"], k["desc"], k["u_right"], k["depth"], m); kf.set_bow(slot, k["fv"]); kf.set_flags(slot, k["has_mp"])
    return kf


def _state(kf, mp, n_slots):
    recs, okf, oi = mp.get(0, mp.capacity)
    return [(kf.get(s)["flags"].copy(), kf.get_map_points(s)) for s in range(n_slots)], recs.tobytes(), okf.copy(), oi.copy()


@pytest.fixture(scope="module")
def record_scene():
    cur, nbs, truth, W = R.scene(21, 200, 3, mismatch_frac=0.3)
    cur["has_mp"][::7] = 1                                  # features that hold a map point already
    FE = [R.compute_F12(cur, nb) for nb in nbs]
    return cur, nbs, [f for f, _ in FE], [e for _, e in FE]


@pytest.mark.parametrize("n_nb", [0, 1, 3])
def test_create_new_map_points_store(corb, pyorc, record_scene, n_nb):
    cur, nbs, F12, ep = record_scene
    nbs, F12, ep = nbs[:n_nb], F12[:n_nb], ep[:n_nb]
    kf = _fill(corb, cur, nbs); mp = corb.MapPointStore(400, 4); cam = _cam(corb, cur)
    slots = list(range(1, n_nb + 1))
    before = _state(kf, mp, n_nb + 1)
    out = kf.CreateNewMapPoints(0, slots, F12, ep, cam)
    after = _state(kf, mp, n_nb + 1)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(before[0], after[0])) and before[1] == after[1]      # apply = 0: nothing changes
    dev = {}
    for j in range(n_nb):
        for p in range(out["pair_offset"][j], out["pair_offset"][j + 1]):
            if out["source"][p] == 0:
                dev[(j, int(out["pairs"][p, 0]), int(out["pairs"][p, 1]))] = out["x3d"][p]
    ref = R.create_new_map_points(pyorc, cur, nbs, F12, ep, x3d_svd=dev, first_mp_id=5000, client_id=3)
    assert np.array_equal(out["pair_offset"], ref["pair_offset"]) and np.array_equal(out["pairs"], ref["pairs"])
    assert np.array_equal(out["status"], ref["status"]) and np.array_equal(out["source"], ref["source"]) and out["n_new"] == ref["n_new"]
    assert np.array_equal(out["x3d"].view(np.uint32), ref["x3d"].view(np.uint32))
    for j in range(n_nb):
        s = slice(out["pair_offset"][j], out["pair_offset"][j + 1])
        check_points(cur, nbs[j], out["pairs"][s], out["x3d"][s], out["status"][s], out["source"][s])
        hx, hst, hsrc, hn = corb.TriangulatePairs(cur, nbs[j], out["pairs"][s])          # the host-array form on the same data
        assert np.array_equal(hx.view(np.uint32), out["x3d"][s].view(np.uint32)) and np.array_equal(hst, out["status"][s]) and np.array_equal(hsrc, out["source"][s])
    if n_nb == 3:
        # the seed holds both couplings between neighbours: a feature accepted at its first neighbour (and absent afterwards), and one rejected there and accepted later
        first = {}
        for j in range(n_nb):
            for p in range(ref["pair_offset"][j], ref["pair_offset"][j + 1]):
                first.setdefault(int(ref["pairs"][p, 0]), []).append((j, int(ref["status"][p])))
        assert any(v[0][1] == R.OK and len(v) == 1 for v in first.values())
        assert any(len(v) >= 2 and v[0][1] != R.OK and v[1][1] == R.OK for v in first.values())
        assert all(st != R.OK for v in first.values() for _, st in v[:-1])
    # too small a map store: CORB_ERR_CAPACITY, nothing written
    if ref["n_new"] > 1:
        with pytest.raises(corb.CorbError, match=r"\(-2\)"):
            kf.CreateNewMapPoints(0, slots, F12, ep, cam, mp_store=mp, first_mp_slot=mp.capacity - ref["n_new"] + 1, first_mp_id=5000, client_id=3, apply=True)
        again = _state(kf, mp, n_nb + 1)
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(before[0], again[0])) and before[1] == again[1]
    first_slot = 7
    got = kf.CreateNewMapPoints(0, slots, F12, ep, cam, mp_store=mp, first_mp_slot=first_slot, first_mp_id=5000, client_id=3, apply=True)
    assert all(np.array_equal(got[k], out[k]) for k in ("pair_offset", "pairs", "status", "source")) and np.array_equal(got["x3d"].view(np.uint32), out["x3d"].view(np.uint32))
    recs, okf, oi = mp.get(0, mp.capacity)
    n_new = ref["n_new"]
    for k, r in enumerate(ref["records"]):
        g = recs[first_slot + k]
        assert g["id"] == r["id"] and g["ref_kf_id"] == r["ref_kf_id"] and g["client_id"] == 3 and g["n_obs"] == 2 and g["flags"] == 0
        assert [(int(okf[first_slot + k, q]), int(oi[first_slot + k, q])) for q in range(2)] == r["obs"]
        assert np.array_equal(g["descriptor"], r["descriptor"])
        for f in ("world_pos", "normal"):
            assert np.array_equal(g[f].view(np.uint32), r[f].view(np.uint32)), f
        assert np.float32(g["min_distance"]).view(np.uint32) == np.float32(r["min_distance"]).view(np.uint32) and np.float32(g["max_distance"]).view(np.uint32) == np.float32(r["max_distance"]).view(np.uint32)
    if n_new:
        c = mp.get_counters(first_slot, n_new)
        assert not c["n_visible"].any() and not c["n_found"].any() and not c["replaced_by"].any()
    zero = np.zeros(1, corb.MP_RECORD_DTYPE).tobytes()
    assert all(recs[s].tobytes() == zero for s in range(mp.capacity) if not first_slot <= s < first_slot + n_new)        # every other record is untouched
    for s in range(n_nb + 1):
        g = kf.get(s)
        assert np.array_equal(g["flags"], ref["flags"][s]) and np.array_equal(kf.get_map_points(s), ref["mp_ids"][s])
    scale = cur["scale"]
    for j in range(n_nb):
        pr, n = kf.SearchForTriangulation(0, kf, slots[j], F12[j], float(ep[j][0]), float(ep[j][1]), scale, scale * scale, False, checkOri=False)
        assert not ref["flags"][0][pr.reshape(-1, 2)[:, 0]].any()
    kf.close(); mp.close()


def test_create_new_map_points_arguments(corb, record_scene):
    cur, nbs, F12, ep = record_scene
    kf = _fill(corb, cur, nbs[:1]); cam = _cam(corb, cur); L = corb.load()
    off = np.zeros(4, np.int32); pr = np.zeros((400, 2), np.int32); x = np.zeros((400, 3), np.float32); st = np.zeros(400, np.uint8); src = np.zeros(400, np.uint8); nn = C.c_int(0)
    F = np.ascontiguousarray(F12[0], np.float32); e = np.asarray(ep[0], np.float32)

    def call(cur_slot, nb, n_nb, F12p):
        nb = np.asarray(nb, np.int32)
        return L.corb_create_new_map_points_store(kf.h, cur_slot, corb._p(nb), n_nb, F12p, corb._p(e), C.byref(cam), 0, 0, None, 0, 0, 0, corb._p(off), corb._p(pr), corb._p(x), corb._p(st),
                                                  corb._p(src), C.byref(nn))
    assert call(0, [1], 1, corb._p(F)) == 0
    assert call(0, [2], 1, corb._p(F)) == -1          # an empty slot
    assert call(2, [1], 1, corb._p(F)) == -1
    assert call(0, [1], -1, corb._p(F)) == -1
    assert call(0, [1], 1, None) == -1                # NULL F12
    assert call(0, [0], 1, corb._p(F)) == -1          # the current keyframe as its own neighbour
    kf.close()

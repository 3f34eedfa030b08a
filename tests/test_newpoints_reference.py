"""CPU tests of the numpy restatement of CreateNewMapPoints' triangulation loop (tests/newpoints_reference.py): exact geometry, one case per status and source, and the
w == 0 exit.  The GPU tests (test_gpu_newpoints.py) compare the device against this restatement."""
import collections
import numpy as np
import newpoints_reference as R


def test_exact_geometry_is_triangulated():
    """two KITTI-calibrated keyframes 1 m apart, points at 5-40 m, exact projections: every pair is OK and the SVD branch recovers the world point to 1e-3 relative"""
    k1, k2, pairs, W = R.exact_pair(40, 1)
    X, st, src = R.decide(k1, k2, pairs)
    assert (st == R.OK).all() and (src == 0).all()
    assert (np.abs(X - W).max(axis=1) <= 1e-3 * np.abs(W).max(axis=1)).all()


def test_one_case_per_status_and_source():
    k1, k2, pairs, names = R.status_cases()
    X, st, src = R.decide(k1, k2, pairs)
    got = {n: (int(s), int(r)) for n, s, r in zip(names, st, src)}
    assert got == dict(ok_svd=(R.OK, 0), no_parallax=(R.NO_PARALLAX, 0), source1=(R.OK, 1), source2=(R.OK, 2), both_stereo=(R.OK, 1), behind_1=(R.BEHIND_1, 0),
                       behind_2=(R.BEHIND_2, 1), reproj_1=(R.REPROJ_1, 0), reproj_2=(R.REPROJ_2, 1), scale=(R.SCALE, 0))
    # both sides stereo: only side 1's stereo parallax is evaluated (`else if`, LocalMapping.cc:290) -- side 2 alone gives source 2, both give source 1
    i = names.index("both_stereo"); j = names.index("source2")
    assert k2["u_right"][i] >= 0 and k2["u_right"][j] >= 0 and src[i] == 1 and src[j] == 2
    # x3D is reported for pairs a later test rejects, and not where none was computed
    assert np.abs(X[names.index("reproj_1")]).max() > 0 and np.abs(X[names.index("behind_1")]).max() > 0 and not X[names.index("no_parallax")].any()


def test_mixed_scene_holds_every_status():
    """the scene the GPU test runs: all seven reachable statuses and all three sources occur (counts as constructed for seed 11)"""
    cur, nb, pairs = R.mixed_pairs(11, 257)
    X, st, src = R.decide(cur, nb, pairs)
    assert sorted(collections.Counter(st.tolist()).items()) == [(0, 232), (1, 18), (3, 1), (4, 1), (5, 2), (6, 2), (7, 1)]
    assert sorted(collections.Counter(src.tolist()).items()) == [(0, 123), (1, 85), (2, 49)]


def test_w_zero():
    """:310 needs the null vector's fourth COMPONENT to vanish: a hand-made A whose first column is zero has v = e1, w == 0.  (A zero fourth column gives v = e4, w = 1,
    x3D = 0: the :310 exit is not taken.)"""
    k1, k2, pairs, names = R.status_cases()
    A = np.array([[0, 1, 2, 3], [0, -1, 1, 2], [0, 2, -1, 1], [0, 1, 1, -3]], np.float32)
    v = R.svd_point(A)
    assert abs(abs(v[0]) - 1) < 1e-12 and np.float32(v[3]) == 0
    X, st, src = R.decide_pair(k1, k2, 0, 0, v_svd=v)
    assert st == R.W_ZERO and src == 0 and not X.any()
    v4 = R.svd_point(A[:, ::-1].copy())
    assert abs(abs(v4[3]) - 1) < 1e-12
    X, st, src = R.decide_pair(k1, k2, 0, 0, v_svd=v4)
    assert st != R.W_ZERO and not X.any()


def test_stereo_parallax_is_the_double_angle_cosine():
    for mb, d in ((0.5371657, 6.0), (0.5371657, 0.4), (0.12, 35.5)):
        ref = np.cos(2 * np.arctan2(np.float64(np.float32(mb) / np.float32(2)), np.float64(np.float32(d))))
        assert abs(float(R._cos_stereo(mb, d)) - ref) <= 2.0 ** -24

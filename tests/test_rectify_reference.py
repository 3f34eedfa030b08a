"""CPU tests of the rectifier's definition alone (tests/rectify_reference.py): the weights, the exact cases a reader can check by hand, the rounding rules, the
perturbation of the running sums on the EuRoC maps, and the proof that the GPU tests' inputs (tests/rectify_cases.py) cover the kinds they claim."""
import numpy as np

import rectify_cases as G
import rectify_reference as R

f32, f64 = np.float32, np.float64
K0 = np.array([[512, 0, 256], [0, 512, 128], [0, 0, 1]], f64)


def test_every_weight_set_sums_to_32768():
    ax, ay = np.meshgrid(np.arange(32), np.arange(32))
    w = R.weights(ax, ay)
    assert ax.size == 1024 and (sum(w) == 32768).all() and all((x >= 0).all() for x in w)


def test_identity_calibration_gives_identity_maps_and_a_copy():
    mx, my = R.init_undistort_rectify_map(K0, np.zeros(8), np.eye(3), K0, (67, 45))
    j, i = np.meshgrid(np.arange(67, dtype=f32), np.arange(45, dtype=f32))
    assert np.array_equal(mx, j) and np.array_equal(my, i)
    src = np.random.default_rng(1).integers(0, 256, (45, 67), dtype=np.uint8)
    dst, kind = R.remap(src, mx, my)
    # the last row and column read taps outside with weight 0: still a copy
    assert np.array_equal(dst, src) and R.kind_histogram(kind)[R.INSIDE] == 44 * 66
    # a 3x4 P and its left 3x3 are the same thing
    P = np.concatenate([K0, [[-47.9], [0], [0]]], 1)
    assert all(np.array_equal(a, b) for a, b in zip(R.init_undistort_rectify_map(K0, np.zeros(8), np.eye(3), P, (67, 45)), (mx, my)))
    assert R.init_undistort_rectify_map(K0, np.zeros(8), np.zeros((3, 3)), K0, (8, 8)) is None and R.inverse3(np.ones((3, 3))) is None


def test_integer_and_half_pixel_shifts():
    src = np.random.default_rng(2).integers(0, 256, (31, 41), dtype=np.uint8)
    j, i = np.meshgrid(np.arange(41, dtype=f32), np.arange(31, dtype=f32))
    dst, _ = R.remap(src, j + f32(3), i - f32(2))                          # dst(i, j) = src(i - 2, j + 3)
    want = np.zeros_like(src); want[2:, :38] = src[:29, 3:]
    assert np.array_equal(dst, want)
    dst, _ = R.remap(src, j + f32(0.5), i)
    a = src.astype(int); b = np.concatenate([a[:, 1:], np.zeros((31, 1), int)], 1)
    assert np.array_equal(dst, (a + b + 1) >> 1)
    dst, _ = R.remap(src, j, i + f32(0.5))
    b = np.concatenate([a[1:], np.zeros((1, 41), int)], 0)
    assert np.array_equal(dst, (a + b + 1) >> 1)


def test_rounding_ties_negative_fractions_and_saturation():
    mx = np.array([[16.5 / 32, 17.5 / 32, -0.5, -1.0 / 32, 40000.0, -40000.0, 5 + 31.0 / 32]], f32)
    ix, iy, ax, ay = R.fix_maps(mx, np.zeros_like(mx))
    assert (ix * 32 + ax).tolist()[0][:2] == [16, 18]                      # half to even
    assert (ix[0, 2], ax[0, 2]) == (-1, 16) and (ix[0, 3], ax[0, 3]) == (-1, 31)
    assert (ix[0, 4], ix[0, 5]) == (32767, -32768) and (ix[0, 6], ax[0, 6]) == (5, 31) and not iy.any() and not ay.any()
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 26, -2.0 ** 26):
        assert R.fix_maps(np.array([[bad]], f32), np.zeros((1, 1), f32)) is None and R.fix_maps(np.zeros((1, 1), f32), np.array([[bad]], f32)) is None
    assert R.fix_maps(np.array([[np.nextafter(f32(2.0 ** 26), f32(0))]], f32), np.zeros((1, 1), f32)) is not None


def test_euroc_maps_are_within_one_float_step_of_the_closed_form():
    """The running sums perturb the double by parts in 10^13: only a rounding tie can move the float, and then by one step."""
    l, r, size, s = G.euroc_eyes()
    assert size == (752, 480) and l[1][4:].tolist() == [0, 0, 0, 0] and l[1][0] == -0.28340811 and r[3][3] == -47.90639384423901
    for eye, cal in enumerate((l, r)):
        mx, my = G.euroc_maps(eye)
        assert mx.shape == (480, 752) and mx.dtype == f32
        cx, cy = R.closed_form_map(*cal, size)
        for m, c in ((mx, cx), (my, cy)):
            assert (np.abs(m.astype(f64) - c.astype(f32).astype(f64)) <= np.spacing(np.abs(c).astype(f32)).astype(f64)).all()
            assert np.abs(m.astype(f64) - c).max() < 1e-4                   # and within float rounding of the unrounded value
        # at the principal point a rectifying warp is close to the identity (the lens bends the corners by tens of pixels)
        assert abs(mx[248, 367] - 367) < 16 and abs(my[248, 367] - 248) < 16


def test_small_case_covers_every_kind_it_claims():
    W, H = G.SMALL["raw_width"], G.SMALL["raw_height"]
    for eye in range(2):
        mx, my = G.small_maps(eye)
        assert mx.shape == (G.SMALL["height"], G.SMALL["width"]) and G.SMALL["width"] % 4 and W % 4
        ix, iy, ax, ay = R.fix_maps(mx, my)
        assert (ix[G.TIE_DOWN] * 32 + ax[G.TIE_DOWN], ix[G.TIE_UP] * 32 + ax[G.TIE_UP]) == (10 * 32 + 16, 10 * 32 + 18)
        assert (iy[G.TIE_DOWN] * 32 + ay[G.TIE_DOWN], iy[G.TIE_UP] * 32 + ay[G.TIE_UP]) == (7 * 32 + 16, 7 * 32 + 18)
        assert (ix[G.NEG_FRAC], ax[G.NEG_FRAC]) == (-1, 16) and (ax[G.FRAC_31], ay[G.FRAC_31]) == (31, 31)
        assert ix[G.SAT_HIGH] == 32767 and ix[G.SAT_LOW] == -32768
        assert len(np.unique(ax)) == 32 and len(np.unique(ay)) == 32
    assert not np.array_equal(G.small_maps(0)[0], G.small_maps(1)[0])
    for frame in range(2):
        img, kind = G.small_expected(frame)
        for eye in range(2):
            hist = R.kind_histogram(kind[eye])
            assert (hist >= 1).all() and len(hist) == 13, dict(zip(R.KIND_NAMES, hist.tolist()))
            assert hist[R.INSIDE] > 0.8 * kind[eye].size
            assert (img[eye][kind[eye] >= R.OUT_LEFT] == 0).all() and img[eye].std() > 10
    assert not np.array_equal(G.small_expected(0)[0], G.small_expected(1)[0])


def test_euroc_case_kinds():
    """the EuRoC case of the GPU tests claims the inside kind only: the barrel distortion makes the rectified image read strictly inside the raw one"""
    img, kind = G.euroc_expected()
    for eye in range(2):
        hist = R.kind_histogram(kind[eye])
        assert hist[R.INSIDE] > 0.9 * kind[eye].size and hist.sum() == kind[eye].size, dict(zip(R.KIND_NAMES, hist.tolist()))


def test_settings_parser_reads_matrices_and_scalars():
    s = R.parse_settings(G.EUROC)
    assert s["LEFT.K"].shape == (3, 3) and s["LEFT.D"].shape == (1, 5) and s["RIGHT.P"].shape == (3, 4) and s["LEFT.R"].shape == (3, 3)
    assert s["Camera.bf"] == 47.90639384423901 and s["ORBextractor.nFeatures"] == 1200 and s["LEFT.width"] == 752 and s["Viewer.PointSize"] == 2

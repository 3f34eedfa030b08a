"""CPU tests of the RGB-D / monocular front-end's restatement (tests/cam_reference.py) and of the C-ABI's refusal without a GPU."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cam_reference as R  # noqa: E402


def test_grey_known_answers():
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]]], np.uint8)
    assert R.grey(px, rgb=1).tolist() == [[76, 150, 29, 255, 0]]
    assert R.grey(px, rgb=0).tolist() == [[29, 150, 76, 255, 0]]             # BGR order: the first byte is blue
    rgba = np.concatenate([px, np.full((1, 5, 1), 200, np.uint8)], axis=-1)
    assert R.grey(rgba, rgb=1).tolist() == [[76, 150, 29, 255, 0]]           # alpha ignored
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(R.grey(g), g) and np.array_equal(R.grey(np.stack([g] * 3, -1)), g)


def test_grey_weighs_the_channels_of_the_synthetic_frame(synth):
    c, d = synth.rgbd_frame(0)
    assert c.shape == (480, 640, 3) and d.shape == (480, 640) and d.dtype == np.uint16
    g_rgb, g_bgr = R.grey(c, 1), R.grey(c, 0)
    assert not np.array_equal(g_rgb, g_bgr) and not np.array_equal(g_rgb, c[..., 0])
    assert (d == 0).any() and (d == 65535).any() and ((d > 0) & (d < 50)).any()
    c4, _ = synth.rgbd_frame(0, channels=4)
    assert np.array_equal(R.grey(c4, 1), g_rgb)
    m = synth.mono_frame(0)
    assert m.shape == (480, 752) and m.dtype == np.uint8


def test_depth_scale_rule():
    f, conv = R.depth_scale(5000.0, False)
    assert f == np.float32(1) / np.float32(5000) and conv
    assert R.depth_scale(0.0, False) == (1.0, True)                     # u16 is always converted
    assert R.depth_scale(1e-6, True) == (1.0, False)                    # |factor| < 1e-5 -> 1: an f32 image is used as it is
    assert R.depth_scale(1.0, True) == (1.0, False)
    f, conv = R.depth_scale(2.0, True)
    assert f == np.float32(0.5) and conv


def test_zero_distortion_is_the_identity_and_k1_zero_passes_through():
    rng = np.random.default_rng(3)
    kp = np.zeros(500, R_KP)
    kp["x"] = rng.uniform(0, 640, 500); kp["y"] = rng.uniform(0, 480, 500)
    assert R.keys_un(kp, R.TUM3).tobytes() == kp.tobytes()
    assert R.keys_un(kp, R.QUIRK).tobytes() == kp.tobytes()            # k1 == 0: p1, p2, k2 ignored (Frame.cc:410)
    # the undistortion itself with all-zero coefficients maps a pixel onto itself to within the double round trip
    ux, uy = R.undistort_points(kp["x"], kp["y"], R.TUM3)
    assert np.abs(ux - kp["x"]).max() <= 6.2e-5 and np.abs(uy - kp["y"]).max() <= 3.1e-5


R_KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def test_redistorting_the_undistorted_tum1_keypoints_lands_on_the_input(synth, pyorc):
    """Five fixed-point iterations invert the Brown model closely inside the image: on the synthetic TUM1 frame's 1008 keypoints the largest
    residual observed is 1.6e-3 px, the median 8.9e-6 px (the iteration is least converged near the corners)."""
    c, d = synth.rgbd_frame(0)
    f = R.frame(pyorc.Extractor(nfeatures=1000), c, d, R.TUM1)
    assert len(f["keys"]) > 800
    assert np.abs(f["keys_un"]["x"] - f["keys"]["x"]).max() > 5           # TUM1 is far from the identity
    dx, dy = R.distort_points(f["keys_un"]["x"], f["keys_un"]["y"], R.TUM1)
    r = np.hypot(dx - f["keys"]["x"], dy - f["keys"]["y"])
    assert r.max() < 3e-3 and np.median(r) < 3e-5
    ok = f["depth"] > 0
    assert ok.sum() > 0.5 * len(ok) and (~ok).sum() > 0
    assert np.array_equal(f["u_right"][ok], f["keys_un"]["x"][ok] - np.float32(40.0) / f["depth"][ok])


def test_image_bounds():
    assert R.image_bounds(R.TUM3).tolist() == [0, 640, 0, 480]
    assert R.image_bounds(R.QUIRK).tolist() == [0, 640, 0, 480]
    b = R.image_bounds(R.TUM1)
    assert 0 < b[0] < 20 and 620 < b[1] < 640 and 0 < b[2] < 20 and 460 < b[3] < 480      # barrel-corrected corners move inwards for TUM1
    e = R.image_bounds(R.EUROC)
    assert e[0] < 0 and e[1] > 752 and e[2] < 0 and e[3] > 480                              # EuRoC's pincushion correction moves them out


def test_rgbd_create_without_a_device_fails(corb):
    if corb.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(corb.CorbError):
        corb.RgbdFrontend()
    with pytest.raises(corb.CorbError):
        corb.RgbdFrontend(sensor=corb.SENSOR_MONOCULAR, width=752, height=480, channels=1)

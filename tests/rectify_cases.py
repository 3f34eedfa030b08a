"""Seeded inputs of the rectifier's tests, shared by the CPU test that proves what they cover (tests/test_rectify_reference.py) and the GPU tests that run them
(tests/test_gpu_rectify.py)."""
import os

import numpy as np

import rectify_reference as R

f32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EUROC = os.path.join(GOLD, "EuRoC.yaml")

# the small case: the smallest configuration tests/test_gpu_orb.py runs, both widths no multiple of 4
SMALL = dict(width=129, height=97, raw_width=141, raw_height=103, nlevels=3, nfeatures=300, max_frames=2)
# where the small maps hold their special entries: (row, column) -> what the CPU test checks there
TIE_DOWN, TIE_UP, NEG_FRAC, FRAC_31, SAT_HIGH, SAT_LOW = (20, 10), (20, 11), (30, 0), (20, 12), (10, 5), (10, 6)


def _synth():
    import corbload
    corbload.load_pkg()
    from corb_slam_amd import synth
    return synth


def small_maps(eye):
    """maps of 129 x 97 into a 141 x 103 raw image that cover all thirteen kinds, both rounding ties, a negative fractional coordinate, fraction 31 and a
    coordinate that saturates int16 -- different per eye"""
    w, h, W, H = SMALL["width"], SMALL["height"], SMALL["raw_width"], SMALL["raw_height"]
    rng = np.random.default_rng(7100 + eye)
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    # a mild warp that stays inside, on a 1/32 grid plus off-grid noise (every fraction 0..31 occurs)
    mx = 1.0 + j * ((W - 3.0) / w) + 0.9 * np.sin(i / (11.0 + eye)) + rng.uniform(0, 1, (h, w))
    my = 1.0 + i * ((H - 3.0) / h) + 0.9 * np.cos(j / (13.0 - eye)) + rng.uniform(0, 1, (h, w))
    mx = np.clip(mx, 0, W - 1.001); my = np.clip(my, 0, H - 1.001)
    mx[:, 0] = -0.5; mx[:, 1] = W - 1 + 0.25                    # ix = -1 (ax = 16), ix = W - 1: the partial sides, and with the rows below the corners
    my[0, :] = -0.75; my[1, :] = H - 1 + 0.5                    # iy = -1, iy = H - 1
    mx[:, 2] = -1.5; mx[:, 3] = W + 3.25                        # outside left / right
    my[2, 4:] = -3.0; my[3, 4:] = H + 2.0                       # outside top / bottom
    mx[SAT_HIGH] = 40000.0; mx[SAT_LOW] = -40000.0              # saturates int16
    mx[TIE_DOWN] = 10 + 16.5 / 32; mx[TIE_UP] = 10 + 17.5 / 32; mx[FRAC_31] = 20 + 31.0 / 32
    my[20, 10:13] = [7 + 16.5 / 32, 7 + 17.5 / 32, 7 + 31.0 / 32]
    my[NEG_FRAC] = 40.25
    return mx.astype(f32), my.astype(f32)


def small_raw(frame):
    """[2][103][141] raw pair of `frame`: the synthetic stereo pair at the raw size"""
    return np.ascontiguousarray(np.stack(_synth().stereo_pair(40 + frame, SMALL["raw_width"], SMALL["raw_height"])))


def small_expected(frame):
    """the definition's rectified pair [2][97][129] and the kinds [2][97][129] of the small case"""
    raw = small_raw(frame)
    out = [R.remap(raw[e], *small_maps(e)) for e in range(2)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def euroc_eyes():
    s = R.parse_settings(EUROC)
    return R.eye_from_settings(s, "LEFT"), R.eye_from_settings(s, "RIGHT"), (int(s["LEFT.width"]), int(s["LEFT.height"])), s


EUROC_SEED = 3          # synth.stereo_pair(EUROC_SEED, 752, 480): the oracle alone gives at least 50 stereo matches on its rectified pair (asserted where it is used)
_euroc = {}


def euroc_maps(eye):
    if eye not in _euroc:
        l, r, size, _ = euroc_eyes()
        _euroc[eye] = R.init_undistort_rectify_map(*(l, r)[eye], size)
    return _euroc[eye]


def euroc_raw():
    return np.ascontiguousarray(np.stack(_synth().stereo_pair(EUROC_SEED, 752, 480)))


def euroc_expected():
    """the definition's rectified pair [2][480][752] and its kinds"""
    if "exp" not in _euroc:
        raw = euroc_raw()
        out = [R.remap(raw[e], *euroc_maps(e)) for e in range(2)]
        _euroc["exp"] = (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]))
    return _euroc["exp"]

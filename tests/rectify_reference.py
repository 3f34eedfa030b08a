"""The definition of the stereo rectifier (include/corb_stereo_rectify.h): what Examples/Stereo/stereo_euroc.cc:64-98,136-137 and
Examples/ROS/ORB_SLAM2/src/ros_stereo.cc:82-107,161-162 compute with cv::initUndistortRectifyMap(K, D, R, P, size, CV_32F, M1, M2) and cv::remap(raw, out, M1, M2,
cv::INTER_LINEAR), stated as readings (OpenCV is neither on the test machines nor vendored by the reference; DESIGN.md section 2 repeats the readings).

Maps: float64, one IEEE operation at a time, no fused multiply-add; the running sums along a row are part of the definition, so the column loop is serial and the
rows are vectorised.  The order of every expression is the one of csrc/rectify_math.h."""
import re

import numpy as np

f32, f64 = np.float32, np.float64
MAP_LIMIT = f32(2.0 ** 26)

# kinds of a destination pixel: where its four taps (ix, iy) (ix+1, iy) (ix, iy+1) (ix+1, iy+1) lie with respect to the W x H source
INSIDE = 0
PART_LEFT, PART_RIGHT, PART_TOP, PART_BOTTOM = 1, 2, 3, 4              # two taps inside: ix == -1, ix == W-1, iy == -1, iy == H-1
CORNER_TL, CORNER_TR, CORNER_BL, CORNER_BR = 5, 6, 7, 8               # one tap inside
OUT_LEFT, OUT_RIGHT, OUT_TOP, OUT_BOTTOM = 9, 10, 11, 12              # no tap inside: ix+1 < 0, ix >= W, iy+1 < 0, iy >= H (the first that holds, in this order)
KIND_NAMES = ("inside", "part_left", "part_right", "part_top", "part_bottom", "corner_tl", "corner_tr", "corner_bl", "corner_br",
              "out_left", "out_right", "out_top", "out_bottom")


def p3_times_r(P, R):
    P = np.asarray(P, f64).reshape(3, 4); R = np.asarray(R, f64).reshape(3, 3)
    A = np.zeros((3, 3), f64)
    for r in range(3):
        for c in range(3):
            A[r, c] = (P[r, 0] * R[0, c] + P[r, 1] * R[1, c]) + P[r, 2] * R[2, c]
    return A


def inverse3(A):
    """adjugate times 1 / det, the determinant expanded along the first row; None if it is zero or not finite"""
    a = [f64(v) for v in np.asarray(A, f64).reshape(9)]
    with np.errstate(all="ignore"):
        c00 = a[4] * a[8] - a[5] * a[7]; c01 = a[3] * a[8] - a[5] * a[6]; c02 = a[3] * a[7] - a[4] * a[6]
        det = (a[0] * c00 - a[1] * c01) + a[2] * c02
        if not (det != 0.0) or not np.isfinite(det):
            return None
        i = f64(1.0) / det
        return np.array([c00 * i, (a[2] * a[7] - a[1] * a[8]) * i, (a[1] * a[5] - a[2] * a[4]) * i,
                         (a[5] * a[6] - a[3] * a[8]) * i, (a[0] * a[8] - a[2] * a[6]) * i, (a[2] * a[3] - a[0] * a[5]) * i,
                         c02 * i, (a[1] * a[6] - a[0] * a[7]) * i, (a[0] * a[4] - a[1] * a[3]) * i], f64)


def _distort(x, y, K, D):
    K = np.asarray(K, f64).reshape(9); fx, fy, cx, cy = K[0], K[4], K[2], K[5]
    k1, k2, p1, p2, k3, k4, k5, k6 = (f64(v) for v in np.asarray(D, f64).reshape(8))
    x2 = x * x; y2 = y * y; r2 = x2 + y2; _2xy = 2 * x * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    u = fx * ((x * kr + p1 * _2xy) + p2 * (r2 + 2 * x2)) + cx
    v = fy * ((y * kr + p1 * (r2 + 2 * y2)) + p2 * _2xy) + cy
    return u, v


def init_undistort_rectify_map(K, D, R, P, size):
    """cv::initUndistortRectifyMap(K, D, R, P, (w, h), CV_32F): (map_x, map_y) float32 [h][w]; None if P3x3 R has no inverse.  P: 3x4 (or 3x3)."""
    w, h = size
    P = np.asarray(P, f64)
    P = np.concatenate([P.reshape(3, 3), np.zeros((3, 1))], 1) if P.size == 9 else P.reshape(3, 4)
    iR = inverse3(p3_times_r(P, R))
    if iR is None:
        return None
    i = np.arange(h, dtype=f64)
    _x = i * iR[1] + iR[2]; _y = i * iR[4] + iR[5]; _w = i * iR[7] + iR[8]
    mx = np.zeros((h, w), f32); my = np.zeros((h, w), f32)
    with np.errstate(all="ignore"):
        for j in range(w):
            w_ = 1.0 / _w; x = _x * w_; y = _y * w_
            u, v = _distort(x, y, K, D)
            mx[:, j] = u.astype(f32); my[:, j] = v.astype(f32)
            _x = _x + iR[0]; _y = _y + iR[3]; _w = _w + iR[6]
    return mx, my


def closed_form_map(K, D, R, P, size):
    """the same maps without running sums: _x = j iR[0] + i iR[1] + iR[2] ... (float64 arrays, not rounded) -- the test of the running sums' perturbation"""
    w, h = size
    iR = inverse3(p3_times_r(np.asarray(P, f64).reshape(3, 4), R))
    j, i = np.meshgrid(np.arange(w, dtype=f64), np.arange(h, dtype=f64))
    _x = j * iR[0] + i * iR[1] + iR[2]; _y = j * iR[3] + i * iR[4] + iR[5]; _w = j * iR[6] + i * iR[7] + iR[8]
    return _distort(_x / _w, _y / _w, K, D)


def fix_maps(map_x, map_y):
    """the fixed-point form: (ix, iy int16, ax, ay in 0..31); None if an entry is not finite or its magnitude is 2^26 or more"""
    mx = np.asarray(map_x, f32); my = np.asarray(map_y, f32)
    if not (np.isfinite(mx).all() and np.isfinite(my).all() and (np.abs(mx) < MAP_LIMIT).all() and (np.abs(my) < MAP_LIMIT).all()):
        return None
    sx = np.rint(mx * f32(32)).astype(np.int64); sy = np.rint(my * f32(32)).astype(np.int64)         # the float32 product is exact; rint: half to even
    ix = np.clip(sx >> 5, -32768, 32767).astype(np.int16); iy = np.clip(sy >> 5, -32768, 32767).astype(np.int16)
    return ix, iy, (sx & 31).astype(np.int32), (sy & 31).astype(np.int32)


def weights(ax, ay):
    ax = np.asarray(ax, np.int64); ay = np.asarray(ay, np.int64)
    return 32 * (32 - ax) * (32 - ay), 32 * ax * (32 - ay), 32 * (32 - ax) * ay, 32 * ax * ay


def remap(src, map_x, map_y):
    """cv::remap(src, dst, map_x, map_y, INTER_LINEAR, BORDER_CONSTANT, 0) on an 8-bit one-channel image: (dst uint8 of the maps' shape, kind int8).
    src is W x H, which may differ from the maps' size."""
    src = np.asarray(src, np.uint8); H, W = src.shape
    ix, iy, ax, ay = fix_maps(map_x, map_y)
    ix = ix.astype(np.int64); iy = iy.astype(np.int64)

    def tap(x, y):
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(ok, src[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0).astype(np.int64), ok
    t00, o00 = tap(ix, iy); t01, o01 = tap(ix + 1, iy); t10, o10 = tap(ix, iy + 1); t11, o11 = tap(ix + 1, iy + 1)
    w00, w01, w10, w11 = weights(ax, ay)
    val = (w00 * t00 + w01 * t01 + w10 * t10 + w11 * t11 + 16384) >> 15
    out_l = ix + 1 < 0; out_r = ix >= W; out_t = iy + 1 < 0; out_b = iy >= H
    outside = out_l | out_r | out_t | out_b
    dst = np.where(outside, 0, val).astype(np.uint8)
    kind = np.full(ix.shape, -1, np.int8)
    xl, xr, yt, yb = ix == -1, ix == W - 1, iy == -1, iy == H - 1
    xin, yin = (ix >= 0) & (ix < W - 1), (iy >= 0) & (iy < H - 1)
    kind[xin & yin] = INSIDE
    kind[xl & yin] = PART_LEFT; kind[xr & yin] = PART_RIGHT; kind[xin & yt] = PART_TOP; kind[xin & yb] = PART_BOTTOM
    kind[xl & yt] = CORNER_TL; kind[xr & yt] = CORNER_TR; kind[xl & yb] = CORNER_BL; kind[xr & yb] = CORNER_BR
    for k, m in ((OUT_BOTTOM, out_b), (OUT_TOP, out_t), (OUT_RIGHT, out_r), (OUT_LEFT, out_l)):       # the first that holds wins: written last
        kind[m] = k
    assert (kind >= 0).all()
    n_in = o00.astype(int) + o01 + o10 + o11
    assert ((n_in == 0) == outside).all() or (W < 2 or H < 2)
    return dst, kind


def kind_histogram(kind):
    return np.bincount(np.asarray(kind).reshape(-1).astype(np.int64), minlength=13)


# ---- the settings file (Examples/Stereo/EuRoC.yaml): `LEFT.K: !!opencv-matrix` blocks with rows, cols, dt, data: [...] and plain `KEY: number` entries ----
def parse_settings(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^([A-Za-z_][\w.]*):\s*!!opencv-matrix\s*\n\s*rows:\s*(\d+)\s*\n\s*cols:\s*(\d+)\s*\n\s*dt:\s*(\w)\s*\n\s*data:\s*\[([^\]]*)\]", txt, re.M):
        out[m.group(1)] = np.array([float(v) for v in m.group(5).replace("\n", " ").split(",") if v.strip()], f64).reshape(int(m.group(2)), int(m.group(3)))
    for m in re.finditer(r"^([A-Za-z_][\w.]*):\s*([-+0-9.eE]+)\s*$", txt, re.M):
        out[m.group(1)] = float(m.group(2))
    return out


def eye_from_settings(s, side):
    """(K[9], D[8], R[9], P[12]) of `side` ("LEFT" / "RIGHT"): D zero-filled where the settings give 4 or 5 coefficients"""
    D = np.zeros(8, f64); d = s[side + ".D"].reshape(-1); D[: len(d)] = d
    return s[side + ".K"].reshape(9).copy(), D, s[side + ".R"].reshape(9).copy(), s[side + ".P"].reshape(12).copy()

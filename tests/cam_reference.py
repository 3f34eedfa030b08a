"""CPU restatement of the RGB-D / monocular front-end's per-frame conversions (numpy): the parity partner of corb_rgbd_* beside the oracle's
extractor.  It restates, in the reference's order and arithmetic:

  1. cvtColor RGB2GRAY / BGR2GRAY / RGBA2GRAY / BGRA2GRAY of OpenCV 2.4.8 (RGB2Gray<uchar>): (4899 R + 9617 G + 1868 B + 8192) >> 14
  2. the depth scale of Tracking::GrabImageRGBD (Tracking.cc:141-145, 226-227): Mat::convertTo(CV_32F, f) = (float)src * f + 0.0f per pixel
  4. Frame::UndistortKeyPoints (Frame.cc:408-438): cv::undistortPoints of OpenCV 2.4.8 (cvUndistortPoints) in double, five iterations
  5. Frame::ComputeStereoFromRGBD (Frame.cc:647-668)
  6. Frame::ComputeImageBounds (Frame.cc:440-468)

numpy's float64 / float32 element-wise operations are single IEEE operations (no contraction), so the restatement is bit-exact where the
device's non-fused arithmetic is."""
import numpy as np

# calibrations: the numbers of the reference client's settings files (Examples/RGB-D/TUM{1,2,3}.yaml, Examples/Monocular/EuRoC.yaml)
TUM1 = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, k1=0.262383, k2=-0.953104, p1=-0.005358, p2=0.002628, k3=1.163314,
            bf=40.0, depth_map_factor=5000.0, width=640, height=480)
TUM2 = dict(fx=520.908620, fy=521.007327, cx=325.141442, cy=249.701764, k1=0.231222, k2=-0.784899, p1=-0.003257, p2=-0.000105, k3=0.917205,
            bf=40.0, depth_map_factor=5208.0, width=640, height=480)
TUM3 = dict(fx=535.4, fy=539.2, cx=320.1, cy=247.6, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, bf=40.0, depth_map_factor=5000.0, width=640, height=480)
EUROC = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, k1=-0.28340811, k2=0.07395907, p1=0.00019359, p2=1.76187114e-05, k3=0.0,
             bf=0.0, depth_map_factor=0.0, width=752, height=480)
# artificial: k1 == 0 with tangential terms -- Frame::UndistortKeyPoints passes the keypoints through (and ComputeImageBounds keeps 0, w, 0, h)
QUIRK = dict(TUM3, p1=0.004, p2=-0.003, k2=0.1)

CAM_KEYS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "bf", "depth_map_factor")


def grey(colour, rgb=1):
    """cvtColor to grey as Tracking::GrabImageRGBD picks it: one channel as is; 3 / 4 channels RGB(A) or BGR(A) order by Camera.RGB"""
    c = np.asarray(colour, np.uint8)
    if c.ndim == 2:
        return c.copy()
    s0, s1, s2 = (c[..., i].astype(np.int32) for i in range(3))
    r, b = (s0, s2) if rgb else (s2, s0)
    return ((4899 * r + 9617 * s1 + 1868 * b + 8192) >> 14).astype(np.uint8)


def depth_scale(depth_map_factor, f32_input):
    """(f, convert): f = 1 / DepthMapFactor in float (1 if |DepthMapFactor| < 1e-5); convert unless the input is CV_32F and |f - 1| <= 1e-5"""
    f = np.float32(depth_map_factor)
    f = np.float32(1) if abs(float(f)) < 1e-5 else np.float32(np.float32(1) / f)
    convert = abs(float(np.float32(f - np.float32(1)))) > 1e-5 or not f32_input
    return f, convert


def depth_at(depth, keys, depth_map_factor):
    """the depth Frame::ComputeStereoFromRGBD reads: imDepth.at<float>((int)kp.y, (int)kp.x) of the converted image, at the distorted keypoints"""
    f32_input = depth.dtype == np.float32
    f, convert = depth_scale(depth_map_factor, f32_input)
    raw = depth[keys["y"].astype(np.int32), keys["x"].astype(np.int32)]
    d = raw.astype(np.float32)
    if convert:
        with np.errstate(invalid="ignore", over="ignore"):
            d = d * f + np.float32(0)
    return d.astype(np.float32)


def _k(cam):
    k = np.zeros(8, np.float64)
    k[:4] = [np.float64(np.float32(cam[n])) for n in ("k1", "k2", "p1", "p2")]
    k[4] = np.float64(np.float32(cam.get("k3", 0.0)))
    return k


def undistort_points(x, y, cam):
    """cv::undistortPoints(pts, K, D, noArray(), K) of OpenCV 2.4.8 on float32 points -> float32 (x, y); every term literally, zero terms included"""
    fx, fy, cx, cy = (np.float64(np.float32(cam[n])) for n in ("fx", "fy", "cx", "cy"))
    k = _k(cam)
    P = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    RR = np.zeros((3, 3), np.float64)                    # cvMatMul(P, I): a double GEMM
    I = np.eye(3)
    for i in range(3):
        for j in range(3):
            s = np.float64(0)
            for m in range(3):
                s = s + P[i, m] * I[m, j]
            RR[i, j] = s
    ifx = np.float64(1.) / fx
    ify = np.float64(1.) / fy
    x = np.asarray(x, np.float32).astype(np.float64)
    y = np.asarray(y, np.float32).astype(np.float64)
    x0 = x = (x - cx) * ifx
    y0 = y = (y - cy) * ify
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
        deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
        x = (x0 - deltaX) * icdist
        y = (y0 - deltaY) * icdist
    xx = RR[0, 0] * x + RR[0, 1] * y + RR[0, 2]
    yy = RR[1, 0] * x + RR[1, 1] * y + RR[1, 2]
    ww = 1. / (RR[2, 0] * x + RR[2, 1] * y + RR[2, 2])
    return (xx * ww).astype(np.float32), (yy * ww).astype(np.float32)


def distort_points(x, y, cam):
    """the forward Brown model (k1, k2, k3 radial, p1, p2 tangential) of undistorted pixels: the inverse undistort_points approximates"""
    fx, fy, cx, cy = (float(np.float32(cam[n])) for n in ("fx", "fy", "cx", "cy"))
    k = _k(cam)
    xn = (np.asarray(x, np.float64) - cx) / fx
    yn = (np.asarray(y, np.float64) - cy) / fy
    r2 = xn * xn + yn * yn
    radial = 1 + k[0] * r2 + k[1] * r2 * r2 + k[4] * r2 * r2 * r2
    xd = xn * radial + 2 * k[2] * xn * yn + k[3] * (r2 + 2 * xn * xn)
    yd = yn * radial + k[2] * (r2 + 2 * yn * yn) + 2 * k[3] * xn * yn
    return xd * fx + cx, yd * fy + cy


def keys_un(keys, cam):
    """Frame::UndistortKeyPoints: mvKeysUn (a copy of mvKeys if k1 == 0)"""
    out = keys.copy()
    if np.float32(cam["k1"]) == 0:
        return out
    out["x"], out["y"] = undistort_points(keys["x"], keys["y"], cam)
    return out


def stereo_from_rgbd(keys, kun, depth, cam):
    """Frame::ComputeStereoFromRGBD: (mvuRight, mvDepth) as float32, -1 where the depth is not > 0"""
    d = depth_at(depth, keys, cam["depth_map_factor"])
    with np.errstate(invalid="ignore"):
        ok = d > 0
    ur = np.full(len(keys), -1, np.float32); dp = np.full(len(keys), -1, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        ur[ok] = kun["x"][ok] - np.float32(cam["bf"]) / d[ok]
    dp[ok] = d[ok]
    return ur, dp


def image_bounds(cam):
    """Frame::ComputeImageBounds: float32 (mnMinX, mnMaxX, mnMinY, mnMaxY)"""
    w, h = cam["width"], cam["height"]
    if np.float32(cam["k1"]) == 0:
        return np.array([0, w, 0, h], np.float32)
    u, v = undistort_points(np.array([0, w, 0, w], np.float32), np.array([0, 0, h, h], np.float32), cam)
    return np.array([min(u[0], u[2]), max(u[1], u[3]), min(v[0], v[1]), max(v[2], v[3])], np.float32)


def frame(ex, colour, depth, cam, rgb=1):
    """the whole restated frame with the oracle's extractor `ex` (pyorc.Extractor): dict(grey, keys, desc, keys_un, u_right, depth)"""
    g = grey(colour, rgb)
    kp, desc = ex.extract(g)
    ku = keys_un(kp, cam)
    if depth is None:
        ur = np.full(len(kp), -1, np.float32); dp = np.full(len(kp), -1, np.float32)
    else:
        ur, dp = stereo_from_rgbd(kp, ku, depth, cam)
    return dict(grey=g, keys=kp, desc=desc, keys_un=ku, u_right=ur, depth=dp)

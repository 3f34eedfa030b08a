"""corb_slam_amd -- the ctypes harness over libcorb_accel.so (the MI355X-native CORB-SLAM hot path).

The product is the C-ABI library (include/*.h) plus the C++ adapter in host/; this package only drives it
from tests/, bench.py and __graft_entry__.py.  It has two layers:
  _abi.py      the mirror of the C ABI, stated once: constants, structures, record dtypes, one prototype
               per exported function, and bind() that puts the prototypes onto an opened library
  _abi_fusion.py  the same for the seventh header, include/corb_map_fusion.h, as a table of its own (bind_fusion())
  _abi_tracklocal.py  the same for the eighth header, include/corb_track_local_map.h (bind_tracklocal())
  _abi_trackframe.py  the same for the ninth header, include/corb_track_frame.h (bind_trackframe())
  _abi_traj.py        the same for the tenth header, include/corb_trajectory.h (bind_traj())
  _abi_loopdetect.py  the same for the eleventh header, include/corb_loop_detect.h (bind_loopdetect())
  __init__.py  (this file) load(), the handle owner, and the classes and functions that marshal numpy
               arrays into the calls -- about 1900 lines, most of them array marshalling
Class / method names mirror the reference (ORBextractor::operator(), ORBmatcher::SearchByBoW /
SearchForTriangulation, Optimizer::GlobalBundleAdjustemnt).  Every C call looks `load` up in this module at
call time (`load().corb_...`) and no object keeps the library, so a test that replaces `load` sees every call.
There is NO fallback: if the HIP library is missing or no gfx950 device is visible, every call raises CorbError.
"""
import ctypes as C
import os
import numpy as np

from ._abi import *         # noqa: F401,F403 -- every name of the mirror, the underscore ones included (_abi.__all__)
from ._abi_fusion import *  # noqa: F401,F403 -- include/corb_map_fusion.h: a table of its own beside the six headers' (see _abi_fusion.py)
from ._abi_tracklocal import *  # noqa: F401,F403 -- include/corb_track_local_map.h: likewise (see _abi_tracklocal.py)
from ._abi_trackframe import *  # noqa: F401,F403 -- include/corb_track_frame.h: likewise (see _abi_trackframe.py)
from ._abi_traj import *  # noqa: F401,F403 -- include/corb_trajectory.h: likewise (see _abi_traj.py)
from ._abi_loopdetect import *  # noqa: F401,F403 -- include/corb_loop_detect.h: likewise (see _abi_loopdetect.py)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcorb_accel.so")

# Optimizer::LocalBundleAdjustment (Optimizer.cc:487-838) and Optimizer::PoseOptimization (272-485) as stage lists
_HM, _HS = float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815)))
# (the final "Check inlier observations" pass of LocalBundleAdjustment tests EVERY edge -- also those set to level 1 after the first round -- with
# its last computed chi2 and a fresh depth: allow_reactivate = 1 on the second stage; Optimizer.cc:763-790)
LOCAL_BA_STAGES = [(5, 1, 5.991, 7.815, 1, 0, 0, 0, 0, _HM, _HS), (10, 0, 5.991, 7.815, 1, 0, 1, 0, 0, _HM, _HS)]
POSE_OPT_STAGES = [(10, 1, 5.991, 7.815, 0, 1, 1, 1, 1, _HM, _HS)] * 3 + [(10, 0, 5.991, 7.815, 0, 1, 1, 1, 1, _HM, _HS)]

_lib = None


def load():
    """dlopen libcorb_accel.so and bind the prototypes (once); raises CorbError if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CorbError("libcorb_accel.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                            "there is no CPU fallback")
        _lib = bind_loopdetect(bind_traj(bind_trackframe(bind_tracklocal(bind_fusion(bind(C.CDLL(LIB_PATH)))))))
    return _lib


class _Handle:
    """The one owner of a library handle: `h` (a c_void_p, null once closed), the name of the function that destroys it, and whether this object owns the
    handle or borrows it from another object (a borrowed handle is never destroyed)."""
    _destroy = None
    h, _owned = None, False         # of an object whose create never ran (immutable: no c_void_p is shared between objects)

    def _create(self, what, *args):
        """call the create function `what`, whose last parameter receives the handle, and own the result"""
        self.h, self._owned = C.c_void_p(), True
        _chk(getattr(load(), what)(*args, C.byref(self.h)), what)

    @classmethod
    def _adopt(cls, handle, owned=True, **attributes):
        """an object of the class around an existing handle (no __init__), with the attributes given"""
        self = cls.__new__(cls)
        self.h, self._owned = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle), owned
        self.__dict__.update(attributes)
        return self

    def close(self):
        h, self.h = self.h, C.c_void_p()
        if h and self._owned:
            getattr(load(), self._destroy)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _chk(rc, what):
    if rc != 0:
        raise CorbError("%s failed (%d): %s" % (what, rc, load().corb_last_error().decode(errors="replace")))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def device_count():
    return load().corb_device_count()


class ORBextractor(_Handle):
    """Mirror of ORB_SLAM2::ORBextractor (corbslam_client/include/ORBextractor.h:45-114).  _handle: the extractor of a front-end, borrowed."""
    _destroy = "corb_orb_destroy"

    def __init__(self, nfeatures=2000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7,
                 width=1241, height=376, max_images=1, device=0, _handle=None):
        self.nlevels, self.width, self.height, self.max_images = nlevels, width, height, max_images
        if _handle is None:
            cfg = OrbConfig(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, max_images, device)
            self._create("corb_orb_create", C.byref(cfg))
        else:
            self.h, self._owned = C.c_void_p(_handle), False
        self.cap = self._out_cap(nfeatures)

    def _out_cap(self, nfeatures):
        return nfeatures + 16 * self.nlevels + 256

    # getters (ORBextractor.h:62-82)
    def tables(self):
        n = self.nlevels
        sc, isc, s2, is2 = (np.zeros(n, np.float32) for _ in range(4))
        quota = np.zeros(n, np.int32); umax = np.zeros(16, np.int32)
        _chk(load().corb_orb_tables(self.h, _p(sc), _p(isc), _p(s2), _p(is2), _p(quota), _p(umax)), "corb_orb_tables")
        return dict(scale=sc, inv_scale=isc, sigma2=s2, inv_sigma2=is2, quota=quota, umax=umax)

    def GetScaleFactors(self):
        return self.tables()["scale"]

    def GetInverseScaleFactors(self):
        return self.tables()["inv_scale"]

    def __call__(self, image):
        """operator()(image, mask, keypoints, descriptors): returns (keypoints[KP_DTYPE], descriptors[n,32])."""
        image = np.ascontiguousarray(image, np.uint8)
        kps = np.zeros(self.cap, KP_DTYPE); desc = np.zeros((self.cap, 32), np.uint8); n = C.c_int()
        if image.size == 0:
            _chk(load().corb_orb_extract(self.h, None, 0, 0, 0, _p(kps), _p(desc), self.cap, C.byref(n)), "corb_orb_extract")
        else:
            h, w = image.shape
            _chk(load().corb_orb_extract(self.h, _p(image), w, h, w, _p(kps), _p(desc), self.cap, C.byref(n)), "corb_orb_extract")
        return kps[: n.value].copy(), desc[: n.value].copy()

    # batched path
    def upload(self, slot, image):
        image = np.ascontiguousarray(image, np.uint8)
        assert image.shape == (self.height, self.width)
        _chk(load().corb_orb_upload(self.h, slot, _p(image), self.width), "corb_orb_upload")
        self._keep = image

    def run(self, n_images):
        _chk(load().corb_orb_run(self.h, n_images), "corb_orb_run")

    def sync(self):
        _chk(load().corb_orb_sync(self.h), "corb_orb_sync")

    def fetch(self, slot):
        kps = np.zeros(self.cap, KP_DTYPE); desc = np.zeros((self.cap, 32), np.uint8); n = C.c_int()
        _chk(load().corb_orb_fetch(self.h, slot, _p(kps), _p(desc), self.cap, C.byref(n)), "corb_orb_fetch")
        return kps[: n.value].copy(), desc[: n.value].copy()

    def pyramid_level(self, slot, level, blurred=False):
        w, h = C.c_int(), C.c_int()
        _chk(load().corb_orb_pyramid_level(self.h, slot, level, bool(blurred), None, 0, C.byref(w), C.byref(h)), "pyramid_level")
        out = np.zeros((h.value, w.value), np.uint8)
        _chk(load().corb_orb_pyramid_level(self.h, slot, level, bool(blurred), _p(out), out.size, C.byref(w), C.byref(h)), "pyramid_level")
        return out

    def candidates(self, slot, level):
        cap = 1 << 20
        out = np.zeros(cap, KP_DTYPE); n = C.c_int()
        _chk(load().corb_orb_fetch_candidates(self.h, slot, level, _p(out), cap, C.byref(n)), "fetch_candidates")
        return out[: n.value].copy()

    def profile(self, enable=True):
        """corb_orb_profile: a mode, not a flag -- 0 off, 1 (True) time the product sequence, 2 time every kernel unsplit on one stream"""
        _chk(load().corb_orb_profile(self.h, int(enable)), "corb_orb_profile")

    def profile_read(self):
        arr = (KernelTime * 64)(); n = C.c_int()
        _chk(load().corb_orb_profile_read(self.h, arr, 64, C.byref(n)), "corb_orb_profile_read")
        return {arr[i].name.decode(): (arr[i].total_ms, arr[i].launches) for i in range(n.value)}


_pinned_keep = []


def warmup(device=0):
    """corb_warmup: create the two workspace lanes (stream, events, pinned block) now instead of inside the first optimisation of the process."""
    _chk(load().corb_warmup(device), "corb_warmup")


def release_scratch(device=0):
    """corb_release_scratch: the workspace arenas and the host-array staging of `device` back to the runtime; returns the bytes freed."""
    n = C.c_uint64(0)
    _chk(load().corb_release_scratch(device, C.byref(n)), "corb_release_scratch")
    return int(n.value)


def scratch_fill(lane, word, min_bytes, device=0):
    """corb_scratch_fill (test aid): the lane's arena as one chunk of at least `min_bytes`, every 32-bit word of it, of the staging and of the pinned block = `word`;
    returns the chunk's capacity."""
    cap = C.c_uint64(0)
    _chk(load().corb_scratch_fill(device, lane, word, min_bytes, C.byref(cap)), "corb_scratch_fill")
    return int(cap.value)


def scratch_report(lane, device=0):
    """corb_scratch_report (test aid): (arena capacity, number of chunks, staging capacity) of the lane"""
    cap = C.c_uint64(0); n = C.c_int(0); st = C.c_uint64(0)
    _chk(load().corb_scratch_report(device, lane, C.byref(cap), C.byref(n), C.byref(st)), "corb_scratch_report")
    return int(cap.value), int(n.value), int(st.value)


def scratch_read(lane, offset, nbytes, device=0):
    """corb_scratch_read (test aid): `nbytes` bytes at `offset` of the lane's single arena chunk as a uint8 array"""
    out = np.empty(int(nbytes), np.uint8)
    _chk(load().corb_scratch_read(device, lane, offset, nbytes, _p(out)), "corb_scratch_read")
    return out


def pinned_empty(shape, dtype):
    """numpy array in page-locked host memory (hipHostMalloc): copies to / from it are DMA transfers and asynchronous on the handle's stream.
    The allocation lives until the process exits."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    ptr = C.c_void_p()                                      # (through the library: the HIP runtime IT is linked with must own the allocation)
    _chk(load().corb_pinned_alloc(max(nbytes, 1), C.byref(ptr)), "corb_pinned_alloc")
    buf = (C.c_uint8 * max(nbytes, 1)).from_address(ptr.value)
    _pinned_keep.append(buf)
    return np.frombuffer(buf, np.uint8, nbytes).view(dtype).reshape(shape)


class StereoFrontend(_Handle):
    """Frame::Frame(stereo) hot path (corbslam_client/src/Frame.cc:61-117): left/right extraction +
    ComputeStereoMatches for a batch of frames."""
    _destroy = "corb_stereo_destroy"

    def __init__(self, nfeatures=2000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7,
                 width=1241, height=376, max_frames=1, fx=718.856, bf=386.1448, device=0):
        cfg = StereoConfig(OrbConfig(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, 0, device),
                           max_frames, fx, bf)
        self._create("corb_stereo_create", C.byref(cfg))
        self.max_frames = max_frames
        self.orb = ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, 2 * max_frames,
                                device, _handle=load().corb_stereo_orb(self.h))
        self._keep = []

    def upload(self, frame, left, right):
        left = np.ascontiguousarray(left, np.uint8); right = np.ascontiguousarray(right, np.uint8)
        _chk(load().corb_stereo_upload(self.h, frame, _p(left), _p(right), left.shape[1]), "corb_stereo_upload")
        self._keep.append((left, right))

    def run(self, n_frames):
        _chk(load().corb_stereo_run(self.h, n_frames), "corb_stereo_run")

    def sync(self):
        _chk(load().corb_stereo_sync(self.h), "corb_stereo_sync")
        self._keep = []

    def upload_batch(self, first, packed):
        """packed: uint8 array [n_frames][2][height][width] (left, right), C-contiguous; pinned memory makes it a DMA."""
        assert packed.flags["C_CONTIGUOUS"] and packed.dtype == np.uint8
        _chk(load().corb_stereo_upload_batch(self.h, first, packed.shape[0], _p(packed)), "corb_stereo_upload_batch")

    def fetch_batch(self, first, n, out=None):
        """All results of frames first .. first+n-1 in one set of copies.  Returns dict of strided arrays:
        kp [2n][cap], desc [2n][cap][32], counts [2n], u_right / depth [n][cap], n_matched [n]  (image 2f = left, 2f+1 = right)."""
        cap = load().corb_orb_capacity(self.orb.h)
        if out is None:
            out = dict(kp=np.zeros((2 * n, cap), KP_DTYPE), desc=np.zeros((2 * n, cap, 32), np.uint8), counts=np.zeros(2 * n, np.int32),
                       u_right=np.zeros((n, cap), np.float32), depth=np.zeros((n, cap), np.float32), n_matched=np.zeros(n, np.int32))
        _chk(load().corb_orb_fetch_batch(self.orb.h, 2 * first, 2 * n, _p(out["kp"]), _p(out["desc"]), _p(out["counts"])), "corb_orb_fetch_batch")
        _chk(load().corb_stereo_fetch_matches_batch(self.h, first, n, _p(out["u_right"]), _p(out["depth"]), _p(out["n_matched"])), "corb_stereo_fetch_matches_batch")
        return out

    def frame_layout(self):
        lay = StereoFrameLayout()
        _chk(load().corb_stereo_frame_layout(self.h, C.byref(lay)), "corb_stereo_frame_layout")
        return lay

    def frames(self, packed, result=None, timing=None):
        """corb_stereo_frames: Frame::Frame(stereo) for the n frames of `packed` ([n][2][height][width] uint8) in ONE call -- one transfer each way, one
        synchronisation.  result: uint8 array of n * frame_layout().frame_bytes bytes (page-locked: pinned_empty); timing: a StereoFrameTiming to fill.
        Returns the result block (parse with unpack_frame)."""
        assert packed.flags["C_CONTIGUOUS"] and packed.dtype == np.uint8
        n = packed.shape[0]
        if result is None:
            result = np.zeros(n * self.frame_layout().frame_bytes, np.uint8)
        _chk(load().corb_stereo_frames(self.h, n, _p(packed), _p(result), C.byref(timing) if timing is not None else None), "corb_stereo_frames")
        return result

    def unpack_frame(self, result, f=0):
        """views into frame f's block of a corb_stereo_frames result"""
        lay = self.frame_layout()
        b = result[f * lay.frame_bytes: (f + 1) * lay.frame_bytes]
        nl, nr, nm, status = (int(x) for x in b[:16].view(np.int32))
        kp = lambda off, n: b[off: off + n * KP_DTYPE.itemsize].view(KP_DTYPE)
        return dict(kl=kp(lay.off_kp_left, nl), kr=kp(lay.off_kp_right, nr), dl=b[lay.off_desc_left: lay.off_desc_left + 32 * nl].reshape(nl, 32),
                    dr=b[lay.off_desc_right: lay.off_desc_right + 32 * nr].reshape(nr, 32), u_right=b[lay.off_u_right: lay.off_u_right + 4 * nl].view(np.float32),
                    depth=b[lay.off_depth: lay.off_depth + 4 * nl].view(np.float32), n_matched=nm, status=status)

    def fetch(self, frame):
        kl, dl = self.orb.fetch(2 * frame)
        kr, dr = self.orb.fetch(2 * frame + 1)
        ur = np.zeros(self.orb.cap, np.float32); dp = np.zeros(self.orb.cap, np.float32)
        n, nm = C.c_int(), C.c_int()
        _chk(load().corb_stereo_fetch_matches(self.h, frame, _p(ur), _p(dp), self.orb.cap, C.byref(n), C.byref(nm)), "fetch_matches")
        return dict(kl=kl, dl=dl, kr=kr, dr=dr, u_right=ur[: n.value].copy(), depth=dp[: n.value].copy(), n_matched=nm.value)


class StereoRectifier(_Handle):
    """What the reference's stereo mains for unrectified cameras do before TrackStereo (Examples/Stereo/stereo_euroc.cc:64-98,136-137): the maps of
    cv::initUndistortRectifyMap from LEFT / RIGHT {K, D, R, P}, and cv::remap(INTER_LINEAR) of every raw pair, on the device in front of a StereoFrontend
    (include/corb_stereo_rectify.h).  left / right: (K, D, R, P) with K, R 3x3, P 3x4 and D of 4, 5 or 8 coefficients.  Close it before its front-end."""

    _destroy = "corb_rect_destroy"

    def __init__(self, stereo_frontend, left, right, raw_width, raw_height):
        self.sf = stereo_frontend
        self.width, self.height, self.raw_width, self.raw_height = stereo_frontend.orb.width, stereo_frontend.orb.height, int(raw_width), int(raw_height)
        cfg = RectifyConfig(); cfg.raw_width = self.raw_width; cfg.raw_height = self.raw_height
        for eye, (K, D, R, P) in ((cfg.left, left), (cfg.right, right)):
            d = np.zeros(8); dd = np.asarray(D, np.float64).reshape(-1); d[: len(dd)] = dd
            for name, v, n in (("K", K, 9), ("D", d, 8), ("R", R, 9), ("P", P, 12)):
                setattr(eye, name, (C.c_double * n)(*np.asarray(v, np.float64).reshape(n)))
        self._create("corb_rect_create", C.byref(cfg), stereo_frontend.h)

    @staticmethod
    def read_settings(path):
        """The `NAME: !!opencv-matrix` blocks (rows, cols, dt, data: [...]) and the plain `NAME: number` entries of an OpenCV FileStorage settings file as a dict
        (its %YAML:1.0 first line and `data:[` are not YAML a library would read, and none is needed)."""
        import re
        txt = open(path).read(); out = {}
        for m in re.finditer(r"^([A-Za-z_][\w.]*):\s*!!opencv-matrix\s*\n\s*rows:\s*(\d+)\s*\n\s*cols:\s*(\d+)\s*\n\s*dt:\s*(\w+)\s*\n\s*data:\s*\[([^\]]*)\]", txt, re.M):
            out[m.group(1)] = np.array([float(v) for v in m.group(5).split(",") if v.strip()], np.float64).reshape(int(m.group(2)), int(m.group(3)))
        for m in re.finditer(r"^([A-Za-z_][\w.]*):\s*([-+0-9.eE]+)\s*$", txt, re.M):
            out[m.group(1)] = float(m.group(2))
        return out

    @classmethod
    def from_settings(cls, stereo_frontend, path):
        """LEFT.* / RIGHT.* of a settings file (stereo_euroc.cc:64-93); the raw size is LEFT.width x LEFT.height"""
        s = cls.read_settings(path)
        need = [e + k for e in ("LEFT.", "RIGHT.") for k in ("K", "D", "R", "P", "width", "height")]
        if any(k not in s for k in need):
            raise CorbError("%s: calibration parameters to rectify stereo are missing (%s)" % (path, ", ".join(k for k in need if k not in s)))
        eye = lambda e: (s[e + ".K"], s[e + ".D"], s[e + ".R"], s[e + ".P"])
        return cls(stereo_frontend, eye("LEFT"), eye("RIGHT"), int(s["LEFT.width"]), int(s["LEFT.height"]))

    def maps(self, eye):
        mx = np.zeros((self.height, self.width), np.float32); my = np.zeros((self.height, self.width), np.float32)
        _chk(load().corb_rect_maps(self.h, eye, _p(mx), _p(my)), "corb_rect_maps")
        return mx, my

    def set_maps(self, eye, map_x, map_y):
        mx = np.ascontiguousarray(map_x, np.float32); my = np.ascontiguousarray(map_y, np.float32)
        assert mx.shape == (self.height, self.width) and my.shape == mx.shape
        _chk(load().corb_rect_set_maps(self.h, eye, _p(mx), _p(my)), "corb_rect_set_maps")

    def _raw(self, packed):
        assert packed.flags["C_CONTIGUOUS"] and packed.dtype == np.uint8 and packed.shape[1:] == (2, self.raw_height, self.raw_width)
        return packed.shape[0]

    def upload_batch(self, first, packed):
        """packed: uint8 [n_frames][2][raw_height][raw_width] (raw left, raw right); afterwards the front-end's run / sync / fetch work unchanged"""
        _chk(load().corb_rect_upload_batch(self.h, first, self._raw(packed), _p(packed)), "corb_rect_upload_batch")

    def frames(self, packed, result=None, timing=None):
        """corb_rect_frames: StereoFrontend.frames for raw input; returns the result block that StereoFrontend.unpack_frame parses"""
        n = self._raw(packed)
        if result is None:
            result = np.zeros(n * self.sf.frame_layout().frame_bytes, np.uint8)
        _chk(load().corb_rect_frames(self.h, n, _p(packed), _p(result), C.byref(timing) if timing is not None else None), "corb_rect_frames")
        return result


class RgbdFrontend(_Handle):
    """Frame::Frame(RGB-D) / Frame::Frame(monocular) hot path (corbslam_client/src/Frame.cc:119-228) with the input conversions of
    Tracking::GrabImageRGBD / GrabImageMonocular (Tracking.cc:206-264): colour -> grey, extraction, UndistortKeyPoints, ComputeStereoFromRGBD.
    Defaults: TUM1's RGB-D settings file.  One frame of input = colour [height][width][channels] (or [height][width] grey) followed by the depth image
    [height][width] (uint16 or float32, RGB-D only); pack_input builds the block."""
    _destroy = "corb_rgbd_destroy"

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7, width=640, height=480, max_frames=1,
                 sensor=SENSOR_RGBD, channels=3, rgb=1, fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989,
                 k1=0.262383, k2=-0.953104, p1=-0.005358, p2=0.002628, k3=1.163314, bf=40.0, depth_map_factor=5000.0, depth_format=DEPTH_U16, device=0):
        cfg = CameraConfig(OrbConfig(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, 0, device), max_frames, sensor, channels, rgb,
                           fx, fy, cx, cy, k1, k2, p1, p2, k3, bf, depth_map_factor, depth_format)
        self._create("corb_rgbd_create", C.byref(cfg))
        self.max_frames, self.width, self.height, self.channels = max_frames, width, height, channels
        self.sensor, self.depth_format = sensor, depth_format
        self.orb = ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, max_frames, device, _handle=load().corb_rgbd_orb(self.h))
        self.layout = self.frame_layout()

    def pack_input(self, frames):
        """frames: list of (colour, depth) pairs (depth None for monocular) -> uint8 [n][input_bytes]"""
        out = np.zeros((len(frames), self.layout.input_bytes), np.uint8)
        for i, (col, dep) in enumerate(frames):
            b = np.ascontiguousarray(col, np.uint8).reshape(-1).view(np.uint8)
            out[i, : b.size] = b
            if self.sensor == SENSOR_RGBD:
                d = np.ascontiguousarray(dep, np.float32 if self.depth_format == DEPTH_F32 else np.uint16).reshape(-1).view(np.uint8)
                out[i, b.size: b.size + d.size] = d
        return out

    def upload_batch(self, first, packed):
        """packed: uint8 [n][input_bytes], C-contiguous (pack_input)"""
        assert packed.flags["C_CONTIGUOUS"] and packed.dtype == np.uint8 and packed.size == packed.shape[0] * self.layout.input_bytes
        _chk(load().corb_rgbd_upload_batch(self.h, first, packed.shape[0], _p(packed)), "corb_rgbd_upload_batch")

    def run(self, n_frames):
        _chk(load().corb_rgbd_run(self.h, n_frames), "corb_rgbd_run")

    def sync(self):
        _chk(load().corb_rgbd_sync(self.h), "corb_rgbd_sync")

    def fetch_batch(self, first, n):
        """strided results of frames first .. first+n-1: keys / keys_un [n][cap], desc [n][cap][32], u_right / depth [n][cap], counts [n]"""
        cap = self.layout.capacity
        out = dict(keys=np.zeros((n, cap), KP_DTYPE), keys_un=np.zeros((n, cap), KP_DTYPE), desc=np.zeros((n, cap, 32), np.uint8),
                   u_right=np.zeros((n, cap), np.float32), depth=np.zeros((n, cap), np.float32), counts=np.zeros(n, np.int32))
        _chk(load().corb_rgbd_fetch_batch(self.h, first, n, _p(out["keys"]), _p(out["keys_un"]), _p(out["desc"]), _p(out["u_right"]), _p(out["depth"]),
                                          _p(out["counts"])), "corb_rgbd_fetch_batch")
        return out

    def fetch(self, frame):
        """frame `frame`'s results after run + sync: dict(keys, keys_un, desc, u_right, depth)"""
        o = self.fetch_batch(frame, 1)
        n = int(o["counts"][0])
        return dict(keys=o["keys"][0, :n].copy(), keys_un=o["keys_un"][0, :n].copy(), desc=o["desc"][0, :n].copy(), u_right=o["u_right"][0, :n].copy(),
                    depth=o["depth"][0, :n].copy())

    def frame_layout(self):
        lay = RgbdFrameLayout()
        _chk(load().corb_rgbd_frame_layout(self.h, C.byref(lay)), "corb_rgbd_frame_layout")
        return lay

    def frames(self, packed, result=None, timing=None):
        """corb_rgbd_frames: the n frames of `packed` (uint8 [n][input_bytes]) in ONE call; result: n * frame_bytes bytes (page-locked: pinned_empty);
        timing: a StereoFrameTiming to fill.  Returns the result block (parse with unpack_frame)."""
        assert packed.flags["C_CONTIGUOUS"] and packed.dtype == np.uint8
        n = packed.shape[0]
        if result is None:
            result = np.zeros(n * self.layout.frame_bytes, np.uint8)
        _chk(load().corb_rgbd_frames(self.h, n, _p(packed), _p(result), C.byref(timing) if timing is not None else None), "corb_rgbd_frames")
        return result

    def unpack_frame(self, result, f=0):
        """views into frame f's block of a corb_rgbd_frames result"""
        lay = self.layout
        b = result[f * lay.frame_bytes: (f + 1) * lay.frame_bytes]
        n, status = (int(x) for x in b[:8].view(np.int32))
        kp = lambda off: b[off: off + n * KP_DTYPE.itemsize].view(KP_DTYPE)
        f32 = lambda off: b[off: off + 4 * n].view(np.float32)
        return dict(keys=kp(lay.off_keys), keys_un=kp(lay.off_keys_un), desc=b[lay.off_desc: lay.off_desc + 32 * n].reshape(n, 32),
                    u_right=f32(lay.off_u_right), depth=f32(lay.off_depth), status=status)

    def bounds(self):
        """Frame::ComputeImageBounds: (mnMinX, mnMaxX, mnMinY, mnMaxY) as float32"""
        out = np.zeros(4, np.float32)
        _chk(load().corb_rgbd_image_bounds(self.h, _p(out)), "corb_rgbd_image_bounds")
        return out


def _fv(node_id, offset, idx, keep):
    node_id = np.ascontiguousarray(node_id, np.uint32); offset = np.ascontiguousarray(offset, np.int32)
    idx = np.ascontiguousarray(idx, np.uint32)
    keep += [node_id, offset, idx]
    return _FeatVec(len(node_id), _p(node_id), _p(offset), _p(idx))


class ORBmatcher:
    """Mirror of ORB_SLAM2::ORBmatcher (corbslam_client/include/ORBmatcher.h:41-107), flat-array form."""
    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

    def __init__(self, nnratio=0.6, checkOri=True, device=0):
        self.nnratio, self.checkOri, self.device = float(nnratio), bool(checkOri), device
        load()                                                  # (a missing library is reported here, not by the first search)

    @staticmethod
    def DescriptorDistance(a, b, device=0):
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32); b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
        out = np.zeros(len(a), np.int32)
        _chk(load().corb_descriptor_distance(_p(a), _p(b), len(a), _p(out), device), "corb_descriptor_distance")
        return out

    def _bow(self, variant, desc1, angle1, valid1, fv1, desc2, angle2, valid2, fv2):
        keep = []
        d1 = np.ascontiguousarray(desc1, np.uint8); d2 = np.ascontiguousarray(desc2, np.uint8)
        a1 = np.ascontiguousarray(angle1, np.float32); a2 = np.ascontiguousarray(angle2, np.float32)
        v1 = np.ascontiguousarray(valid1, np.uint8); v2 = np.ascontiguousarray(valid2, np.uint8)
        A = _BowSide(_p(d1), _p(a1), _p(v1), len(d1), _fv(*fv1, keep))
        B = _BowSide(_p(d2), _p(a2), _p(v2), len(d2), _fv(*fv2, keep))
        nslots = len(d2) if variant == 0 else len(d1)
        match = np.zeros(max(nslots, 1), np.int32); n = C.c_int()
        _chk(load().corb_search_by_bow(variant, C.byref(A), C.byref(B), self.nnratio, self.checkOri, _p(match),
                                       C.byref(n), self.device), "corb_search_by_bow")
        return match[:nslots], n.value

    def SearchByBoW(self, kf, frame):
        """SearchByBoW(KeyFrame*,Frame&) / SearchByBoWInServer: kf, frame = dict(desc, angle, valid, fv)."""
        return self._bow(0, kf["desc"], kf["angle"], kf["valid"], kf["fv"], frame["desc"], frame["angle"],
                         frame.get("valid", np.ones(len(frame["desc"]), np.uint8)), frame["fv"])

    SearchByBoWInServer = SearchByBoW

    def SearchByBoW_KFKF(self, kf1, kf2):
        """SearchByBoW(KeyFrame*,KeyFrame*)"""
        return self._bow(1, kf1["desc"], kf1["angle"], kf1["valid"], kf1["fv"], kf2["desc"], kf2["angle"], kf2["valid"], kf2["fv"])

    @staticmethod
    def _frame_view(fr, keep):
        k = np.ascontiguousarray(fr["keys_un"], KP_DTYPE); ur = np.ascontiguousarray(fr["u_right"], np.float32)
        d = np.ascontiguousarray(fr["desc"], np.uint8); cl = np.ascontiguousarray(fr["claimed"], np.uint8); sc = np.ascontiguousarray(fr["scale"], np.float32)
        keep += [k, ur, d, cl, sc]
        return _FrameView(_p(k), _p(ur), _p(d), len(k), _p(cl), fr["min_x"], fr["min_y"], fr["max_x"], fr["max_y"], _p(sc), len(sc))

    def SearchByProjection(self, frame, mps, mp_desc, th):
        """SearchByProjection(Frame&, const vector<MapPoint*>&, th): mps = TRACKED_DTYPE records (isInFrustum outputs)."""
        keep = []; fv = self._frame_view(frame, keep)
        mps = np.ascontiguousarray(mps, TRACKED_DTYPE); mp_desc = np.ascontiguousarray(mp_desc, np.uint8)
        match = np.zeros(max(len(frame["keys_un"]), 1), np.int32); n = C.c_int()
        _chk(load().corb_search_by_projection_map(C.byref(fv), _p(mps), _p(mp_desc), len(mps), th, self.nnratio, _p(match), C.byref(n), self.device),
             "corb_search_by_projection_map")
        return match[: len(frame["keys_un"])].copy(), n.value

    def SearchByProjection_Frame(self, cur, Tcw, Tlw, fx, fy, cx, cy, bf, mb, last, last_desc, th, bMono):
        """SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono)"""
        keep = []; fv = self._frame_view(cur, keep)
        Tcw = np.ascontiguousarray(Tcw, np.float32).reshape(16); Tlw = np.ascontiguousarray(Tlw, np.float32).reshape(16)
        last = np.ascontiguousarray(last, LAST_DTYPE); last_desc = np.ascontiguousarray(last_desc, np.uint8)
        match = np.zeros(max(len(cur["keys_un"]), 1), np.int32); n = C.c_int()
        _chk(load().corb_search_by_projection_frame(C.byref(fv), _p(Tcw), _p(Tlw), fx, fy, cx, cy, bf, mb, _p(last), _p(last_desc), len(last),
                                                    th, bool(bMono), self.checkOri, _p(match), C.byref(n), self.device),
             "corb_search_by_projection_frame")
        return match[: len(cur["keys_un"])].copy(), n.value

    @staticmethod
    def _kf_view(kf, keep):
        k = np.ascontiguousarray(kf["keys_un"], KP_DTYPE); ur = np.ascontiguousarray(kf["u_right"], np.float32)
        d = np.ascontiguousarray(kf["desc"], np.uint8); sc = np.ascontiguousarray(kf["scale"], np.float32); s2 = np.ascontiguousarray(kf["inv_level_sigma2"], np.float32)
        keep += [k, ur, d, sc, s2]
        return _KeyFrameView(_p(k), _p(ur), _p(d), len(k), kf["min_x"], kf["min_y"], kf["max_x"], kf["max_y"], _p(sc), _p(s2), len(sc),
                             kf["log_scale_factor"], kf["fx"], kf["fy"], kf["cx"], kf["cy"], kf["bf"])

    def SearchByProjection_Reloc(self, cur, claimed, Tcw, pts, desc, th, ORBdist):
        """SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist)"""
        keep = []; kv = self._kf_view(cur, keep)
        claimed = np.ascontiguousarray(claimed, np.uint8); Tcw = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        pts = np.ascontiguousarray(pts, MP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
        match = np.zeros(max(len(cur["keys_un"]), 1), np.int32); n = C.c_int()
        _chk(load().corb_search_by_projection_reloc(C.byref(kv), _p(claimed), _p(Tcw), _p(pts), _p(desc), len(pts), th, ORBdist, self.checkOri,
                                                    _p(match), C.byref(n), self.device), "corb_search_by_projection_reloc")
        return match[: len(cur["keys_un"])].copy(), n.value

    def SearchForInitialization(self, f1, f2, prev_matched, window_size=100):
        """ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORBmatcher.cc:540-655).  Returns (vnMatches12, vbPrevMatched after the call, nmatches)."""
        keep = []
        def fv(fr):
            fr = dict(fr); fr.setdefault("claimed", np.zeros(len(fr["keys_un"]), np.uint8)); fr.setdefault("u_right", -np.ones(len(fr["keys_un"]), np.float32))
            return self._frame_view(fr, keep)
        v1, v2 = fv(f1), fv(f2)
        pm = np.array(prev_matched, np.float32, copy=True).reshape(-1, 2); assert len(pm) == len(f1["keys_un"])
        m = np.zeros(max(len(pm), 1), np.int32); n = C.c_int()
        _chk(load().corb_search_for_initialization(C.byref(v1), C.byref(v2), _p(pm), window_size, self.nnratio, self.checkOri, _p(m), C.byref(n), self.device),
             "corb_search_for_initialization")
        return m[: len(pm)].copy(), pm, n.value

    def SearchByProjection_Scw(self, kf, claimed, Scw, pts, desc, th):
        """SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th) (ORBmatcher.cc:425-538).
        claimed[idx] = vpMatched[idx] is set on entry (None: nothing set).  Returns (match per keyframe feature: point index or -1, nmatches)."""
        keep = []; kv = self._kf_view(kf, keep)
        nk = len(kf["keys_un"])
        claimed = np.zeros(nk, np.uint8) if claimed is None else np.ascontiguousarray(claimed, np.uint8)
        Scw = np.ascontiguousarray(Scw, np.float32).reshape(16)
        pts = np.ascontiguousarray(pts, MP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
        match = np.zeros(max(nk, 1), np.int32); n = C.c_int()
        _chk(load().corb_search_by_projection_scw(C.byref(kv), _p(claimed), _p(Scw), _p(pts), _p(desc), len(pts), th, _p(match), C.byref(n), self.device),
             "corb_search_by_projection_scw")
        return match[:nk].copy(), n.value

    def Fuse(self, kf, T, Ow, pts, desc, th, sim3=False):
        """Fuse(KeyFrame*, vpMapPoints, th) (sim3=False, T = Tcw, Ow = camera centre) / Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint) (sim3=True).
        Returns (best feature per point or -1, best distance, nFused)."""
        keep = []; kv = self._kf_view(kf, keep)
        T = np.ascontiguousarray(T, np.float32).reshape(16); Ow = np.ascontiguousarray(Ow if Ow is not None else np.zeros(3), np.float32)
        pts = np.ascontiguousarray(pts, MP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
        bi = np.zeros(max(len(pts), 1), np.int32); bd = np.zeros(max(len(pts), 1), np.int32); n = C.c_int()
        _chk(load().corb_fuse(C.byref(kv), _p(T), _p(Ow), bool(sim3), _p(pts), _p(desc), len(pts), th, _p(bi), _p(bd), C.byref(n), self.device), "corb_fuse")
        return bi[: len(pts)].copy(), bd[: len(pts)].copy(), n.value

    def SearchBySim3(self, kf1, kf2, T1w, T2w, pts1, desc1, pts2, desc2, s12, R12, t12, th):
        keep = []; k1 = self._kf_view(kf1, keep); k2 = self._kf_view(kf2, keep)
        T1w = np.ascontiguousarray(T1w, np.float32).reshape(16); T2w = np.ascontiguousarray(T2w, np.float32).reshape(16)
        pts1 = np.ascontiguousarray(pts1, MP_DTYPE); pts2 = np.ascontiguousarray(pts2, MP_DTYPE)
        desc1 = np.ascontiguousarray(desc1, np.uint8); desc2 = np.ascontiguousarray(desc2, np.uint8)
        R12 = np.ascontiguousarray(R12, np.float32).reshape(9); t12 = np.ascontiguousarray(t12, np.float32).reshape(3)
        m = np.zeros(max(len(pts1), 1), np.int32); n = C.c_int()
        _chk(load().corb_search_by_sim3(C.byref(k1), C.byref(k2), _p(T1w), _p(T2w), _p(pts1), _p(desc1), _p(pts2), _p(desc2), s12,
                                        _p(R12), _p(t12), th, _p(m), C.byref(n), self.device), "corb_search_by_sim3")
        return m[: len(pts1)].copy(), n.value

    def SearchForTriangulation(self, kf1, kf2, F12, ex, ey, scale2, sigma2_2, bOnlyStereo):
        keep = []
        def side(k):
            d = np.ascontiguousarray(k["desc"], np.uint8); kp = np.ascontiguousarray(k["kp"], KP_DTYPE)
            ur = np.ascontiguousarray(k["u_right"], np.float32); mp = np.ascontiguousarray(k["has_mp"], np.uint8)
            keep.extend([d, kp, ur, mp])
            return _TriSide(_p(d), _p(kp), _p(ur), _p(mp), len(d), _fv(*k["fv"], keep))
        A, B = side(kf1), side(kf2)
        F = np.ascontiguousarray(F12, np.float32).reshape(9)
        sc = np.ascontiguousarray(scale2, np.float32); sg = np.ascontiguousarray(sigma2_2, np.float32)
        pairs = np.zeros((max(len(kf1["desc"]), 1), 2), np.int32); n = C.c_int()
        _chk(load().corb_search_for_triangulation(C.byref(A), C.byref(B), _p(F), ex, ey,
                                                  _p(sc), _p(sg), len(sc), bool(bOnlyStereo), self.checkOri, _p(pairs),
                                                  C.byref(n), self.device), "corb_search_for_triangulation")
        return pairs[: n.value].copy(), n.value


def TriangulatePairs(kf1, kf2, pairs, device=0):
    """The triangulation loop of LocalMapping::CreateNewMapPoints (LocalMapping.cc:268-398) for the pairs of one SearchForTriangulation call (corb_triangulate_pairs).
    kf1 / kf2: dict(kp (mvKeysUn), u_right, depth, Tcw, fx, fy, cx, cy, bf, mb, scale).  Returns (x3D [n, 3], status, source, n_new)."""
    keep = []
    def side(k):
        kp = np.ascontiguousarray(k["kp"], KP_DTYPE); ur = np.ascontiguousarray(k["u_right"], np.float32); dp = np.ascontiguousarray(k["depth"], np.float32)
        sc = np.ascontiguousarray(k["scale"], np.float32); keep.extend([kp, ur, dp, sc])
        s = _NewPointSide(); s.keys_un, s.u_right, s.depth, s.n = _p(kp), _p(ur), _p(dp), len(kp)
        T = np.ascontiguousarray(k["Tcw"], np.float32).reshape(16)
        for i in range(16):
            s.Tcw[i] = float(T[i])
        for f in ("fx", "fy", "cx", "cy", "bf", "mb"):
            setattr(s, f, float(np.float32(k[f])))
        s.scale, s.nlevels = _p(sc), len(sc)
        return s
    A, B = side(kf1), side(kf2)
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2); n = len(pr)
    x3d = np.zeros((max(n, 1), 3), np.float32); st = np.zeros(max(n, 1), np.uint8); src = np.zeros(max(n, 1), np.uint8); nn = C.c_int(0)
    _chk(load().corb_triangulate_pairs(C.byref(A), C.byref(B), _p(pr), n, _p(x3d), _p(st), _p(src), C.byref(nn), device), "corb_triangulate_pairs")
    return x3d[:n], st[:n], src[:n], nn.value


def _sim3_ransac_result(c, n_ev, max_events, cap, events, flags, counts, q):
    k = min(int(n_ev[c]), max_events)
    return dict(ransac_max_its=int(cap[c]), n_events=int(n_ev[c]), events=events[c, :k].copy(), inliers=flags[c, :k].astype(bool),
                counts=counts[c].copy(), q=q[c].copy())


def Sim3Ransac(problems, rand_values, probability=0.99, min_inliers=20, max_iterations=300, fix_scale=False, max_events=None, device=0):
    """Sim3Solver's RANSAC for a list of candidates in one call (corb_sim3_ransac).  problems: dicts(p1c [n, 3], p2c [n, 3], sigma2_1 [n], sigma2_2 [n], K1, K2 =
    (fx, fy, cx, cy)); rand_values [n_problems, max_iterations, 3] results of rand().  Returns per problem dict(ransac_max_its, n_events, events (SIM3_EVENT_DTYPE, the
    first max_events), inliers [events, n] bool, counts [max_iterations], q [max_iterations, 4])."""
    n = len(problems); max_events = max_iterations if max_events is None else int(max_events)
    arr = (_Sim3RansacProblem * max(n, 1))(); keep = []
    for c, q in enumerate(problems):
        a = [np.ascontiguousarray(q[k], np.float32) for k in ("p1c", "p2c", "sigma2_1", "sigma2_2")]
        keep.append(a)
        K = [float(np.float32(v)) for v in tuple(q["K1"]) + tuple(q["K2"])]
        arr[c] = _Sim3RansacProblem(len(a[2]), *[_p(x) for x in a], *K)
    stride = max([len(a[2]) for a in keep] + [1])
    rv = np.ascontiguousarray(rand_values, np.int32).reshape(-1)
    assert len(rv) == n * max_iterations * 3
    cap = np.zeros(max(n, 1), np.int32); n_ev = np.zeros(max(n, 1), np.int32); ev = np.zeros((max(n, 1), max(max_events, 1)), SIM3_EVENT_DTYPE)
    fl = np.zeros((max(n, 1), max(max_events, 1), stride), np.uint8); cnt = np.zeros((max(n, 1), max_iterations), np.int32); qo = np.zeros((max(n, 1), max_iterations, 4), np.float32)
    _chk(load().corb_sim3_ransac(C.cast(arr, C.c_void_p), n, probability, min_inliers, max_iterations, bool(fix_scale), _p(rv), max_events, stride,
                                 _p(cap), _p(n_ev), _p(ev), _p(fl), _p(cnt), _p(qo), device), "corb_sim3_ransac")
    out = [_sim3_ransac_result(c, n_ev, max_events, cap, ev, fl, cnt, qo) for c in range(n)]
    for c, r in enumerate(out):
        r["inliers"] = r["inliers"][:, : len(keep[c][2])]
    return out


class Sim3Solver:
    """Sim3Solver (C/include/Sim3Solver.h) over corb_sim3_ransac: one library call evaluates every hypothesis, then iterate() is replayed from the events.  The
    constructor takes what the reference's leaves (:37-112): mvX3Dc1 / mvX3Dc2, mvLevelSigma2 of the two octaves, both intrinsics (fx, fy, cx, cy); indices1 / n1 =
    mvnIndices1 / mN1 scatter vbInliers as :195-197 do (default: the correspondences themselves).  The draws are an argument: rand_values [maxIterations, 3] results of
    rand() in [0, 2^31), or a seeded numpy.random.RandomState."""

    def __init__(self, p1c, p2c, sigma2_1, sigma2_2, K1, K2, bFixScale=False, indices1=None, n1=None, rand_values=None, seed=0, device=0):
        self.problem = dict(p1c=np.ascontiguousarray(p1c, np.float32).reshape(-1, 3), p2c=np.ascontiguousarray(p2c, np.float32).reshape(-1, 3),
                            sigma2_1=np.ascontiguousarray(sigma2_1, np.float32), sigma2_2=np.ascontiguousarray(sigma2_2, np.float32), K1=tuple(K1), K2=tuple(K2))
        self.N = len(self.problem["sigma2_1"]); self.mbFixScale = bool(bFixScale); self.device = device
        self.mvnIndices1 = np.arange(self.N) if indices1 is None else np.asarray(indices1, np.int64)
        self.mN1 = int(n1) if n1 is not None else (self.N if indices1 is None else int(self.mvnIndices1.max(initial=-1)) + 1)
        self._rand = rand_values; self._seed = seed
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        self.mRansacProb, self.mRansacMinInliers, self._max_its = float(probability), int(minInliers), int(maxIterations)
        self.mnIterations = 0; self._res = None; self._last = None

    def _run(self):
        if self._res is None:
            rv = self._rand if self._rand is not None else np.random.RandomState(self._seed).randint(0, 2 ** 31, (self._max_its, 3))
            rv = np.ascontiguousarray(rv, np.int32).reshape(-1, 3)[: self._max_its]
            self._res = Sim3Ransac([self.problem], rv[None], self.mRansacProb, self.mRansacMinInliers, self._max_its, self.mbFixScale, device=self.device)[0]
            self.mRansacMaxIts = self._res["ransac_max_its"]
        return self._res

    def iterate(self, nIterations):
        """-> (T12 4x4 float32 or None, bNoMore, vbInliers [mN1] bool, nInliers)"""
        vbInliers = np.zeros(self.mN1, bool)
        if self.N < self.mRansacMinInliers:
            return None, True, vbInliers, 0
        r = self._run(); cap = r["ransac_max_its"]
        end = min(self.mnIterations + int(nIterations), cap)
        for k, e in enumerate(r["events"]):
            if self.mnIterations < e["iteration"] <= end:
                self.mnIterations = int(e["iteration"]); self._last = e
                vbInliers[self.mvnIndices1[r["inliers"][k]]] = True
                T = np.eye(4, dtype=np.float32)
                T[:3, :3] = e["s12"] * e["R12"].reshape(3, 3); T[:3, 3] = e["t12"]
                return T, False, vbInliers, int(e["n_inliers"])
        self.mnIterations = end
        return None, self.mnIterations >= cap, vbInliers, 0

    def find(self):
        """-> (T12 or None, vbInliers12, nInliers)"""
        if self.N < self.mRansacMinInliers:
            return None, np.zeros(self.mN1, bool), 0
        T, _, vb, n = self.iterate(self._run()["ransac_max_its"])
        return T, vb, n

    # the best model so far; as every caller reads them after iterate() returned a transformation, they are that return's
    def GetEstimatedRotation(self):
        return None if self._last is None else self._last["R12"].reshape(3, 3).copy()

    def GetEstimatedTranslation(self):
        return None if self._last is None else self._last["t12"].copy()

    def GetEstimatedScale(self):
        return None if self._last is None else float(self._last["s12"])


def PnPRansac(problems, rand_values, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991, tail_iterations=0, max_records=None, device=0):
    """PnPsolver's RANSAC, Refine() included, for a list of candidates in one call (corb_pnp_ransac).  problems: dicts(p3dw [n, 3], p2d [n, 2], sigma2 [n], K = (fx, fy,
    cx, cy)); rand_values [n_problems, max_iterations + tail_iterations, min_set] results of rand().  Returns per problem dict(ransac_max_its, ransac_min_inliers,
    n_records, records (PNP_RECORD_DTYPE, the first max_records), best_inliers / refined_inliers [records, n] bool, counts [max_iterations + tail_iterations], pose
    [.., 16] float64 = R[9], t[3], rep_errors[3], chosen N of every hypothesis, refine_pose [records, 16])."""
    n = len(problems); stride_its = int(max_iterations) + int(tail_iterations)
    max_records = stride_its if max_records is None else int(max_records)
    arr = (_PnPRansacProblem * max(n, 1))(); keep = []
    for c, q in enumerate(problems):
        a = [np.ascontiguousarray(q[k], np.float32) for k in ("p3dw", "p2d", "sigma2")]
        keep.append(a)
        arr[c] = _PnPRansacProblem(len(a[2]), *[_p(x) for x in a], *[float(np.float32(v)) for v in q["K"]])
    stride = max([len(a[2]) for a in keep] + [1])
    rv = np.ascontiguousarray(rand_values, np.int32).reshape(-1)
    assert len(rv) == n * stride_its * min_set
    n1, r1 = max(n, 1), max(max_records, 1)
    cap = np.zeros(n1, np.int32); mi = np.zeros(n1, np.int32); n_rec = np.zeros(n1, np.int32); rec = np.zeros((n1, r1), PNP_RECORD_DTYPE)
    bf = np.zeros((n1, r1, stride), np.uint8); rf = np.zeros((n1, r1, stride), np.uint8); cnt = np.zeros((n1, max(stride_its, 1)), np.int32)
    po = np.zeros((n1, max(stride_its, 1), 16), np.float64); rpo = np.zeros((n1, r1, 16), np.float64)
    _chk(load().corb_pnp_ransac(C.cast(arr, C.c_void_p), n, probability, min_inliers, max_iterations, min_set, epsilon, th2,
                                tail_iterations, _p(rv), max_records, stride, _p(cap), _p(mi), _p(n_rec), _p(rec), _p(bf), _p(rf), _p(cnt), _p(po), _p(rpo), device),
         "corb_pnp_ransac")
    out = []
    for c in range(n):
        k = min(int(n_rec[c]), max_records); nc = len(keep[c][2])
        out.append(_pnp_ransac_result(c, k, nc, cap, mi, n_rec, rec, bf, rf, cnt, po, rpo))
    return out


def _pnp_ransac_result(c, k, nc, cap, mi, n_rec, rec, bf, rf, cnt, po, rpo):
    return dict(ransac_max_its=int(cap[c]), ransac_min_inliers=int(mi[c]), n_records=int(n_rec[c]), records=rec[c, :k].copy(), best_inliers=bf[c, :k, :nc].astype(bool),
                refined_inliers=rf[c, :k, :nc].astype(bool), counts=cnt[c].copy(), pose=po[c].copy(), refine_pose=rpo[c, :k].copy())


def PnPRansacStore(frames, slot, mp_store, cam, matched_ids, rand_values, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991,
                   tail_iterations=0, max_records=None):
    """PnPsolver's constructor, RANSAC and Refine() on records (corb_pnp_ransac_store): the frame = record `slot` of the KeyFrameStore `frames`, matched_ids [n_candidates,
    n(slot)] = one row of vvpMapPointMatches per candidate as MapPoint ids.  Returns per candidate what PnPRansac returns (both inlier sets per feature of the frame =
    vbInliers) plus n_corr and index = mvKeyPointIndices."""
    n1 = load().corb_kf_store_count(frames.h, slot)          # the host-known count: an empty slot (-1) is the library's error to report
    ids = np.ascontiguousarray(matched_ids, np.uint64); ids = ids.reshape(len(ids), -1); n = len(ids)
    assert n == 0 or n1 <= 0 or ids.shape[1] == n1
    stride_its = int(max_iterations) + int(tail_iterations); max_records = stride_its if max_records is None else int(max_records)
    rv = np.ascontiguousarray(rand_values, np.int32).reshape(-1)
    assert len(rv) == n * stride_its * min_set
    nn, r1, s1 = max(n, 1), max(max_records, 1), max(n1, 1)
    cap = np.zeros(nn, np.int32); mi = np.zeros(nn, np.int32); n_rec = np.zeros(nn, np.int32); rec = np.zeros((nn, r1), PNP_RECORD_DTYPE)
    bf = np.zeros((nn, r1, s1), np.uint8); rf = np.zeros((nn, r1, s1), np.uint8); cnt = np.zeros((nn, max(stride_its, 1)), np.int32)
    po = np.zeros((nn, max(stride_its, 1), 16), np.float64); rpo = np.zeros((nn, r1, 16), np.float64); ncorr = np.zeros(nn, np.int32); index = np.full((nn, s1), -1, np.int32)
    _chk(load().corb_pnp_ransac_store(frames.h, slot, mp_store.h, C.byref(cam), _p(ids), n, probability, min_inliers, max_iterations, min_set,
                                      epsilon, th2, tail_iterations, _p(rv), max_records, _p(cap), _p(mi), _p(n_rec), _p(rec), _p(bf), _p(rf), _p(ncorr),
                                      _p(index), _p(cnt), _p(po), _p(rpo)), "corb_pnp_ransac_store")
    out = []
    for c in range(n):
        r = _pnp_ransac_result(c, min(int(n_rec[c]), max_records), n1, cap, mi, n_rec, rec, bf, rf, cnt, po, rpo)
        r["n_corr"] = int(ncorr[c]); r["index"] = index[c, : ncorr[c]].copy()
        out.append(r)
    return out


def pnp_replay(counts, records, m, cap, s, n_iterations):
    """iterate()'s loop (C/src/PnPsolver.cc:227-300) as a function of what corb_pnp_ransac returns: counts = c_i of the evaluated hypotheses, records = the call's records,
    m = ransac_min_inliers, cap = ransac_max_its, s = mnIterations before the call.  Returns (kind, record index or None, mnIterations after): kind 'refined' = the
    refined pose of that record, 'best' = bNoMore with its unrefined pose, None = bNoMore with an empty Mat.  The call returns at the first i >= s with c_i >= m whose
    last record at or before i is ok, else at max(cap, s + n_iterations) -- or where the evaluated hypotheses end."""
    end = min(max(cap, s + int(n_iterations)), len(counts))
    its = [int(r["iteration"]) - 1 for r in records]
    b = -1
    for i in range(end):
        if b + 1 < len(its) and its[b + 1] == i:
            b += 1
        if i >= s and counts[i] >= m and b >= 0 and records[b]["refine_ok"]:
            return "refined", b, i + 1
    return ("best" if b >= 0 else None), (b if b >= 0 else None), max(end, s)


class PnPsolver:
    """PnPsolver (C/include/PnPsolver.h) over corb_pnp_ransac: one library call evaluates every hypothesis and every Refine(), then iterate() is replayed by pnp_replay.  The
    constructor takes what the reference's leaves (:67-110): mvP3Dw, mvP2D, mvSigma2 and (fx, fy, cx, cy); indices / n_matches = mvKeyPointIndices /
    mvpMapPointMatches.size() scatter vbInliers as :274-279 do (default: the correspondences themselves).  The draws are an argument: rand_values [>= maxIterations +
    tail, minSet] results of rand() in [0, 2^31), or a seeded numpy.random.RandomState.  mRansacMaxIts + tail_iterations hypotheses are evaluated: the reference's loop
    runs on behind the cap for as long as it is called (:227), here iterate() reports bNoMore once the evaluated hypotheses run out."""

    def __init__(self, p3dw, p2d, sigma2, K, indices=None, n_matches=None, rand_values=None, seed=0, tail_iterations=0, device=0):
        self.problem = dict(p3dw=np.ascontiguousarray(p3dw, np.float32).reshape(-1, 3), p2d=np.ascontiguousarray(p2d, np.float32).reshape(-1, 2),
                            sigma2=np.ascontiguousarray(sigma2, np.float32).reshape(-1), K=tuple(K))
        self.N = len(self.problem["sigma2"]); self.device = device; self._tail = int(tail_iterations)
        self.mvKeyPointIndices = np.arange(self.N) if indices is None else np.asarray(indices, np.int64)
        self._n_matches = int(n_matches) if n_matches is not None else (self.N if indices is None else int(self.mvKeyPointIndices.max(initial=-1)) + 1)
        self._rand = rand_values; self._seed = seed
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        self._par = (float(probability), int(minInliers), int(maxIterations), int(minSet), float(epsilon), float(th2))
        self.mnIterations = 0; self._res = None

    def _run(self):
        if self._res is None:
            pr, mi, its, ms, eps, th2 = self._par; total = its + self._tail
            rv = self._rand if self._rand is not None else np.random.RandomState(self._seed).randint(0, 2 ** 31, (total, ms))
            rv = np.ascontiguousarray(rv, np.int32).reshape(-1, ms)[:total]
            self._res = PnPRansac([self.problem], rv[None], pr, mi, its, ms, eps, th2, self._tail, device=self.device)[0]
            self.mRansacMaxIts = self._res["ransac_max_its"]; self.mRansacMinInliers = self._res["ransac_min_inliers"]
        return self._res

    def iterate(self, nIterations):
        """-> (Tcw 4x4 float32 or None, bNoMore, vbInliers [mvpMapPointMatches.size()] bool, nInliers)"""
        vbInliers = np.zeros(self._n_matches, bool)
        r = self._run()
        if r["ransac_max_its"] == 0:                                    # N < mRansacMinInliers (:218-222)
            return None, True, vbInliers, 0
        evaluated = r["ransac_max_its"] + self._tail
        kind, b, self.mnIterations = pnp_replay(r["counts"][:evaluated], r["records"], r["ransac_min_inliers"], r["ransac_max_its"], self.mnIterations, nIterations)
        if kind is None:
            return None, True, vbInliers, 0
        e = r["records"][b]; refined = kind == "refined"
        vbInliers[self.mvKeyPointIndices[r["refined_inliers" if refined else "best_inliers"][b]]] = True
        T = np.eye(4, dtype=np.float32); T[:3] = e["Tcw_refined" if refined else "Tcw_best"].reshape(3, 4)
        return T, not refined, vbInliers, int(e["n_refined" if refined else "n_inliers"])

    def find(self):
        """-> (Tcw or None, vbInliers, nInliers)"""
        T, _, vb, n = self.iterate(self._run()["ransac_max_its"])
        return T, vb, n


def _keys(k):
    """keypoints as KP_DTYPE records: a KP_DTYPE array, or [n, 2] coordinates"""
    k = np.asarray(k)
    if k.dtype == KP_DTYPE:
        return np.ascontiguousarray(k)
    out = np.zeros(len(k), KP_DTYPE); xy = np.asarray(k, np.float32).reshape(-1, 2)
    out["x"] = xy[:, 0]; out["y"] = xy[:, 1]
    return out


def MonoInitialize(problems, rand_values, sigma=1.0, max_iterations=200, min_parallax=1.0, min_triangulated=50, p3d_stride=None, flags_stride=None, device=0):
    """Initializer::Initialize for a list of (reference, current) pairs in one call (corb_mono_initialize).  problems: dicts(keys1, keys2 (KP_DTYPE or [n, 2]), matches12
    [n1], K = (fx, fy, cx, cy)); rand_values [n_problems, max_iterations, 8] results of rand().  Returns per problem dict(result (INIT_RESULT_DTYPE record), p3d [n1, 3],
    triangulated [n1] bool, inliers_h / inliers_f [N] bool, scores [max_iterations, 2], raw = the call's rows of p3d_stride / flags_stride entries before that slicing)."""
    n = len(problems); arr = (_InitProblem * max(n, 1))(); keep = []
    for c, q in enumerate(problems):
        a = (_keys(q["keys1"]), _keys(q["keys2"]), np.ascontiguousarray(q["matches12"], np.int32))
        keep.append(a)
        arr[c] = _InitProblem(_p(a[0]), len(a[0]), _p(a[1]), len(a[1]), _p(a[2]), *[float(np.float32(v)) for v in q["K"]])
    Ns = [int((a[2] >= 0).sum()) for a in keep]
    ps = max([len(a[0]) for a in keep] + [1]) if p3d_stride is None else int(p3d_stride)
    fs = max(Ns + [1]) if flags_stride is None else int(flags_stride)
    rv = np.ascontiguousarray(rand_values, np.int32).reshape(-1)
    assert len(rv) == n * int(max_iterations) * 8
    n1 = max(n, 1)
    res = np.zeros(n1, INIT_RESULT_DTYPE); p3d = np.zeros((n1, ps, 3), np.float32); tri = np.zeros((n1, ps), np.uint8)
    ih = np.zeros((n1, fs), np.uint8); i_f = np.zeros((n1, fs), np.uint8); sc = np.zeros((n1, int(max_iterations), 2), np.float32)
    _chk(load().corb_mono_initialize(C.cast(arr, C.c_void_p), n, sigma, max_iterations, min_parallax, min_triangulated, _p(rv), ps, fs, _p(res), _p(p3d),
                                     _p(tri), _p(ih), _p(i_f), _p(sc), device), "corb_mono_initialize")
    return [dict(result=res[c].copy(), p3d=p3d[c, :len(keep[c][0])].copy(), triangulated=tri[c, :len(keep[c][0])].astype(bool), inliers_h=ih[c, :Ns[c]].astype(bool),
                 inliers_f=i_f[c, :Ns[c]].astype(bool), scores=sc[c].copy(), raw=dict(p3d=p3d[c], triangulated=tri[c], inliers_h=ih[c], inliers_f=i_f[c])) for c in range(n)]


class Initializer:
    """Initializer (C/include/Initializer.h) over corb_mono_initialize.  keys1 = ReferenceFrame.mvKeysUn, K = (fx, fy, cx, cy).  The draws are an argument of Initialize:
    rand_values [iterations, 8] results of rand() in [0, 2^31) (the reference's stream is shared with every other RANSAC of the process)."""

    def __init__(self, keys1, K, sigma=1.0, iterations=200, device=0):
        self.mvKeys1 = _keys(keys1); self.mK = tuple(K); self.mSigma = float(sigma); self.mMaxIterations = int(iterations); self.device = device
        self.last = None

    def Initialize(self, keys2, matches12, rand_values):
        """-> (ok, R21 [3, 3], t21 [3], vP3D [n1, 3], vbTriangulated [n1] bool); self.last = everything MonoInitialize returns"""
        r = MonoInitialize([dict(keys1=self.mvKeys1, keys2=keys2, matches12=matches12, K=self.mK)], np.asarray(rand_values)[None], self.mSigma, self.mMaxIterations, 1.0, 50,
                           device=self.device)[0]
        self.last = r; e = r["result"]
        return bool(e["status"] == INIT_OK), e["R21"].reshape(3, 3).copy(), e["t21"].copy(), r["p3d"], r["triangulated"]


def spd_solve(A, b, device=0):
    """corb_spd_solve: x with A x = b for a symmetric positive definite A (hand-written blocked Cholesky, csrc/dense_chol.hip); returns (x, info)"""
    A = np.ascontiguousarray(A, np.float64); b = np.ascontiguousarray(b, np.float64); x = np.zeros(len(b), np.float64); info = C.c_int(0)
    _chk(load().corb_spd_solve(_p(A), len(b), _p(b), _p(x), C.byref(info), device), "corb_spd_solve")
    return x, info.value


def ComputeDistinctiveDescriptors(desc, offset, device=0):
    """MapPoint::ComputeDistinctiveDescriptors for a batch: returns the adopted row (relative) per map point."""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32); offset = np.ascontiguousarray(offset, np.int32)
    best = np.zeros(max(len(offset) - 1, 1), np.int32)
    _chk(load().corb_distinctive_descriptors(_p(desc), _p(offset), len(offset) - 1, _p(best), device), "corb_distinctive_descriptors")
    return best[: len(offset) - 1].copy()


def RebaseMap(To2n, poses, points, device=0):
    """MapFusion::insertServerMapToGlobleMap arithmetic: returns (Tcw * To2n per keyframe, Rwc (p - tcw) per map point)."""
    T = np.ascontiguousarray(To2n, np.float32).reshape(16)
    P = np.array(poses, np.float32).reshape(-1, 16).copy(); X = np.array(points, np.float32).reshape(-1, 3).copy()
    _chk(load().corb_rebase_map(_p(T), _p(P), len(P), _p(X), len(X), device), "corb_rebase_map")
    return P.reshape(-1, 4, 4), X


class Optimizer:
    """Mirror of ORB_SLAM2::Optimizer::GlobalBundleAdjustemnt (sic, corbslam_client/include/Optimizer.h:45)."""

    @staticmethod
    def GlobalBundleAdjustemnt(poses, pose_fixed, points, point_fixed, edges, fx, fy, cx, cy, bf,
                               nIterations=5, bRobust=True, device=0, solver=0, pcg_tol=0.0, pcg_max_iter=0, pc_block=0, intr=None, devflat=False, pc_multilevel=0):
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        pose_fixed = np.ascontiguousarray(pose_fixed, np.uint8); point_fixed = np.ascontiguousarray(point_fixed, np.uint8)
        edges = np.ascontiguousarray(edges, EDGE_DTYPE)
        if intr is not None:
            intr = np.ascontiguousarray(intr, np.float32).reshape(len(poses), 5)   # per-keyframe fx, fy, cx, cy, bf (pKF->fx ... pKF->mbf)
        prob = _BAProblem(len(poses), len(points), len(edges), _p(poses), _p(pose_fixed), _p(points), _p(point_fixed),
                          _p(edges), fx, fy, cx, cy, bf, _p(intr) if intr is not None else None)
        oposes = np.zeros_like(poses); opoints = np.zeros_like(points)
        chi2 = np.zeros(nIterations + 1, np.float64); lam = np.zeros(max(nIterations, 1), np.float64)
        res = _BAResult(_p(oposes), _p(opoints), _p(chi2), _p(lam), 0, 0, 0, 0, 0, 0, 0, 0, 0)
        opt = BAOptions(solver, pcg_tol, pcg_max_iter, pc_block, pc_multilevel)
        if devflat:          # the graph flattening on the device (the path of corb_ba_solve_store)
            _chk(load().corb_ba_solve_devflat(C.byref(prob), nIterations, bool(bRobust), C.byref(res), device, C.byref(opt)), "corb_ba_solve_devflat")
        else:
            _chk(load().corb_ba_solve_ex(C.byref(prob), nIterations, bool(bRobust), None, C.byref(res), device, C.byref(opt)), "corb_ba_solve_ex")
        return dict(poses=oposes.reshape(-1, 4, 4), points=opoints, chi2=chi2[: res.iters_done + 1],
                    lam=lam[: res.iters_done], iters_done=res.iters_done, trials=res.trials_total,
                    solver=res.solver_used, pcg_iterations=res.pcg_iterations, reserved0=res.reserved0,
                    structure=dict(free_poses=res.free_poses, free_points=res.free_points, active_edges=res.active_edges, nnz_blocks=res.nnz_blocks,
                                   schur_pairs=res.schur_pairs, pc_block=res.pc_block, pc_levels=res.pc_levels),
                    certificate=dict(pcg_residual_max=res.pcg_residual_max, pcg_residual_last=res.pcg_residual_last, grad_inf=res.grad_inf, pcg_refined_trials=res.pcg_refined_trials),
                    ms=dict(total=res.ms_total, build=res.ms_build, schur=res.ms_schur, solve=res.ms_solve, update=res.ms_update))


    @staticmethod
    def _staged(stages, poses, pose_fixed, points, point_fixed, edges, fx, fy, cx, cy, bf, device=0, solver=0, intr=None, stop=None):
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        pose_fixed = np.ascontiguousarray(pose_fixed, np.uint8); point_fixed = np.ascontiguousarray(point_fixed, np.uint8)
        edges = np.ascontiguousarray(edges, EDGE_DTYPE)
        if intr is not None:
            intr = np.ascontiguousarray(intr, np.float32).reshape(len(poses), 5)   # per-keyframe fx, fy, cx, cy, bf (pKF->fx ... pKF->mbf)
        prob = _BAProblem(len(poses), len(points), len(edges), _p(poses), _p(pose_fixed), _p(points), _p(point_fixed),
                          _p(edges), fx, fy, cx, cy, bf, _p(intr) if intr is not None else None)
        oposes = np.zeros_like(poses); opoints = np.zeros_like(points)
        res = _BAResult(_p(oposes), _p(opoints), None, None, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        st = (BAStage * len(stages))(*[BAStage(*s) for s in stages])
        outl = np.zeros(max(len(edges), 1), np.uint8)
        opt = BAOptions(solver, 0.0, 0, 0)
        # pbStopFlag (tests): "before" = raised before the call; "after_first_stage" = the flag aliases the result's iteration counter, which turns
        # non-zero exactly when the first optimize() returns (a deterministic stand-in for LocalMapping::InterruptBA during the first round)
        one = C.c_int(1)
        sp = None if stop is None else (C.cast(C.byref(one), C.c_void_p) if stop == "before" else C.cast(C.byref(res, _BAResult.iters_done.offset), C.c_void_p))
        _chk(load().corb_ba_solve_staged(C.byref(prob), st, len(stages), sp, C.byref(res), _p(outl), device, C.byref(opt)), "corb_ba_solve_staged")
        return dict(poses=oposes.reshape(-1, 4, 4), points=opoints, outlier=outl[: len(edges)].copy(), iters_done=res.iters_done,
                    trials=res.trials_total, ms_total=res.ms_total, device_route=bool(res.reserved0), solver=res.solver_used,
                    pcg_iterations=res.pcg_iterations, pcg_refined_trials=res.pcg_refined_trials, reserved0=res.reserved0,
                    structure=dict(free_poses=res.free_poses, free_points=res.free_points, active_edges=res.active_edges, nnz_blocks=res.nnz_blocks,
                                   schur_pairs=res.schur_pairs, pc_block=res.pc_block, pc_levels=res.pc_levels))

    @staticmethod
    def LocalBundleAdjustment(*args, **kw):
        """Optimizer::LocalBundleAdjustment: local keyframes free, fixed keyframes fixed; returns poses, points and the
        observations to erase (outlier[i] = 1 -> pKFi->EraseMapPointMatch / pMP->EraseObservation)."""
        return Optimizer._staged(LOCAL_BA_STAGES, *args, **kw)

    @staticmethod
    def PoseOptimization(Tcw, points, obs, inv_sigma2, fx, fy, cx, cy, bf, device=0, solver=0):
        """Optimizer::PoseOptimization(Frame*): one free pose, fixed map points; obs = (u, v, uRight) per matched point.
        Returns (Tcw, mvbOutlier, nInitialCorrespondences - nBad).  solver 0/3: fused single-workgroup kernel, 1: general path."""
        n = len(points)
        edges = np.zeros(n, EDGE_DTYPE)
        edges["pose"] = 0; edges["point"] = np.arange(n); edges["u"] = obs[:, 0]; edges["v"] = obs[:, 1]; edges["ur"] = obs[:, 2]
        edges["inv_sigma2"] = inv_sigma2
        r = Optimizer._staged(POSE_OPT_STAGES, np.asarray(Tcw, np.float32).reshape(1, 16), np.zeros(1, np.uint8), points, np.ones(n, np.uint8),
                              edges, fx, fy, cx, cy, bf, device=device, solver=solver)
        return r["poses"][0], r["outlier"].astype(bool), int(n - r["outlier"].sum())

    @staticmethod
    def OptimizeEssentialGraph(g, iterations=20, bFixScale=False, device=0):
        """Optimizer::OptimizeEssentialGraph on a flattened graph (dict like synth.essential_graph)."""
        S = np.ascontiguousarray(g["S"], np.float64).copy()
        fixed = np.ascontiguousarray(g["fixed"], np.uint8); vi = np.ascontiguousarray(g["vi"], np.int32); vj = np.ascontiguousarray(g["vj"], np.int32)
        meas = np.ascontiguousarray(g["meas"], np.float64)
        Tiw = np.zeros((len(S), 16), np.float32); pts = np.ascontiguousarray(g["points"], np.float32).copy(); ref = np.ascontiguousarray(g["ref"], np.int32)
        chi2 = np.zeros(iterations + 1, np.float64); it = C.c_int32()
        _chk(load().corb_optimize_essential_graph(len(S), _p(S), _p(fixed), len(vi), _p(vi), _p(vj), _p(meas), iterations, bool(bFixScale), _p(Tiw), len(pts),
                                                  _p(ref), _p(pts), _p(chi2), C.byref(it), device), "corb_optimize_essential_graph")
        return dict(S=S, chi2=chi2[: it.value + 1], iters_done=it.value, Tiw=Tiw.reshape(-1, 4, 4), points=pts)

    @staticmethod
    def OptimizeSim3(problems, th2=10.0, bFixScale=False, device=0):
        """Optimizer::OptimizeSim3 for a list of loop-closure candidates (dicts like synth.sim3_problem).  Returns a list of
        dict(R, t, s, removed, n_in, iters_done)."""
        n = len(problems)
        arr = (_Sim3Problem * n)(); keep = []; rem = []
        R = np.zeros((n, 9), np.float64); t = np.zeros((n, 3), np.float64); s = np.zeros(n, np.float64)
        for f, q in enumerate(problems):
            a = [np.ascontiguousarray(q[k], np.float32) for k in ("p1c", "p2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")]
            keep.append(a); rem.append(np.zeros(max(len(a[0]), 1), np.uint8))
            K = [float(np.float32(q[k])) for k in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2")]
            arr[f] = _Sim3Problem(len(a[0]), *[_p(x) for x in a], *K)
            R[f] = np.asarray(q["R12"], np.float64).reshape(9); t[f] = np.asarray(q["t12"], np.float64).reshape(3); s[f] = q["s12"]
        rptr = (C.c_void_p * n)(*[r.ctypes.data for r in rem])
        nin = np.zeros(n, np.int32); its = np.zeros(n, np.int32)
        _chk(load().corb_optimize_sim3(arr, n, _p(R), _p(t), _p(s), th2, bool(bFixScale), C.cast(rptr, C.c_void_p), _p(nin), _p(its), device), "corb_optimize_sim3")
        return [dict(R=R[f].reshape(3, 3).copy(), t=t[f].copy(), s=float(s[f]), removed=rem[f][: len(keep[f][0])].copy(), n_in=int(nin[f]), iters_done=int(its[f])) for f in range(n)]

    @staticmethod
    def PoseOptimizationBatch(frames, fx, fy, cx, cy, bf, device=0):
        """corb_pose_optimization_batch: frames = list of (Tcw, points, obs, inv_sigma2).  Returns a list of
        (Tcw, mvbOutlier, n_inliers) -- one workgroup per frame, one launch for the whole batch."""
        n = len(frames)
        arr = (_PoseOptFrame * n)()
        keep = []
        outl = []
        for f, (Tcw, points, obs, inv_sigma2) in enumerate(frames):
            T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
            P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
            u = np.ascontiguousarray(obs[:, 0], np.float32); v = np.ascontiguousarray(obs[:, 1], np.float32); ur = np.ascontiguousarray(obs[:, 2], np.float32)
            w = np.ascontiguousarray(inv_sigma2, np.float32)
            o = np.zeros(max(len(P), 1), np.uint8)
            keep.append((T, P, u, v, ur, w)); outl.append(o)
            arr[f] = _PoseOptFrame(_p(T), len(P), _p(P), _p(u), _p(v), _p(ur), _p(w), fx, fy, cx, cy, bf)
        Tout = np.zeros((n, 16), np.float32)
        ninl = np.zeros(n, np.int32)
        optr = (C.c_void_p * n)(*[o.ctypes.data for o in outl])
        _chk(load().corb_pose_optimization_batch(arr, n, _p(Tout), C.cast(optr, C.c_void_p), _p(ninl), device), "corb_pose_optimization_batch")
        return [(Tout[f].reshape(4, 4).copy(), outl[f][: len(keep[f][1])].astype(bool), int(ninl[f])) for f in range(n)]


def bow_profile(enable, device=0):
    _chk(load().corb_bow_profile(bool(enable), device), "corb_bow_profile")


def bow_profile_read():
    """{name: (total_ms, launches)} since the last read (corb_bow_profile_read)"""
    out = (KernelTime * 32)(); n = C.c_int(0)
    _chk(load().corb_bow_profile_read(C.cast(out, C.c_void_p), 32, C.byref(n)), "corb_bow_profile_read")
    return dict((out[i].name.decode(), (out[i].total_ms, out[i].launches)) for i in range(min(n.value, 32)))


class Vocabulary(_Handle):
    """ORBVocabulary (DBoW2::TemplatedVocabulary, L1_NORM / TF_IDF) on the device (corb_voc_*): flat arrays in -- node ids 1 .. n in array order, the root is node 0 -- or
    the text format of loadFromTextFile."""
    _destroy = "corb_voc_destroy"

    def __init__(self, k, L, parent, is_leaf, descriptor, weight, scoring=0, weighting=0, device=0):
        p = np.ascontiguousarray(parent, np.int32); lf = np.ascontiguousarray(is_leaf, np.int32); d = np.ascontiguousarray(descriptor, np.uint8).reshape(-1, 32)
        w = np.ascontiguousarray(weight, np.float64)
        if not (len(p) == len(lf) == len(d) == len(w)):
            raise CorbError("Vocabulary: the node arrays differ in length")
        self.device = device
        c = _VocDesc(int(k), int(L), int(scoring), int(weighting), len(p), _p(p), _p(lf), _p(d), _p(w))
        self._create("corb_voc_create", C.byref(c), device)

    @classmethod
    def from_text(cls, path, device=0):
        h = C.c_void_p()
        _chk(load().corb_voc_load_text(os.fsencode(path), device, C.byref(h)), "corb_voc_load_text")
        return cls._adopt(h, device=device)

    train_stats = None          # of a trained vocabulary: CorbVocTrainStats as a dict

    @classmethod
    def train(cls, sets, k, L, seed, max_iterations=100, device=0):
        """TemplatedVocabulary::create(training_features, k, L) on the device (corb_voc_train): sets = one [n, 32] descriptor array per training image, empty ones allowed"""
        sets = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in sets]
        off = np.zeros(len(sets) + 1, np.int32); off[1:] = np.cumsum([len(d) for d in sets])
        desc = np.ascontiguousarray(np.concatenate(sets)) if sets else np.zeros((0, 32), np.uint8)
        return cls._train_raw(desc, off, k, L, seed, max_iterations, device)

    @classmethod
    def _train_raw(cls, desc, off, k, L, seed, max_iterations, device):
        h = C.c_void_p()
        opt = VocTrainOptions(int(k), int(L), int(max_iterations), 0, int(seed) & (2 ** 64 - 1)); st = VocTrainStats()
        _chk(load().corb_voc_train(_p(desc), _p(np.ascontiguousarray(off, np.int32)), len(off) - 1, C.byref(opt), device, C.byref(h), C.byref(st)), "corb_voc_train")
        return cls._adopt(h, device=device, train_stats=st.as_dict())

    @classmethod
    def train_store(cls, store, slots, k, L, seed, max_iterations=100):
        """corb_voc_train_store: every slot of a KeyFrameStore is one training image; the descriptors stay on the device"""
        h = C.c_void_p(); sl = np.ascontiguousarray(slots, np.int32)
        opt = VocTrainOptions(int(k), int(L), int(max_iterations), 0, int(seed) & (2 ** 64 - 1)); st = VocTrainStats()
        _chk(load().corb_voc_train_store(store.h, _p(sl), len(sl), C.byref(opt), C.byref(h), C.byref(st)), "corb_voc_train_store")
        return cls._adopt(h, device=getattr(store, "device", 0), train_stats=st.as_dict())

    def flat(self, cap_nodes=None):
        """corb_voc_get: the flat arrays of the vocabulary, as dbow_reference.Vocabulary.flat() names them"""
        i = self.info(); n = i["n_nodes"] - 1 if cap_nodes is None else int(cap_nodes)
        p = np.zeros(n, np.int32); lf = np.zeros(n, np.int32); d = np.zeros((n, 32), np.uint8); w = np.zeros(n, np.float64); got = C.c_int(0)
        _chk(load().corb_voc_get(self.h, _p(p), _p(lf), _p(d), _p(w), n, C.byref(got)), "corb_voc_get")
        return dict(k=i["k"], L=i["L"], scoring=0, weighting=0, parent=p, is_leaf=lf, descriptor=d, weight=w)

    def save_text(self, path, digits=0):
        """corb_voc_save_text: the reference's saveToTextFile; digits = 17 reloads bit for bit"""
        _chk(load().corb_voc_save_text(self.h, os.fsencode(path), digits), "corb_voc_save_text")

    def info(self):
        v = [C.c_int32(0) for _ in range(4)]
        _chk(load().corb_voc_info(self.h, *[C.byref(x) for x in v]), "corb_voc_info")
        return dict(k=v[0].value, L=v[1].value, n_nodes=v[2].value, n_words=v[3].value)

    def transform_sets(self, sets, levelsup, per_feature=False):
        """corb_voc_transform: a list of [n, 32] descriptor arrays in one call -> per set (word, value, fv_node, fv_off, fv_idx[, feat_word, feat_node])"""
        sets = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in sets]
        off = np.zeros(len(sets) + 1, np.int32); off[1:] = np.cumsum([len(d) for d in sets])
        t = int(off[-1]); ns = len(sets)
        desc = np.concatenate(sets) if sets else np.zeros((0, 32), np.uint8)
        word = np.zeros(t, np.uint32); val = np.zeros(t, np.float64); bc = np.zeros(ns, np.int32); node = np.zeros(t, np.uint32); fo = np.zeros(t + ns, np.int32)
        idx = np.zeros(t, np.uint32); nn = np.zeros(ns, np.int32); fw = np.zeros(t, np.int32) if per_feature else None; fn = np.zeros(t, np.uint32) if per_feature else None
        _chk(load().corb_voc_transform(self.h, _p(np.ascontiguousarray(desc)), _p(off), ns, levelsup, _p(word), _p(val), _p(bc), _p(node), _p(fo), _p(idx), _p(nn), _p(fw), _p(fn)),
             "corb_voc_transform")
        out = []
        for s in range(ns):
            o = int(off[s]); k = int(nn[s]); o2 = fo[o + s:o + s + k + 1].copy()
            r = (word[o:o + bc[s]].copy(), val[o:o + bc[s]].copy(), node[o:o + k].copy(), o2, idx[o:o + int(o2[k])].copy())
            out.append(r + (fw[o:off[s + 1]].copy(), fn[o:off[s + 1]].copy()) if per_feature else r)
        return out

    def transform(self, desc, levelsup, per_feature=False):
        """TemplatedVocabulary::transform(features, BowVector, FeatureVector, levelsup)"""
        return self.transform_sets([desc], levelsup, per_feature)[0]


class KeyFrameDatabase(_Handle):
    """KeyFrameDatabase (C/src/KeyFrameDatabase.cc) over entries of a device-resident table (corb_kfdb_*).  The detect functions take (query entry, query id); the loop
    variant also the connected keyframes as entries and minScore.  They return the candidates as entries, in the reference's order."""

    _destroy = "corb_kfdb_destroy"

    def __init__(self, voc, capacity, max_words):
        self.voc = voc; self.capacity = capacity; self.max_words = max_words
        self._create("corb_kfdb_create", voc.h, capacity, max_words)

    def set_bow(self, entry, word, value):
        w = np.ascontiguousarray(word, np.uint32); v = np.ascontiguousarray(value, np.float64)
        if len(w) != len(v):
            raise CorbError("KeyFrameDatabase.set_bow: words and values differ in length")
        _chk(load().corb_kfdb_set_bow(self.h, entry, _p(w), _p(v), len(w)), "corb_kfdb_set_bow")

    def get_bow(self, entry):
        w = np.zeros(self.max_words, np.uint32); v = np.zeros(self.max_words, np.float64); n = C.c_int(0)
        _chk(load().corb_kfdb_get_bow(self.h, entry, _p(w), _p(v), self.max_words, C.byref(n)), "corb_kfdb_get_bow")
        return w[:n.value].copy(), v[:n.value].copy()

    def add(self, entry):
        _chk(load().corb_kfdb_add(self.h, entry), "corb_kfdb_add")

    def erase(self, entry):
        _chk(load().corb_kfdb_erase(self.h, entry), "corb_kfdb_erase")

    def clear(self):
        _chk(load().corb_kfdb_clear(self.h), "corb_kfdb_clear")

    def set_neighbours(self, entries, nb):
        e = np.ascontiguousarray(np.atleast_1d(entries), np.int32); b = np.ascontiguousarray(nb, np.int32).reshape(len(e), 10)
        _chk(load().corb_kfdb_set_neighbours(self.h, _p(e), len(e), _p(b)), "corb_kfdb_set_neighbours")

    def state(self, first=0, n=None):
        n = self.capacity - first if n is None else n
        out = np.zeros(n, KFDB_STATE_DTYPE)
        _chk(load().corb_kfdb_get_state(self.h, first, n, _p(out)), "corb_kfdb_get_state")
        return out

    def score(self, entry_a, entries_b):
        b = np.ascontiguousarray(entries_b, np.int32); out = np.zeros(len(b), np.float64)
        _chk(load().corb_kfdb_score(self.h, entry_a, _p(b), len(b), _p(out)), "corb_kfdb_score")
        return out

    def detect(self, kind, query_entry, query_id, connected=(), min_score=0.0, cap=None):
        cap = self.capacity if cap is None else cap
        c = np.ascontiguousarray(list(connected), np.int32); out = np.zeros(max(cap, 1), np.int32); n = C.c_int(0)
        rc = load().corb_kfdb_detect(self.h, kind, query_entry, query_id, _p(c), len(c), min_score, _p(out), cap, C.byref(n))
        self.last_count = n.value
        _chk(rc, "corb_kfdb_detect")
        return out[:n.value].copy()

    def detect_batch(self, kind, entries, ids, cap=None):
        """corb_kfdb_detect_batch: the queries (entries[i], ids[i]) in list order, as `detect` called for one after the other -> (offsets[n + 1], candidates).
        cap=None leaves room for every entry per query.  After a CorbError, last_rc / last_count hold the return code and the room needed."""
        e = np.ascontiguousarray(entries, np.int32).reshape(-1); i = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        if len(e) != len(i):
            raise CorbError("KeyFrameDatabase.detect_batch: entries and ids differ in length")
        cap = len(e) * self.capacity if cap is None else cap
        off = np.zeros(len(e) + 1, np.int32); out = np.zeros(max(cap, 1), np.int32); n = C.c_int(0)
        rc = load().corb_kfdb_detect_batch(self.h, kind, _p(e), _p(i), len(e), _p(off), _p(out), cap, C.byref(n))
        self.last_rc, self.last_count, self.last_offsets = rc, n.value, off
        _chk(rc, "corb_kfdb_detect_batch")
        return off, out[:n.value].copy()

    def DetectLoopCandidates(self, query_entry, query_id, connected, min_score):
        return self.detect(0, query_entry, query_id, connected, min_score)

    def DetectRelocalizationCandidates(self, query_entry, query_id):
        return self.detect(1, query_entry, query_id)

    def DetectMapFusionCandidatesFromDB(self, query_entry, query_id):
        return self.detect(2, query_entry, query_id)


class Covisibility(_Handle):
    """The covisibility graph over a KeyFrameStore and a MapPointStore (corb_covis_*): KeyFrame::UpdateConnections, the covisibility queries, LocalMapping::KeyFrameCulling
    and the window of Optimizer::LocalBundleAdjustment on records.  Keyframes are named by their slots; the queries answer slots."""

    _destroy = "corb_covis_destroy"

    def __init__(self, kf_store, mp_store, max_connections=0):
        self.kf = kf_store; self.mp = mp_store; self.M = max_connections if max_connections > 0 else 512
        self._create("corb_covis_create", kf_store.h, mp_store.h, max_connections)

    def UpdateConnections(self, slots, th=15):
        """corb_covis_update for the slots in list order; returns the front of each keyframe's ordered list (its id, NO_ID if none)"""
        s = np.ascontiguousarray(np.atleast_1d(slots), np.int32); fp = np.full(max(len(s), 1), NO_ID, np.uint64)
        _chk(load().corb_covis_update(self.h, _p(s), len(s), th, _p(fp)), "corb_covis_update")
        return fp[:len(s)].copy()

    def EraseConnections(self, slot):
        _chk(load().corb_covis_erase(self.h, slot), "corb_covis_erase")

    def get(self, slot):
        """the row of a slot: (ids, weights) of the weight map in descending (weight, id), and (ids, weights) of the ordered list"""
        M = self.M; ai = np.zeros(M, np.uint64); aw = np.zeros(M, np.int32); oi = np.zeros(M, np.uint64); ow = np.zeros(M, np.int32); na = C.c_int(0); no = C.c_int(0)
        _chk(load().corb_covis_get(self.h, slot, _p(ai), _p(aw), C.byref(na), _p(oi), _p(ow), C.byref(no), M), "corb_covis_get")
        return (ai[:na.value].copy(), aw[:na.value].copy()), (oi[:no.value].copy(), ow[:no.value].copy())

    def query(self, slot, N=0, min_weight=0, cap=None):
        cap = self.M if cap is None else cap
        out = np.zeros(max(cap, 1), np.int32); w = np.zeros(max(cap, 1), np.int32); n = C.c_int(0)
        _chk(load().corb_covis_query(self.h, slot, N, min_weight, _p(out), _p(w), cap, C.byref(n)), "corb_covis_query")
        return out[:n.value].copy(), w[:n.value].copy()

    def GetVectorCovisibleKeyFrames(self, slot):
        return self.query(slot)[0]

    def GetBestCovisibilityKeyFrames(self, slot, N):
        return self.query(slot, N=N)[0]

    def GetCovisiblesByWeight(self, slot, w):
        return self.query(slot, min_weight=w)[0]

    def GetWeight(self, slot_a, slot_b):
        w = C.c_int(0)
        _chk(load().corb_covis_weight(self.h, slot_a, slot_b, C.byref(w)), "corb_covis_weight")
        return w.value

    def KeyFrameCulling(self, cur_slot, monocular, th_depth, cap=None):
        """per covisible keyframe of cur_slot: (slots, nMPs, nRedundantObservations, cull)"""
        cap = self.M if cap is None else cap; m = max(cap, 1)
        ks = np.zeros(m, np.int32); nm = np.zeros(m, np.int32); nr = np.zeros(m, np.int32); cu = np.zeros(m, np.uint8); n = C.c_int(0)
        _chk(load().corb_covis_keyframe_culling(self.h, cur_slot, bool(monocular), th_depth, _p(ks), _p(nm), _p(nr), _p(cu), cap, C.byref(n)),
             "corb_covis_keyframe_culling")
        k = n.value
        return ks[:k].copy(), nm[:k].copy(), nr[:k].copy(), cu[:k].copy()

    def LocalWindow(self, slot, kf_cap, mp_cap):
        """(kf_slots, n_local, mp_slots): lLocalKeyFrames + lFixedCameras and lLocalMapPoints as corb_local_ba_store takes them"""
        ks = np.zeros(max(kf_cap, 1), np.int32); ms = np.zeros(max(mp_cap, 1), np.int32); nl = C.c_int(0); nk = C.c_int(0); nm = C.c_int(0)
        _chk(load().corb_covis_local_window(self.h, slot, _p(ks), kf_cap, C.byref(nl), C.byref(nk), _p(ms), mp_cap, C.byref(nm)), "corb_covis_local_window")
        return ks[:nk.value].copy(), nl.value, ms[:nm.value].copy()

    # ---- the spanning tree (mpParent, mbFirstConnection, mspChildrens per slot) ----
    def SetTree(self, slot, parent_id=NO_ID, first_connection=True, children=()):
        ch = np.ascontiguousarray(children, np.uint64)
        _chk(load().corb_covis_set_tree(self.h, slot, parent_id, bool(first_connection), _p(ch) if len(ch) else None, len(ch)), "corb_covis_set_tree")

    def GetTree(self, slot):
        """(parent id or NO_ID, mbFirstConnection, children ids ascending)"""
        ch = np.zeros(self.M, np.uint64); p = C.c_uint64(0); f = C.c_int(0); n = C.c_int(0)
        _chk(load().corb_covis_get_tree(self.h, slot, C.byref(p), C.byref(f), _p(ch), self.M, C.byref(n)), "corb_covis_get_tree")
        return int(p.value), bool(f.value), ch[:n.value].copy()

    def AddChild(self, slot, child_slot):
        _chk(load().corb_covis_add_child(self.h, slot, child_slot), "corb_covis_add_child")

    def EraseChild(self, slot, child_slot):
        _chk(load().corb_covis_erase_child(self.h, slot, child_slot), "corb_covis_erase_child")

    def ChangeParent(self, slot, other_slot):
        _chk(load().corb_covis_change_parent(self.h, slot, other_slot), "corb_covis_change_parent")

    def ReparentChildren(self, slot):
        """the tree part of KeyFrame::SetBadFlag, after EraseConnections(slot): (ChangeParent calls, whether the reference sets mbBad)"""
        n = C.c_int(0); b = C.c_int(0)
        _chk(load().corb_covis_reparent_children(self.h, slot, C.byref(n), C.byref(b)), "corb_covis_reparent_children")
        return n.value, bool(b.value)

    # ---- CorrectLoop's propagation on records ----
    def CorrectLoop(self, cur_slot, Scw, scale_factor=0.0, cap=None):
        """corb_loop_correct_store for mpCurrentKF = cur_slot and mg2oScw = Scw (8 doubles: quaternion x y z w, t, s): (kf_slots, CorrectedSim3 [n, 8],
        NonCorrectedSim3 [n, 8], points corrected), the set in ascending keyframe id.  Follow it with UpdateConnections(kf_slots)."""
        cap = self.M + 1 if cap is None else int(cap); m = max(cap, 1)
        S = np.ascontiguousarray(Scw, np.float64).reshape(8)
        ks = np.zeros(m, np.int32); co = np.zeros((m, 8), np.float64); nc = np.zeros((m, 8), np.float64); n = C.c_int(0); npt = C.c_int(0)
        _chk(load().corb_loop_correct_store(self.h, cur_slot, _p(S), scale_factor, _p(ks), _p(co), _p(nc), cap, C.byref(n), C.byref(npt)), "corb_loop_correct_store")
        k = n.value
        return ks[:k].copy(), co[:k].copy(), nc[:k].copy(), npt.value

    # ---- the map update after a global bundle adjustment (RunGlobalBundleAdjustment's spread through the tree) ----
    def PropagateGlobalBA(self, origin_slots, loop_kf, queue_cap=0):
        """corb_gba_propagate_store: TcwGBA / pos_gba become Tcw / world_pos, unmarked keyframes are corrected through the child sets; returns the counts"""
        o = np.ascontiguousarray(np.atleast_1d(origin_slots), np.int32); out = GbaPropagation()
        _chk(load().corb_gba_propagate_store(self.h, _p(o) if len(o) else None, len(o), loop_kf, queue_cap, C.byref(out)), "corb_gba_propagate_store")
        return out

    # ---- the loop edges (mspLoopEdges per slot) and Optimizer::OptimizeEssentialGraph on records (include/corb_essential_graph.h) ----
    MAX_LOOP_EDGES = 32          # CORB_COVIS_MAX_LOOP_EDGES

    def AddLoopEdge(self, slot, other_slot):
        _chk(load().corb_covis_add_loop_edge(self.h, slot, other_slot), "corb_covis_add_loop_edge")

    def GetLoopEdges(self, slot, cap=None):
        """the ids of the set, ascending"""
        cap = self.MAX_LOOP_EDGES if cap is None else int(cap)
        ids = np.zeros(max(cap, 1), np.uint64); n = C.c_int(0)
        _chk(load().corb_covis_get_loop_edges(self.h, slot, _p(ids), cap, C.byref(n)), "corb_covis_get_loop_edges")
        return ids[:n.value].copy()

    def ClearLoopEdges(self, slot):
        _chk(load().corb_covis_clear_loop_edges(self.h, slot), "corb_covis_clear_loop_edges")

    @staticmethod
    def _essential_graph_input(loop_slot, cur_slot, corr_slots, corrected, non_corrected, loop_connections, min_weight):
        """loop_connections: [(key slot, [member slots])] in any order.  Returns the structure and the arrays it points into."""
        cs = np.ascontiguousarray(corr_slots, np.int32).reshape(-1); n = len(cs)
        co = np.ascontiguousarray(corrected, np.float64).reshape(n, 8); nc = np.ascontiguousarray(non_corrected, np.float64).reshape(n, 8)
        lc = list(loop_connections)
        lk = np.array([k for k, _ in lc], np.int32); off = np.concatenate([[0], np.cumsum([len(v) for _, v in lc])]).astype(np.int32)
        ls = np.array([x for _, v in lc for x in v], np.int32)
        keep = (cs, co, nc, lk, off, ls)
        return _EssentialGraphInput(int(loop_slot), int(cur_slot), n, len(lc), cs.ctypes.data or None, co.ctypes.data or None, nc.ctypes.data or None,
                                    lk.ctypes.data or None, off.ctypes.data, ls.ctypes.data or None, int(min_weight), 0), keep

    def EssentialGraphPlan(self, loop_slot, cur_slot, corr_slots, corrected, non_corrected, loop_connections, min_weight=100, v_cap=None, e_cap=None):
        """corb_essential_graph_plan: dict(v_slots, S, fixed, snc, vi, vj, kind, meas, counts).  v_cap / e_cap None: sized by a first call that asks for the counts.
        A cap too small raises CorbError with (-2); the counts of that call are in self.last_plan_counts."""
        inp, keep = self._essential_graph_input(loop_slot, cur_slot, corr_slots, corrected, non_corrected, loop_connections, min_weight)
        cnt = EssentialGraphCounts()
        if v_cap is None or e_cap is None:
            rc = load().corb_essential_graph_plan(self.h, C.byref(inp), 0, 0, *([None] * 8), C.byref(cnt))
            if rc not in (0, ERR_CAPACITY):
                _chk(rc, "corb_essential_graph_plan")
            v_cap = cnt.n_vertices if v_cap is None else v_cap; e_cap = cnt.n_edges if e_cap is None else e_cap
        K = max(v_cap, 1); E = max(e_cap, 1)
        vs = np.zeros(K, np.int32); S = np.zeros((K, 8), np.float64); fx = np.zeros(K, np.uint8); snc = np.zeros((K, 8), np.float64)
        vi = np.zeros(E, np.int32); vj = np.zeros(E, np.int32); kind = np.zeros(E, np.uint8); meas = np.zeros((E, 8), np.float64)
        rc = load().corb_essential_graph_plan(self.h, C.byref(inp), v_cap, e_cap, _p(vs), _p(S), _p(fx), _p(snc), _p(vi), _p(vj), _p(kind), _p(meas), C.byref(cnt))
        self.last_plan_counts = cnt.as_dict()
        _chk(rc, "corb_essential_graph_plan")
        k, e = cnt.n_vertices, cnt.n_edges
        return dict(v_slots=vs[:k].copy(), S=S[:k].copy(), fixed=fx[:k].copy(), snc=snc[:k].copy(), vi=vi[:e].copy(), vj=vj[:e].copy(), kind=kind[:e].copy(),
                    meas=meas[:e].copy(), counts=cnt.as_dict())

    def OptimizeEssentialGraph(self, loop_slot, cur_slot, corr_slots, corrected, non_corrected, loop_connections, bFixScale=False, min_weight=100, iterations=20,
                               scale_factor=0.0, v_cap=None):
        """corb_essential_graph_store: plan, solve, commit poses and points into the records.  Returns dict(result, chi2, S): the result structure, the chi2 history
        and the final estimates in vertex order.  v_cap None: the keyframe store's capacity."""
        inp, keep = self._essential_graph_input(loop_slot, cur_slot, corr_slots, corrected, non_corrected, loop_connections, min_weight)
        v_cap = self.kf.capacity if v_cap is None else int(v_cap)
        chi2 = np.zeros(iterations + 1, np.float64); S = np.zeros((max(v_cap, 1), 8), np.float64); out = EssentialGraphResult()
        rc = load().corb_essential_graph_store(self.h, C.byref(inp), iterations, bool(bFixScale), scale_factor, _p(chi2), _p(S), v_cap, C.byref(out))
        self.last_result = out
        _chk(rc, "corb_essential_graph_store")
        return dict(result=out, chi2=chi2[:out.iters_done + 1].copy(), S=S[:out.graph.n_vertices].copy())

    def SetPoseBeforeGBA(self, slot, T):
        a = np.ascontiguousarray(T, np.float32).reshape(16)
        _chk(load().corb_covis_set_pose_before_gba(self.h, slot, _p(a)), "corb_covis_set_pose_before_gba")

    def GetPoseBeforeGBA(self, slot):
        a = np.zeros(16, np.float32)
        _chk(load().corb_covis_get_pose_before_gba(self.h, slot, _p(a)), "corb_covis_get_pose_before_gba")
        return a.reshape(4, 4)


class Trajectory(_Handle):
    """The camera trajectory on records (corb_traj_*, include/corb_trajectory.h): the per-frame log of Tracking::Track, KeyFrame::mTcp and mTimeStamp per slot of the
    graph's keyframe store, and System::SaveTrajectoryKITTI / SaveTrajectoryTUM / SaveKeyFrameTrajectoryTUM.  sensor: System::eSensor (0 MONOCULAR), for the refusal
    of the two frame dumps (System.cc:256, :352), which the C calls leave to their caller."""

    _destroy = "corb_traj_destroy"

    def __init__(self, covis, capacity_frames, sensor=1):
        self.g = covis; self.capacity = int(capacity_frames); self.n_slots = covis.kf.capacity; self.sensor = sensor
        self._create("corb_traj_create", covis.h, self.capacity)

    def reset(self):
        _chk(load().corb_traj_reset(self.h), "corb_traj_reset")

    def append(self, frames, cur_slot, ref_slot, Tcr=None, timestamp=0.0, lost=False):
        """the end of Tracking::Track: Tcr given (what TrackFrameFinish returned), or None: computed on the device from the two records; cur_slot = -1 repeats the last entry"""
        a = None if Tcr is None else np.ascontiguousarray(Tcr, np.float32).reshape(16)
        _chk(load().corb_traj_append(self.h, frames.h if frames is not None else None, cur_slot, ref_slot, _p(a), float(timestamp), bool(lost)), "corb_traj_append")

    def set_keyframe_time(self, slot, timestamp):
        _chk(load().corb_traj_set_keyframe_time(self.h, slot, float(timestamp)), "corb_traj_set_keyframe_time")

    def get_keyframe_time(self, slot):
        v = C.c_double(0)
        _chk(load().corb_traj_get_keyframe_time(self.h, slot, C.byref(v)), "corb_traj_get_keyframe_time")
        return v.value

    def set_bad_pose(self, slot):
        """KeyFrame.cc:666, before the caller sets CORB_KF_BAD"""
        _chk(load().corb_traj_set_bad_pose(self.h, slot), "corb_traj_set_bad_pose")

    def set_tcp(self, slot, Tcp):
        a = np.ascontiguousarray(Tcp, np.float32).reshape(16)
        _chk(load().corb_traj_set_tcp(self.h, slot, _p(a)), "corb_traj_set_tcp")

    def get_tcp(self, slot):
        a = np.zeros(16, np.float32)
        _chk(load().corb_traj_get_tcp(self.h, slot, _p(a)), "corb_traj_get_tcp")
        return a.reshape(4, 4)

    def get_entries(self):
        e = np.zeros(self.capacity, TRAJ_ENTRY_DTYPE); n = C.c_int(0)
        _chk(load().corb_traj_get_entries(self.h, e.ctypes.data_as(C.POINTER(TrajEntry)), self.capacity, C.byref(n)), "corb_traj_get_entries")
        return e[:n.value].copy()

    def frames(self, origin_slot=-1, format=TRAJ_KITTI, cap=None):
        """(rows [n][12 | 7], times [n], entry_index [n], TrajStats) of corb_traj_frames"""
        cap = self.capacity if cap is None else cap; w = 12 if format == TRAJ_KITTI else 7
        rows = np.zeros((max(cap, 1), w), np.float32); times = np.zeros(max(cap, 1), np.float64); idx = np.zeros(max(cap, 1), np.int32); n = C.c_int(0); st = TrajStats()
        _chk(load().corb_traj_frames(self.h, origin_slot, format, _p(rows), _p(times), _p(idx), cap, C.byref(n), C.byref(st)), "corb_traj_frames")
        return rows[:n.value].copy(), times[:n.value].copy(), idx[:n.value].copy(), st

    def keyframes(self, cap=None):
        """(rows [n][7], times [n], ids [n]) of corb_traj_keyframes"""
        cap = self.n_slots if cap is None else cap
        rows = np.zeros((max(cap, 1), 7), np.float32); times = np.zeros(max(cap, 1), np.float64); ids = np.zeros(max(cap, 1), np.uint64); n = C.c_int(0)
        _chk(load().corb_traj_keyframes(self.h, _p(rows), _p(times), _p(ids), cap, C.byref(n)), "corb_traj_keyframes")
        return rows[:n.value].copy(), times[:n.value].copy(), ids[:n.value].copy()

    def save(self, kind, path, origin_slot=-1):
        _chk(load().corb_traj_save(self.h, origin_slot, kind, os.fsencode(path)), "corb_traj_save")

    def _not_monocular(self, what):
        if self.sensor == 0:
            raise CorbError("ERROR: %s cannot be used for monocular." % what)

    def SaveTrajectoryKITTI(self, path, origin_slot=-1):
        self._not_monocular("SaveTrajectoryKITTI"); self.save(TRAJ_KITTI, path, origin_slot)

    def SaveTrajectoryTUM(self, path, origin_slot=-1):
        self._not_monocular("SaveTrajectoryTUM"); self.save(TRAJ_TUM, path, origin_slot)

    def SaveKeyFrameTrajectoryTUM(self, path):
        self.save(TRAJ_KEYFRAME_TUM, path)


def traj_format_rows(kind, rows, times=None):
    """corb_traj_format_rows: the text of the reference's streams for the rows (bytes); host code, no device"""
    w = 12 if kind == TRAJ_KITTI else 7
    r = np.ascontiguousarray(rows, np.float32).reshape(-1, w); t = None if times is None else np.ascontiguousarray(times, np.float64)
    n = C.c_size_t(0)
    rc = load().corb_traj_format_rows(kind, _p(r), _p(t), len(r), None, 0, C.byref(n))
    if rc != -2:
        _chk(rc, "corb_traj_format_rows")
    buf = C.create_string_buffer(max(n.value, 1))
    if n.value:
        _chk(load().corb_traj_format_rows(kind, _p(r), _p(t), len(r), buf, n.value, C.byref(n)), "corb_traj_format_rows")
    return buf.raw[:n.value]


class LoopDetector(_Handle):
    """LoopClosing::DetectLoop on records (corb_loop_detector_*, corb_loop_detect*, include/corb_loop_detect.h) over a Covisibility graph and a KeyFrameDatabase:
    mLastLoopKFid, mnCovisibilityConsistencyTh and mvConsistentGroups live on the device.  A detect call answers one dict per consumed keyframe:
    outcome (LOOP_*), min_score_bits, cand_entries, cand_slots, enough (positions in the candidate list), n_groups."""

    _destroy = "corb_loop_detector_destroy"

    def __init__(self, covis, db, max_candidates=64, max_groups=128):
        self.g = covis; self.db = db; self.max_candidates = int(max_candidates); self.max_groups = int(max_groups); self.n_slots = covis.kf.capacity
        self._create("corb_loop_detector_create", covis.h, db.h, self.max_candidates, self.max_groups)

    def bind(self, slots, entries):
        s = np.ascontiguousarray(np.atleast_1d(slots), np.int32); e = np.ascontiguousarray(np.atleast_1d(entries), np.int32)
        if len(s) != len(e):
            raise CorbError("LoopDetector.bind: slots and entries differ in length")
        _chk(load().corb_loop_detector_bind(self.h, _p(s), _p(e), len(s)), "corb_loop_detector_bind")

    def set_last_loop(self, kf_id):
        _chk(load().corb_loop_detector_set_last_loop(self.h, int(kf_id)), "corb_loop_detector_set_last_loop")

    def get_last_loop(self):
        v = C.c_uint64(0)
        _chk(load().corb_loop_detector_get_last_loop(self.h, C.byref(v)), "corb_loop_detector_get_last_loop")
        return int(v.value)

    def reset(self):
        _chk(load().corb_loop_detector_reset(self.h), "corb_loop_detector_reset")

    def clear_groups(self):
        _chk(load().corb_loop_detector_clear_groups(self.h), "corb_loop_detector_clear_groups")

    def drop_slot(self, slot):
        _chk(load().corb_loop_detector_drop_slot(self.h, int(slot)), "corb_loop_detector_drop_slot")

    def get_groups(self):
        """mvConsistentGroups in order: [(member slots ascending, counter)]"""
        G = self.max_groups; cnt = np.zeros(G, np.int32); off = np.zeros(G + 1, np.int32); mem = np.zeros(max(G * self.n_slots, 1), np.int32)
        ng = C.c_int(0); nm = C.c_int(0)
        _chk(load().corb_loop_detector_get_groups(self.h, _p(cnt), _p(off), _p(mem), G, G * self.n_slots, C.byref(ng), C.byref(nm)), "corb_loop_detector_get_groups")
        return [(mem[off[g]:off[g + 1]].tolist(), int(cnt[g])) for g in range(ng.value)]

    @staticmethod
    def _answer(r, ce, cs, en):
        nc, ne = int(r["n_candidates"]), int(r["n_enough"])
        return dict(outcome=int(r["outcome"]), min_score_bits=int(r["min_score_bits"]), cand_entries=ce[:nc].tolist(), cand_slots=cs[:nc].tolist(), enough=en[:ne].tolist(),
                    n_groups=int(r["n_groups"]))

    def detect(self, slot):
        """corb_loop_detect for mpCurrentKF = the record in `slot`.  After a CorbError, last_result holds what the call reported (n_candidates on a capacity error)."""
        MC = self.max_candidates
        r = np.zeros(1, LOOP_RESULT_DTYPE); ce = np.zeros(MC, np.int32); cs = np.zeros(MC, np.int32); en = np.zeros(MC, np.int32)
        rc = load().corb_loop_detect(self.h, int(slot), r.ctypes.data_as(C.POINTER(LoopDetectResult)), _p(ce), _p(cs), _p(en))
        self.last_result = r[0].copy()
        _chk(rc, "corb_loop_detect")
        return self._answer(r[0], ce, cs, en)

    def detect_queue(self, slots):
        """corb_loop_detect_queue for mlpLoopKeyFrameQueue = slots: the answers of the consumed keyframes.  A CorbError leaves them in last_answers."""
        s = np.ascontiguousarray(np.atleast_1d(slots), np.int32); n = len(s); MC = self.max_candidates
        r = np.zeros(max(n, 1), LOOP_RESULT_DTYPE); ce = np.zeros((max(n, 1), MC), np.int32); cs = np.zeros_like(ce); en = np.zeros_like(ce); done = C.c_int(0)
        rc = load().corb_loop_detect_queue(self.h, _p(s), n, r.ctypes.data_as(C.POINTER(LoopDetectResult)), _p(ce), _p(cs), _p(en), C.byref(done))
        self.last_answers = [self._answer(r[k], ce[k], cs[k], en[k]) for k in range(done.value)]
        _chk(rc, "corb_loop_detect_queue")
        return self.last_answers

    DetectLoop = detect


class KeyFrameStore(_Handle):
    """Device-resident keyframe store (corb_kf_store_*): one fixed-size SoA record per keyframe in HBM -- what the reference serialises per KeyFrame for
    the client -> server push (corbslam_client/include/KeyFrame.h:59-87).  Slots are filled device-to-device from a StereoFrontend, matched without
    uploads (SearchByBoW / SearchForTriangulation on slots) and pushed to the server rank over RCCL (map_push)."""

    _destroy = "corb_kf_store_destroy"

    def __init__(self, capacity, max_features, device=0):
        self.capacity = capacity; self.F = max_features; self.device = device
        self._create("corb_kf_store_create", device, capacity, max_features)

    def record_bytes(self):
        return load().corb_kf_store_record_bytes(self.h)

    def put_from_stereo(self, slot, sf, frame, keyframe_id=0):
        _chk(load().corb_kf_store_put_from_stereo(self.h, slot, sf.h, frame, keyframe_id), "corb_kf_store_put_from_stereo")

    def put_from_rgbd(self, slot, fe, frame, keyframe_id=0):
        """slot <- mvKeysUn / descriptors / mvuRight / mvDepth of frame `frame` of a RgbdFrontend (device-to-device)"""
        _chk(load().corb_kf_store_put_from_rgbd(self.h, slot, fe.h, frame, keyframe_id), "corb_kf_store_put_from_rgbd")

    def put(self, slot, kp, desc, u_right=None, depth=None, keyframe_id=0):
        kp = np.ascontiguousarray(kp, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
        ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32); dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        _chk(load().corb_kf_store_put_host(self.h, slot, _p(kp), _p(desc), _p(ur), _p(dp), len(kp), keyframe_id), "corb_kf_store_put_host")

    def put_frame(self, slot, kp, desc, u_right, depth, meta):
        """corb_kf_store_put_frame: features and header (KF_META_DTYPE record) in one upload"""
        kp = np.ascontiguousarray(kp, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8); m = np.ascontiguousarray(meta, KF_META_DTYPE)
        ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32); dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        _chk(load().corb_kf_store_put_frame(self.h, slot, _p(kp), _p(desc), _p(ur), _p(dp), len(kp), _p(m)), "corb_kf_store_put_frame")

    def set_bow(self, slot, fv):
        node, off, idx = (np.ascontiguousarray(fv[0], np.uint32), np.ascontiguousarray(fv[1], np.int32), np.ascontiguousarray(fv[2], np.uint32))
        c = _FeatVec(len(node), _p(node), _p(off), _p(idx))
        _chk(load().corb_kf_store_set_bow(self.h, slot, C.byref(c)), "corb_kf_store_set_bow")

    def compute_bow(self, slots, voc, levelsup=4, db=None, entries=None):
        """Frame::ComputeBoW / KeyFrame::ComputeBoW on records (corb_kf_store_compute_bow): the FeatureVector into the slots, the BowVector into `entries` of `db`"""
        sl = np.ascontiguousarray(np.atleast_1d(slots), np.int32); en = None if entries is None else np.ascontiguousarray(np.atleast_1d(entries), np.int32)
        if db is not None and (en is None or len(en) != len(sl)):
            raise CorbError("compute_bow: one database entry per slot")
        _chk(load().corb_kf_store_compute_bow(self.h, _p(sl), len(sl), voc.h, levelsup, db.h if db is not None else None, _p(en)), "corb_kf_store_compute_bow")

    def set_flags(self, slot, flags):
        f = None if flags is None else np.ascontiguousarray(flags, np.uint8)
        _chk(load().corb_kf_store_set_flags(self.h, slot, _p(f)), "corb_kf_store_set_flags")

    def get(self, slot):
        F = self.F
        kp = np.zeros(F, KP_DTYPE); desc = np.zeros((F, 32), np.uint8); ur = np.zeros(F, np.float32); dp = np.zeros(F, np.float32); fl = np.zeros(F, np.uint8)
        node = np.zeros(F, np.uint32); off = np.zeros(F + 1, np.int32); idx = np.zeros(F, np.uint32)
        n = C.c_int(0); kid = C.c_uint64(0); nn = C.c_int32(0)
        _chk(load().corb_kf_store_get(self.h, slot, _p(kp), _p(desc), _p(ur), _p(dp), _p(fl), F, C.byref(n), C.byref(kid), _p(node), _p(off), _p(idx), C.byref(nn)), "corb_kf_store_get")
        m = n.value; k = nn.value
        return dict(kp=kp[:m], desc=desc[:m], u_right=ur[:m], depth=dp[:m], flags=fl[:m], id=kid.value, fv=(node[:k].copy(), off[:k + 1].copy(), idx[:off[k]].copy() if k else idx[:0]))

    def put_batch(self, first, meta, feat_offset, kp, desc=None, u_right=None, depth=None, mp_id=None):
        """corb_kf_store_put_batch: n whole keyframes (meta[n] of KF_META_DTYPE, CSR feature arrays) in one upload and one kernel"""
        m = np.ascontiguousarray(meta, KF_META_DTYPE); off = np.ascontiguousarray(feat_offset, np.int32); k = np.ascontiguousarray(kp, KP_DTYPE)
        d = None if desc is None else np.ascontiguousarray(desc, np.uint8); u = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        dp = None if depth is None else np.ascontiguousarray(depth, np.float32); ids = None if mp_id is None else np.ascontiguousarray(mp_id, np.uint64)
        _chk(load().corb_kf_store_put_batch(self.h, first, len(m), _p(m), _p(off), _p(k), _p(d), _p(u), _p(dp), _p(ids)), "corb_kf_store_put_batch")

    # ---- tracking-thread calls on records (corb_track_*): the current / last Frame are slots of this store, the map is a MapPointStore ----
    def TrackSearchLastFrame(self, cur_slot, last_slot, mp_store, Tcw, Tlw, cam, th, mono=False, nnratio=0.9, check_orientation=True, want_match=True):
        """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1470-1614): writes CurrentFrame.mvpMapPoints into the record"""
        n = self._n_features(cur_slot)
        m = np.full(n, -1, np.int32) if want_match else None; cnt = C.c_int(0)
        a = np.ascontiguousarray(Tcw, np.float32).reshape(16); b = np.ascontiguousarray(Tlw, np.float32).reshape(16)
        _chk(load().corb_track_search_last_frame(self.h, cur_slot, last_slot, mp_store.h, _p(a), _p(b), C.byref(cam), th, bool(mono),
                                                 nnratio, bool(check_orientation), _p(m), C.byref(cnt)), "corb_track_search_last_frame")
        return m, cnt.value

    def TrackPoseOptimization(self, slot, mp_store, cam, Tcw, discard_outliers=False, want_outliers=True):
        """Optimizer::PoseOptimization(Frame*) (Optimizer.cc:272-485) on the record: returns (Tcw, mvbOutlier, inliers); pose and outlier flags stay in the record"""
        n = self._n_features(slot)
        a = np.ascontiguousarray(Tcw, np.float32).reshape(16); out = np.zeros(16, np.float32); fl = np.zeros(n, np.uint8) if want_outliers else None; inl = C.c_int32(0)
        _chk(load().corb_track_pose_optimization(self.h, slot, mp_store.h, C.byref(cam), _p(a), _p(out), bool(discard_outliers), _p(fl), C.byref(inl)), "corb_track_pose_optimization")
        return out.reshape(4, 4), (fl.astype(bool) if want_outliers else None), inl.value

    def TrackSearchLocalPoints(self, slot, mp_store, local_ids, cam, Tcw, log_scale_factor, th=1.0, nnratio=0.8, want_match=True, want_tracked=False):
        """Tracking::SearchLocalPoints (Tracking.cc:1168-1216) on the record: isInFrustum on the device, SearchByProjection(Frame&, vpMapPoints, th); returns
        (match into local_ids per feature, matches, points in view[, TRACKED array])"""
        n = self._n_features(slot)
        ids = np.ascontiguousarray(local_ids, np.uint64)
        m = np.full(n, -1, np.int32) if want_match else None; tr = np.zeros(len(ids), TRACKED_DTYPE) if want_tracked else None
        cnt = C.c_int(0); inv = C.c_int(0)
        a = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        _chk(load().corb_track_search_local_points(self.h, slot, mp_store.h, _p(ids), len(ids), C.byref(cam), _p(a), log_scale_factor, th,
                                                   nnratio, _p(m), _p(tr), C.byref(cnt), C.byref(inv)), "corb_track_search_local_points")
        return (m, cnt.value, inv.value, tr) if want_tracked else (m, cnt.value, inv.value)

    def TrackUpdateLocalMap(self, slot, covis, prev_kf_slots=(), kf_cap=None, mp_cap=None):
        """Tracking::UpdateLocalMap (Tracking.cc:1218-1366) for the frame in `slot` of this store against the graph `covis` (corb_track_update_local_map): returns
        (kf_slots, mp_slots, mp_ids, info) -- mvpLocalKeyFrames and mvpLocalMapPoints as slots of the graph's stores, the points' ids as TrackSearchLocalPoints takes
        them, and the LocalMap record (n_kf, n_voted, n_mp, ref_slot, ref_id, counter_empty, n_cleared).  kf_cap / mp_cap default to 128 keyframes and 16384 points;
        a longer list answers CORB_ERR_CAPACITY with nothing written."""
        prev = np.ascontiguousarray(prev_kf_slots, np.int32)
        # the caps size the points pass's launch and the read-back (4 bytes per keyframe, 12 per point of the caps), so the defaults fit a local map, not the store:
        # 128 keyframes (the walk stops beyond 80; only more voters than that give more) and 16384 points.  Larger maps: pass the caps.
        kf_cap = max(min(covis.M, 128), 83, len(prev)) if kf_cap is None else int(kf_cap)
        mp_cap = min(covis.mp.capacity, kf_cap * covis.kf.F, 16384) if mp_cap is None else int(mp_cap)
        ks = np.zeros(max(kf_cap, 1), np.int32); ms = np.zeros(max(mp_cap, 1), np.int32); ids = np.zeros(max(mp_cap, 1), np.uint64); info = LocalMap()
        _chk(load().corb_track_update_local_map(covis.h, self.h, slot, _p(prev) if len(prev) else None, len(prev), _p(ks), kf_cap, _p(ms), _p(ids), mp_cap, C.byref(info)),
             "corb_track_update_local_map")
        return ks[:info.n_kf].copy(), ms[:info.n_mp].copy(), ids[:info.n_mp].copy(), info

    def TrackLocalMap(self, slot, covis, cam, Tcw, frame_id, log_scale_factor, prev_kf_slots=(), last_reloc_frame_id=0, max_frames=30, sensor=1, only_tracking=False,
                      nnratio=0.8, th=0.0, kf_cap=None, mp_cap=None, want_match=True, want_outliers=True):
        """bool Tracking::TrackLocalMap() (Tracking.cc:951-992) for the frame in `slot` of this store against the graph `covis` in one call (corb_track_local_map):
        UpdateLocalMap, SearchLocalPoints, PoseOptimization and the tail, with mnVisible / mnFound and the tracking scratch written into the map-point records.
        Returns a dict: ok (the reference's bool), kf_slots / mp_slots / mp_ids / local as TrackUpdateLocalMap, match (index into the local list per feature or -1),
        outlier (mvbOutlier), n_in_view, n_matches, n_pose_inliers, n_matches_inliers, th_used, Tcw.  The caps default as TrackUpdateLocalMap's."""
        n = max(load().corb_kf_store_count(self.h, slot), 0)          # (an empty slot is the call's to report)
        prev = np.ascontiguousarray(prev_kf_slots, np.int32)
        kf_cap = max(min(covis.M, 128), 83, len(prev)) if kf_cap is None else int(kf_cap)
        mp_cap = min(covis.mp.capacity, kf_cap * covis.kf.F, 16384) if mp_cap is None else int(mp_cap)
        ks = np.zeros(max(kf_cap, 1), np.int32); ms = np.zeros(max(mp_cap, 1), np.int32); ids = np.zeros(max(mp_cap, 1), np.uint64)
        m = np.full(max(n, 1), -1, np.int32) if want_match else None; fl = np.zeros(max(n, 1), np.uint8) if want_outliers else None
        a = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        par = TrackLocalMapParams(frame_id, last_reloc_frame_id, max_frames, sensor, int(bool(only_tracking)), log_scale_factor, nnratio, th); out = TrackLocalMapResult()
        _chk(load().corb_track_local_map(covis.h, self.h, slot, C.byref(cam), _p(a), _p(prev) if len(prev) else None, len(prev), C.byref(par), _p(ks), kf_cap, _p(ms), _p(ids), mp_cap,
                                         _p(m), _p(fl), C.byref(out)), "corb_track_local_map")
        L = out.local
        return dict(ok=bool(out.ok), kf_slots=ks[:L.n_kf].copy(), mp_slots=ms[:L.n_mp].copy(), mp_ids=ids[:L.n_mp].copy(), local=L, match=m[:n] if want_match else None,
                    outlier=fl[:n].astype(bool) if want_outliers else None, n_in_view=out.n_in_view, n_matches=out.n_matches, n_pose_inliers=out.n_pose_inliers,
                    n_matches_inliers=out.n_matches_inliers, th_used=out.th_used, Tcw=np.array(out.Tcw, np.float32).reshape(4, 4))

    def TrackLocalMapStats(self, slot, mp_store, frame_id, last_reloc_frame_id=0, max_frames=30, sensor=1, only_tracking=False):
        """The tail of TrackLocalMap (Tracking.cc:960-991) on a record TrackPoseOptimization(discard_outliers=False) has left (corb_track_local_map_stats): mnFound of
        the inliers' points, the stereo outliers' points leave the frame; returns (mnMatchesInliers, the reference's bool)"""
        cnt = C.c_int32(0); ok = C.c_int(0)
        _chk(load().corb_track_local_map_stats(self.h, slot, mp_store.h, sensor, bool(only_tracking), frame_id, last_reloc_frame_id, max_frames, C.byref(cnt), C.byref(ok)),
             "corb_track_local_map_stats")
        return cnt.value, bool(ok.value)

    def _track_frame_result(self, out, n, m, fl):
        T = lambda a: np.array(a, np.float32).reshape(4, 4)
        return dict(ok=bool(out.ok), vo=bool(out.vo), n_matches_first=out.n_matches_first, searched_wide=bool(out.searched_wide), n_matches=out.n_matches, th_used=out.th_used,
                    n_pose_inliers=out.n_pose_inliers, n_matches_kept=out.n_matches_kept, n_matches_map=out.n_matches_map, Tlw=T(out.Tlw), Tcw_pred=T(out.Tcw_pred), Tcw=T(out.Tcw),
                    match=None if m is None else m[:n], outlier=None if fl is None else fl[:n].astype(bool))

    def TrackWithMotionModel(self, cur_slot, last_slot, kf_store, ref_slot, mp_store, cam, velocity, frame_id, Tlr=None, sensor=1, only_tracking=False, check_replaced=False,
                             nnratio=0.9, check_orientation=True, th=0.0, want_match=True, want_outliers=True):
        """bool Tracking::TrackWithMotionModel() (Tracking.cc:886-949) in one call (corb_track_with_motion_model): CheckReplacedInLastFrame when asked, UpdateLastFrame's
        pose from Tlr and the reference keyframe's record (ref_slot of kf_store) when Tlr is given, SetPose(velocity * Tlw), the fill, SearchByProjection at th and --
        decided on the device -- at 2 th, PoseOptimization, the "Discard outliers" loop with its writes into the map points.  Returns a dict: ok (the reference's bool),
        vo (mbVO), n_matches_first, searched_wide, n_matches, th_used, n_pose_inliers, n_matches_kept, n_matches_map, Tlw, Tcw_pred, Tcw, match (the last frame's
        feature per feature, or -1), outlier (the features the optimisation rejected)."""
        n = max(load().corb_kf_store_count(self.h, cur_slot), 0)          # (an empty slot is the call's to report)
        m = np.full(max(n, 1), -1, np.int32) if want_match else None; fl = np.zeros(max(n, 1), np.uint8) if want_outliers else None
        v = np.ascontiguousarray(velocity, np.float32).reshape(16); r = None if Tlr is None else np.ascontiguousarray(Tlr, np.float32).reshape(16)
        par = TrackFrameParams(frame_id, sensor, int(bool(only_tracking)), int(bool(check_replaced)), int(bool(check_orientation)), nnratio, th); out = TrackFrameResult()
        _chk(load().corb_track_with_motion_model(self.h, cur_slot, last_slot, kf_store.h, ref_slot, mp_store.h, C.byref(cam), _p(v), _p(r), C.byref(par), _p(m), _p(fl), C.byref(out)),
             "corb_track_with_motion_model")
        return self._track_frame_result(out, n, m, fl)

    def TrackReferenceKeyFrame(self, cur_slot, last_slot, kf_store, ref_slot, mp_store, cam, frame_id, voc=None, sensor=1, check_replaced=False, nnratio=0.7,
                               check_orientation=True, want_match=True, want_outliers=True):
        """bool Tracking::TrackReferenceKeyFrame() (Tracking.cc:775-817) in one call (corb_track_reference_keyframe): ComputeBoW when `voc` is given and the record has no
        FeatureVector, SearchByBoW against the reference keyframe (ref_slot of kf_store) with the validity of its features taken from the map, and from 15 matches on
        setMapPointMatches, SetPose(the last record's pose), PoseOptimization and the "Discard outliers" loop.  The dict of TrackWithMotionModel; match = the keyframe's
        feature per feature, or -1."""
        n = max(load().corb_kf_store_count(self.h, cur_slot), 0)
        m = np.full(max(n, 1), -1, np.int32) if want_match else None; fl = np.zeros(max(n, 1), np.uint8) if want_outliers else None
        par = TrackFrameParams(frame_id, sensor, 0, int(bool(check_replaced)), int(bool(check_orientation)), nnratio, 0.0); out = TrackFrameResult()
        _chk(load().corb_track_reference_keyframe(self.h, cur_slot, last_slot, kf_store.h, ref_slot, mp_store.h, C.byref(cam), voc.h if voc is not None else None, C.byref(par),
                                                  _p(m), _p(fl), C.byref(out)), "corb_track_reference_keyframe")
        return self._track_frame_result(out, n, m, fl)

    def TrackFrameFinish(self, cur_slot, kf_store, ref_slot, mp_store, stage):
        """The per-feature loops at the end of Tracking::Track (corb_track_frame_finish).  stage 0: "Clean VO matches" (Tracking.cc:438-447), asynchronous, returns None.
        stage 1: the outliers' points leave the frame (:463-467); returns Tcr = Tcw * GetPoseInverse(reference keyframe) (:491), what the next frame passes as Tlr."""
        Tcr = np.zeros(16, np.float32) if stage else None
        _chk(load().corb_track_frame_finish(self.h, cur_slot, kf_store.h, ref_slot, mp_store.h, stage, _p(Tcr)), "corb_track_frame_finish")
        return Tcr.reshape(4, 4) if stage else None

    def SearchByProjectionScw(self, slot, mp_store, mp_slots, cam, Scw, log_scale_factor, matched_ids, th=10):
        """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cc:425-538) on records (corb_search_by_projection_scw_store): pKF = this store's `slot`,
        vpPoints = mp_slots of mp_store, vpMatched = matched_ids (uint64 per feature, NO_MAP_POINT = NULL).  Returns (vpMatched after the call as ids, match into mp_slots or -1, nmatches)."""
        n = self._n_features(slot)
        ms = np.ascontiguousarray(mp_slots, np.int32); S = np.ascontiguousarray(Scw, np.float32).reshape(16)
        ids = np.array(matched_ids, np.uint64, copy=True); assert len(ids) == n
        m = np.full(max(n, 1), -1, np.int32); cnt = C.c_int(0)
        _chk(load().corb_search_by_projection_scw_store(self.h, slot, mp_store.h, _p(ms), len(ms), C.byref(cam), _p(S), log_scale_factor, th,
                                                        _p(ids), _p(m), C.byref(cnt)), "corb_search_by_projection_scw_store")
        return ids, m[:n], cnt.value

    def Fuse(self, slot, mp_store, mp_slots, cam, Tcw, log_scale_factor, th=3.0, apply=False):
        """ORBmatcher::Fuse(pKF, vpMapPoints, th) on records (corb_fuse_store): pKF = this store's `slot`, vpMapPoints = mp_slots of mp_store.
        Returns (best_idx, best_dist, n_fused, action): action 1 = entered a feature without MapPoint (apply: records updated), 2 = Replace pending."""
        ms = np.ascontiguousarray(mp_slots, np.int32); T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        bi = np.full(max(len(ms), 1), -1, np.int32); bd = np.full(max(len(ms), 1), 256, np.int32); act = np.zeros(max(len(ms), 1), np.uint8); n = C.c_int(0)
        _chk(load().corb_fuse_store(self.h, slot, mp_store.h, _p(ms), len(ms), C.byref(cam), _p(T), log_scale_factor, th, bool(apply),
                                    _p(bi), _p(bd), _p(act), C.byref(n)), "corb_fuse_store")
        return bi[: len(ms)], bd[: len(ms)], n.value, act[: len(ms)]

    def FuseSim3(self, slot, mp_store, mp_slots, cam, Scw, log_scale_factor, th=4.0, apply=False):
        """ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) on records (corb_fuse_sim3_store): Scw = 16 floats.  Returns (best_idx, best_dist, n_fused, action,
        replace_slot): action 1 = entered an empty feature, 2 = replace_slot holds vpReplacePoint (Replace pending, -1: the id has no record), 4 = the feature's point is bad."""
        ms = np.ascontiguousarray(mp_slots, np.int32); T = np.ascontiguousarray(Scw, np.float32).reshape(16); k = max(len(ms), 1)
        bi = np.full(k, -1, np.int32); bd = np.full(k, 256, np.int32); act = np.zeros(k, np.uint8); rs = np.full(k, -1, np.int32); n = C.c_int(0)
        _chk(load().corb_fuse_sim3_store(self.h, slot, mp_store.h, _p(ms), len(ms), C.byref(cam), _p(T), log_scale_factor, th, bool(apply),
                                         _p(bi), _p(bd), _p(rs), _p(act), C.byref(n)), "corb_fuse_sim3_store")
        return bi[: len(ms)], bd[: len(ms)], n.value, act[: len(ms)], rs[: len(ms)]

    def CreateNewMapPoints(self, cur_slot, nb_slots, F12, epipoles, cam, mp_store=None, first_mp_slot=0, first_mp_id=0, client_id=0, only_stereo=False, apply=False):
        """The neighbour loop of LocalMapping::CreateNewMapPoints on records (corb_create_new_map_points_store): matching per neighbour against the evolving flags of
        cur_slot, triangulation, and (apply) the new MapPoint records of mp_store from first_mp_slot on.  F12 [n_nb, 3, 3], epipoles [n_nb, 2].
        Returns dict(pair_offset, pairs, x3d, status, source, n_new)."""
        nb = np.ascontiguousarray(nb_slots, np.int32).reshape(-1); n_nb = len(nb); n1 = self._n_features(cur_slot)
        F = np.ascontiguousarray(F12, np.float32).reshape(-1); ep = np.ascontiguousarray(epipoles, np.float32).reshape(-1)
        assert len(F) == 9 * n_nb and len(ep) == 2 * n_nb
        cap = max(n_nb * n1, 1)
        off = np.zeros(n_nb + 1, np.int32); pr = np.zeros((cap, 2), np.int32); x3d = np.zeros((cap, 3), np.float32); st = np.zeros(cap, np.uint8); src = np.zeros(cap, np.uint8)
        nn = C.c_int(0)
        _chk(load().corb_create_new_map_points_store(self.h, cur_slot, _p(nb), n_nb, _p(F), _p(ep), C.byref(cam), bool(only_stereo), bool(apply),
                                                     mp_store.h if mp_store is not None else None, first_mp_slot, first_mp_id, client_id,
                                                     _p(off), _p(pr), _p(x3d), _p(st), _p(src), C.byref(nn)), "corb_create_new_map_points_store")
        m = int(off[n_nb])
        return dict(pair_offset=off, pairs=pr[:m].copy(), x3d=x3d[:m].copy(), status=st[:m].copy(), source=src[:m].copy(), n_new=nn.value)

    def TrackSearchReloc(self, cur_slot, kf_store, kf_slot, mp_store, cam, Tcw, log_scale_factor, th=10.0, orb_dist=100, check_orientation=True):
        """ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) on records (corb_track_search_reloc): the frame = this store's cur_slot,
        pKF = kf_slot of kf_store, sAlreadyFound = the MapPoints the frame holds.  Returns (match per frame feature = pKF feature or -1, matches); the ids go into the record."""
        n = self._n_features(cur_slot)
        m = np.full(n, -1, np.int32); cnt = C.c_int(0); a = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        _chk(load().corb_track_search_reloc(self.h, cur_slot, kf_store.h, kf_slot, mp_store.h, C.byref(cam), _p(a), log_scale_factor, th,
                                            orb_dist, bool(check_orientation), _p(m), C.byref(cnt)), "corb_track_search_reloc")
        return m, cnt.value

    def SearchBySim3(self, slot1, slot2, mp_store, cam, log_scale_factor, T1w, T2w, s12, R12, t12, th=7.5, matched12_ids=None):
        """ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) on records (corb_search_by_sim3_store).  Returns (match12 = KF2 feature per KF1 feature or -1,
        the MapPoint ids those features hold, matches found)."""
        n1 = self._n_features(slot1)
        m = np.full(n1, -1, np.int32); ids = np.full(n1, NO_MAP_POINT, np.uint64); cnt = C.c_int(0)
        a = np.ascontiguousarray(T1w, np.float32).reshape(16); b = np.ascontiguousarray(T2w, np.float32).reshape(16)
        R = np.ascontiguousarray(R12, np.float32).reshape(9); t = np.ascontiguousarray(t12, np.float32).reshape(3)
        mi = None if matched12_ids is None else np.ascontiguousarray(matched12_ids, np.uint64)
        _chk(load().corb_search_by_sim3_store(self.h, slot1, slot2, mp_store.h, C.byref(cam), log_scale_factor, _p(a), _p(b), _p(mi) if mi is not None else None,
                                              s12, _p(R), _p(t), th, _p(m), _p(ids), C.byref(cnt)), "corb_search_by_sim3_store")
        return m, ids, cnt.value

    def Sim3Ransac(self, slot1, slots2, mp_store, cam1, cams2, matched12_ids, rand_values, probability=0.99, min_inliers=20, max_iterations=300, fix_scale=False, max_events=None):
        """Sim3Solver's constructor and RANSAC on records for the candidates slots2 of keyframe slot1 (corb_sim3_ransac_store).  matched12_ids [n_candidates, n(slot1)] =
        vpMatched12 as MapPoint ids; cams2 = one TrackCamera per candidate.  Returns per candidate what Sim3Ransac returns (inliers per feature of slot1 = vbInliers),
        plus n_corr and index1 (mvnIndices1)."""
        sl = np.ascontiguousarray(slots2, np.int32).reshape(-1); n = len(sl); n1 = self._n_features(slot1)
        max_events = max_iterations if max_events is None else int(max_events)
        ids = np.ascontiguousarray(matched12_ids, np.uint64).reshape(-1); rv = np.ascontiguousarray(rand_values, np.int32).reshape(-1)
        assert len(ids) == n * n1 and len(rv) == n * max_iterations * 3 and len(cams2) == n
        cams = (TrackCamera * max(n, 1))(*cams2)
        m = max(n, 1)
        cap = np.zeros(m, np.int32); n_ev = np.zeros(m, np.int32); ev = np.zeros((m, max(max_events, 1)), SIM3_EVENT_DTYPE)
        fl = np.zeros((m, max(max_events, 1), max(n1, 1)), np.uint8); cnt = np.zeros((m, max_iterations), np.int32); qo = np.zeros((m, max_iterations, 4), np.float32)
        nc = np.zeros(m, np.int32); ix = np.full((m, max(n1, 1)), -1, np.int32)
        _chk(load().corb_sim3_ransac_store(self.h, slot1, _p(sl), n, mp_store.h, C.byref(cam1), C.cast(cams, C.c_void_p), _p(ids), probability, min_inliers,
                                           max_iterations, bool(fix_scale), _p(rv), max_events, _p(cap), _p(n_ev), _p(ev), _p(fl), _p(nc), _p(ix), _p(cnt), _p(qo)),
             "corb_sim3_ransac_store")
        out = []
        for c in range(n):
            r = _sim3_ransac_result(c, n_ev, max_events, cap, ev, fl, cnt, qo)
            r["inliers"] = r["inliers"][:, :n1]; r["n_corr"] = int(nc[c]); r["index1"] = ix[c, : nc[c]].copy()
            out.append(r)
        return out

    def _n_features(self, slot):
        n = load().corb_kf_store_count(self.h, slot)
        if n < 0:
            raise RuntimeError("slot %d holds no frame with a host-known feature count" % slot)
        return n

    def _n_any(self, slot):
        """feature count of a slot: the host's mirror, or (a slot filled from a device-side count) the record's"""
        n = load().corb_kf_store_count(self.h, slot)
        return n if n >= 0 else len(self.get(slot)["kp"])

    def set_meta(self, slot, **kw):
        """pose, intrinsics, ids, flags of the keyframe (KeyFrame.h:65-79); unspecified fields keep the record's values"""
        m = self.get_meta(slot)
        for k, v in kw.items():
            m[k] = np.asarray(v).reshape(m[k].shape) if m[k].shape else v
        _chk(load().corb_kf_store_set_meta(self.h, slot, _p(m)), "corb_kf_store_set_meta")

    def set_meta_raw(self, slot, meta):
        """corb_kf_store_set_meta with a complete KF_META_DTYPE record (no read-modify-write)"""
        m = np.ascontiguousarray(meta, KF_META_DTYPE)
        _chk(load().corb_kf_store_set_meta(self.h, slot, _p(m)), "corb_kf_store_set_meta")

    def get_meta(self, slot):
        m = np.zeros((), KF_META_DTYPE)
        _chk(load().corb_kf_store_get_meta(self.h, slot, _p(m)), "corb_kf_store_get_meta")
        return m

    def set_map_points(self, slot, mp_id):
        a = np.ascontiguousarray(mp_id, np.uint64)
        _chk(load().corb_kf_store_set_map_points(self.h, slot, _p(a)), "corb_kf_store_set_map_points")

    def get_map_points(self, slot):
        a = np.zeros(self.F, np.uint64)
        _chk(load().corb_kf_store_get_map_points(self.h, slot, _p(a), self.F), "corb_kf_store_get_map_points")
        return a[: self._n_any(slot)].copy()

    def SearchByBoW(self, slot_a, other, slot_b, nnratio=0.6, checkOri=True, variant=0):
        na = self._n_any(slot_a); nb = other._n_any(slot_b)
        out = np.full(max(nb if variant == 0 else na, 1), -1, np.int32); n = C.c_int(0)
        _chk(load().corb_search_by_bow_slots(variant, self.h, slot_a, other.h, slot_b, nnratio, bool(checkOri), _p(out), C.byref(n)), "corb_search_by_bow_slots")
        return out[: (nb if variant == 0 else na)], n.value

    def SearchByBoW_batch(self, slots_a, other, slots_b, nnratio=0.6, checkOri=True, variant=0, stride=None):
        """corb_search_by_bow_slots_batch: SearchByBoW for the pairs (slots_a[p], slots_b[p]) -> (match[n_pairs, stride], counts[n_pairs]); a row holds -1 behind its
        length.  stride=None: the longest row."""
        a = np.ascontiguousarray(slots_a, np.int32).reshape(-1); b = np.ascontiguousarray(slots_b, np.int32).reshape(-1)
        if len(a) != len(b):
            raise CorbError("KeyFrameStore.SearchByBoW_batch: the slot lists differ in length")
        if stride is None:
            stride = max([other._n_any(int(s)) for s in set(b.tolist())] if variant == 0 else [self._n_any(int(s)) for s in set(a.tolist())], default=0)
        match = np.full((len(a), stride), -1, np.int32); counts = np.zeros(len(a), np.int32)
        _chk(load().corb_search_by_bow_slots_batch(variant, self.h, _p(a), other.h, _p(b), len(a), nnratio, bool(checkOri), stride, _p(match), _p(counts)), "corb_search_by_bow_slots_batch")
        return match, counts

    def SearchForTriangulation(self, slot_a, other, slot_b, F12, ex, ey, scale2, sigma2_2, bOnlyStereo, checkOri=True):
        na = self._n_any(slot_a)
        F12 = np.ascontiguousarray(F12, np.float32); sc = np.ascontiguousarray(scale2, np.float32); sg = np.ascontiguousarray(sigma2_2, np.float32)
        pairs = np.zeros((max(na, 1), 2), np.int32); n = C.c_int(0)
        _chk(load().corb_search_for_triangulation_slots(self.h, slot_a, other.h, slot_b, _p(F12), ex, ey, _p(sc), _p(sg), len(sc), bool(bOnlyStereo), bool(checkOri), _p(pairs), C.byref(n)),
             "corb_search_for_triangulation_slots")
        return pairs[: n.value].copy(), n.value


def map_fusion_candidates(db, sub, query_slots, query_entries, query_ids, glob, entry_slot, nnratio=0.75, checkOri=True, min_matches=15, cap_rows=None, cap_ids=None):
    """corb_map_fusion_candidates_store: detectKeyFrameInServerMap's detection, matching and discarding for every keyframe of a submap -> (rows, offsets, ids):
    rows (FUSION_ROW_DTYPE) in detection order, rows[offsets[i] : offsets[i + 1]] those of query i, ids the map-point ids of the kept rows (a row's start: ids_offset).
    cap_rows=None / cap_ids=None leave room for every entry per query and for every row with a record."""
    qs = np.ascontiguousarray(query_slots, np.int32).reshape(-1); qe = np.ascontiguousarray(query_entries, np.int32).reshape(-1); qi = np.ascontiguousarray(query_ids, np.uint64).reshape(-1)
    es = np.ascontiguousarray(entry_slot, np.int32).reshape(-1)
    if not (len(qs) == len(qe) == len(qi)) or len(es) != db.capacity:
        raise CorbError("map_fusion_candidates: the query lists differ in length, or entry_slot does not have one entry per database entry")
    cap_rows = len(qs) * db.capacity if cap_rows is None else cap_rows
    if cap_ids is None:
        cap_ids = int((es >= 0).sum()) * sum(max(sub._n_any(int(s)), 0) for s in qs)
    off = np.zeros(len(qs) + 1, np.int32); rows = np.zeros(max(cap_rows, 1), FUSION_ROW_DTYPE); ids = np.zeros(max(cap_ids, 1), np.uint64)
    n_rows = C.c_int(0); n_ids = C.c_int64(0)
    rc = load().corb_map_fusion_candidates_store(db.h, sub.h, _p(qs), _p(qe), _p(qi), len(qs), glob.h, _p(es), nnratio, bool(checkOri), min_matches,
                                                 _p(off), _p(rows), cap_rows, C.byref(n_rows), _p(ids), cap_ids, C.byref(n_ids))
    map_fusion_candidates.last = (rc, n_rows.value, n_ids.value)
    _chk(rc, "corb_map_fusion_candidates_store")
    return rows[:n_rows.value].copy(), off, ids[:n_ids.value].copy()


class MapPointStore(_Handle):
    """Device-resident map-point store (corb_mp_store_*): one fixed-size record per MapPoint -- header (MapPoint.h:52-72) + observation list."""

    _destroy = "corb_mp_store_destroy"

    def __init__(self, capacity, max_obs=32, device=0):
        self.capacity = capacity; self.O = max_obs; self.device = device
        self._create("corb_mp_store_create", device, capacity, max_obs)

    def record_bytes(self):
        return load().corb_mp_store_record_bytes(self.h)

    def put(self, first, records, obs_offset, obs_kf_id, obs_idx):
        rec = np.ascontiguousarray(records, MP_RECORD_DTYPE); off = np.ascontiguousarray(obs_offset, np.int32)
        okf = np.ascontiguousarray(obs_kf_id, np.uint64); oi = np.ascontiguousarray(obs_idx, np.uint32)
        _chk(load().corb_mp_store_put_host(self.h, first, len(rec), _p(rec), _p(off), _p(okf), _p(oi)), "corb_mp_store_put_host")

    def get(self, first, n):
        rec = np.zeros(n, MP_RECORD_DTYPE); okf = np.zeros((n, self.O), np.uint64); oi = np.zeros((n, self.O), np.uint32)
        _chk(load().corb_mp_store_get(self.h, first, n, _p(rec), _p(okf), _p(oi)), "corb_mp_store_get")
        return rec, okf, oi

    def set_counters(self, first, visible, found, replaced_by=None):
        """mnVisible / mnFound / mpReplaced (0 = none, else id + 1) of the records first .. (the header's spare 16 bytes)"""
        n = len(visible); a = np.zeros(n, MP_COUNTERS_DTYPE); a["n_visible"] = visible; a["n_found"] = found
        if replaced_by is not None: a["replaced_by"] = replaced_by
        _chk(load().corb_mp_store_set_counters(self.h, first, n, _p(a)), "corb_mp_store_set_counters")

    def get_counters(self, first, n):
        a = np.zeros(n, MP_COUNTERS_DTYPE)
        _chk(load().corb_mp_store_get_counters(self.h, first, n, _p(a)), "corb_mp_store_get_counters")
        return a

    def set_scratch(self, first, scratch):
        """CorbMapPointScratch of the records first ..: the tracking / local-mapping / loop-closing fields of MapPoint's serialised state the header does not carry"""
        a = np.ascontiguousarray(scratch, MP_SCRATCH_DTYPE)
        _chk(load().corb_mp_store_set_scratch(self.h, first, len(a), _p(a)), "corb_mp_store_set_scratch")

    def get_scratch(self, first, n):
        a = np.zeros(n, MP_SCRATCH_DTYPE)
        _chk(load().corb_mp_store_get_scratch(self.h, first, n, _p(a)), "corb_mp_store_get_scratch")
        return a

    def Replace(self, slot_this, slot_into, kf_store, kf_first, kf_n):
        """MapPoint::Replace(pMP) on records (corb_mp_store_replace): returns 0 (done) or 1 (the same point)"""
        st = C.c_int(0)
        _chk(load().corb_mp_store_replace(self.h, slot_this, slot_into, kf_store.h, kf_first, kf_n, C.byref(st)), "corb_mp_store_replace")
        return st.value

    def build_index(self, first, n):
        """corb_mp_store_build_index: the mnId -> slot table the tracking calls on records look map points up in"""
        _chk(load().corb_mp_store_build_index(self.h, first, n), "corb_mp_store_build_index")


class KeyframeInserter(_Handle):
    """Keyframe insertion on records (include/corb_keyframe_insert.h): the stereo points of CreateNewKeyFrame / StereoInitialization / UpdateLastFrame, the counts of
    NeedNewKeyFrame, ProcessNewKeyFrame's association loop and MapPointCulling.  One handle per client: it owns the calls' device scratch and a stream.  A call that
    answers CORB_ERR_CAPACITY returns its complete outputs with capacity_error = True instead of raising (nothing was written)."""

    _destroy = "corb_kfi_destroy"

    def __init__(self, max_features, max_recent, device=0):
        self.F = max_features; self.R = max_recent
        self._create("corb_kfi_create", device, max_features, max_recent)

    @staticmethod
    def _rc(rc, what):
        if rc != ERR_CAPACITY:
            _chk(rc, what)
        return rc == ERR_CAPACITY

    def CreateStereoPoints(self, kf, slot, mp_store, cam, th_depth, mode=1, apply=False, first_mp_slot=0, first_mp_id=0, client_id=0, frame_id=0, mirror=None, mirror_slot=-1):
        """corb_kfi_create_stereo_points: dict(order, kind, x3d, n_visited, n_created, capacity_error)"""
        n = max(kf._n_features(slot), 1)
        order = np.zeros(n, np.int32); kind = np.zeros(n, np.uint8); x3d = np.zeros((n, 3), np.float32); nv = C.c_int(0); nc = C.c_int(0)
        rc = load().corb_kfi_create_stereo_points(self.h, kf.h, slot, mp_store.h, C.byref(cam), th_depth, mode, bool(apply), first_mp_slot,
                                                  first_mp_id, client_id, frame_id, mirror.h if mirror is not None else None, mirror_slot,
                                                  _p(order), _p(kind), _p(x3d), C.byref(nv), C.byref(nc))
        full = self._rc(rc, "corb_kfi_create_stereo_points")
        return dict(order=order[: nv.value].copy(), kind=kind[: nv.value].copy(), x3d=x3d[: nc.value].copy(), n_visited=nv.value, n_created=nc.value, capacity_error=full)

    def NeedKeyFrameCounts(self, frames, cur_slot, mp_store, th_depth, kf, ref_slot, min_obs, kf_first, kf_n):
        """corb_kfi_need_keyframe_counts: (nTrackedClose, nNonTrackedClose, nRefMatches)"""
        a = C.c_int(0); b = C.c_int(0); c = C.c_int(0)
        _chk(load().corb_kfi_need_keyframe_counts(self.h, frames.h, cur_slot, mp_store.h, th_depth, kf.h, ref_slot, min_obs, kf_first, kf_n,
                                                  C.byref(a), C.byref(b), C.byref(c)), "corb_kfi_need_keyframe_counts")
        return a.value, b.value, c.value

    def ProcessNewKeyFrame(self, kf, slot, mp_store, kf_first, kf_n, scale_factor=1.2, apply=False):
        """corb_kfi_process_new_keyframe: dict(kind, recent_slots, n_added, capacity_error)"""
        n = max(kf._n_features(slot), 1)
        kind = np.zeros(n, np.uint8); recent = np.zeros(n, np.int32); na = C.c_int(0); nr = C.c_int(0)
        rc = load().corb_kfi_process_new_keyframe(self.h, kf.h, slot, mp_store.h, kf_first, kf_n, scale_factor, bool(apply), _p(kind), _p(recent),
                                                  C.byref(na), C.byref(nr))
        full = self._rc(rc, "corb_kfi_process_new_keyframe")
        return dict(kind=kind[: kf._n_features(slot)].copy(), recent_slots=recent[: nr.value].copy(), n_added=na.value, capacity_error=full)

    def MapPointCulling(self, mp_store, recent_slots, cur_kf_id, th_obs, kf, kf_first, kf_n, apply=False):
        """corb_kfi_map_point_culling: dict(decision, kept_slots, n_culled)"""
        sl = np.ascontiguousarray(recent_slots, np.int32); n = len(sl)
        dec = np.zeros(max(n, 1), np.uint8); kept = np.zeros(max(n, 1), np.int32); nk = C.c_int(0); ncu = C.c_int(0)
        _chk(load().corb_kfi_map_point_culling(self.h, mp_store.h, _p(sl) if n else None, n, cur_kf_id, th_obs, kf.h, kf_first, kf_n, bool(apply),
                                               _p(dec), _p(kept), C.byref(nk), C.byref(ncu)), "corb_kfi_map_point_culling")
        return dict(decision=dec[:n].copy(), kept_slots=kept[: nk.value].copy(), n_culled=ncu.value)


def publish_message_layout(counts, kf_record_bytes, mp_record_bytes):
    """corb_pub_message_layout: byte offsets of sections A..E and the message's size.  Pure host arithmetic."""
    c = np.ascontiguousarray(counts, np.int32); off = np.zeros(6, np.int64)
    _chk(load().corb_pub_message_layout(_p(c), kf_record_bytes, mp_record_bytes, _p(off)), "corb_pub_message_layout")
    return off


class _PublishResult:
    """the caller's arrays of a CorbPublishOutputs, sized from the counts and the rooms, and the dict they make"""

    def __init__(self, counts, kf_room, mp_room):
        self.counts = [int(x) for x in counts[:4]]
        self.kinds = [np.zeros(max(n, 1), np.uint8) for n in self.counts]
        self.kf_slots = np.zeros(max(min(self.counts[0], kf_room), 1), np.int32); self.mp_slots = np.zeros(max(min(self.counts[1], mp_room), 1), np.int32)
        self.c = _PublishOutputs(_p(self.kinds[0]), _p(self.kinds[1]), _p(self.kinds[2]), _p(self.kinds[3]), _p(self.kf_slots), _p(self.mp_slots), 0, 0, 0, 0, 0)

    def as_dict(self, counts=None, capacity_error=False):
        n = self.counts if counts is None else [int(x) for x in counts[:4]]
        c = self.c
        return dict(kind_kf_new=self.kinds[0][: n[0]].copy(), kind_mp_new=self.kinds[1][: n[1]].copy(), kind_kf_upd=self.kinds[2][: n[2]].copy(), kind_mp_upd=self.kinds[3][: n[3]].copy(),
                    kf_new_slots=self.kf_slots[: min(c.n_kf_inserted, len(self.kf_slots))].copy(), mp_new_slots=self.mp_slots[: min(c.n_mp_inserted, len(self.mp_slots))].copy(),
                    n_kf_inserted=c.n_kf_inserted, n_mp_inserted=c.n_mp_inserted, n_kf_updated=c.n_kf_updated, n_mp_updated=c.n_mp_updated, no_transform=c.no_transform,
                    capacity_error=capacity_error)


class MapPublisher(_Handle):
    """The server -> clients publish on records (include/corb_map_publish.h): pack on the server's stores, apply on a client's.  One handle per rank: it owns the
    message buffer, the calls' device scratch and a stream.  An apply that answers CORB_ERR_CAPACITY returns its complete outputs with capacity_error = True
    instead of raising (nothing was written)."""

    _destroy = "corb_pub_destroy"

    def __init__(self, device=0):
        self.device = device
        self._create("corb_pub_create", device)

    @staticmethod
    def _pack_args(kf, new_kf_slots, upd_kf_slots, mp, new_mp_slots, upd_mp_slots, trans):
        """trans: {client id: 4x4} or a list of (client id, 4x4) (a list may name an id twice: the call refuses it)"""
        items = sorted(trans.items()) if isinstance(trans, dict) else list(trans)
        ids = np.array([int(k) for k, _ in items], np.int32); T = np.ascontiguousarray([np.asarray(t, np.float32).reshape(16) for _, t in items], np.float32).reshape(-1, 16)
        lists = [np.ascontiguousarray(x, np.int32) for x in (new_kf_slots, upd_kf_slots, new_mp_slots, upd_mp_slots)]
        return ids, T, lists

    def pack(self, kf, new_kf_slots=(), upd_kf_slots=(), mp=None, new_mp_slots=(), upd_mp_slots=(), trans=()):
        """corb_pub_pack: the five sections into the handle's message buffer"""
        ids, T, (a, c, b, d) = self._pack_args(kf, new_kf_slots, upd_kf_slots, mp, new_mp_slots, upd_mp_slots, trans)
        _chk(load().corb_pub_pack(self.h, kf.h if kf is not None else None, _p(a) if len(a) else None, len(a), _p(c) if len(c) else None, len(c),
                                  mp.h if mp is not None else None, _p(b) if len(b) else None, len(b), _p(d) if len(d) else None, len(d),
                                  _p(ids) if len(ids) else None, _p(T) if len(ids) else None, len(ids)), "corb_pub_pack")

    def message(self):
        """corb_pub_message: dict(ptr, bytes, counts, kf_record_bytes, mp_record_bytes) of the last pack"""
        ptr = C.c_void_p(); n = C.c_int64(0); counts = np.zeros(5, np.int32); kb = C.c_int32(0); mb = C.c_int32(0)
        _chk(load().corb_pub_message(self.h, C.byref(ptr), C.byref(n), _p(counts), C.byref(kb), C.byref(mb)), "corb_pub_message")
        return dict(ptr=ptr.value, bytes=n.value, counts=counts, kf_record_bytes=kb.value, mp_record_bytes=mb.value)

    def message_bytes(self):
        """corb_pub_message_read: the message on the host"""
        m = self.message(); buf = np.zeros(max(m["bytes"], 1), np.uint8)
        _chk(load().corb_pub_message_read(self.h, _p(buf), m["bytes"]), "corb_pub_message_read")
        return buf[: m["bytes"]]

    def apply(self, msg, client_id, kf, kf_first, kf_n, kf_free_first, kf_room, mp=None, mp_first=0, mp_n=0, mp_free_first=0, mp_room=0, apply=True):
        """corb_pub_apply of a message() dict (this handle's or another's on the same device): the outputs as a dict"""
        counts = np.ascontiguousarray(msg["counts"], np.int32)
        r = _PublishResult(counts, kf_room if kf is not None else 0, mp_room if mp is not None else 0)
        rc = load().corb_pub_apply(self.h, msg["ptr"], _p(counts), msg["kf_record_bytes"], msg["mp_record_bytes"], client_id, kf.h if kf is not None else None, kf_first, kf_n,
                                   kf_free_first, kf_room, mp.h if mp is not None else None, mp_first, mp_n, mp_free_first, mp_room, bool(apply), C.byref(r.c))
        if rc != ERR_CAPACITY:
            _chk(rc, "corb_pub_apply")
        return r.as_dict(capacity_error=rc == ERR_CAPACITY)


def map_publish_plan(headers, root):
    """corb_map_publish_plan: (verdict code, failing rank) of a publish from what the ranks contributed to the header all-gather.  Pure host arithmetic."""
    h = np.ascontiguousarray(headers, PUBLISH_HEADER_DTYPE); who = C.c_int(-1)
    rc = load().corb_map_publish_plan(len(h), root, _p(h), C.byref(who))
    return rc, who.value


def map_publish_messages(headers, rank, root):
    """corb_map_publish_messages: (sends, recvs) rank `rank` posts for a publish with these gathered headers.  Pure host arithmetic."""
    h = np.ascontiguousarray(headers, PUBLISH_HEADER_DTYPE); W = len(h)
    sends = np.zeros(max(W, 1), PUSH_MSG_DTYPE); recvs = np.zeros(1, PUSH_MSG_DTYPE); ns = C.c_int(0); nr = C.c_int(0)
    _chk(load().corb_map_publish_messages(W, rank, root, _p(h), _p(sends), C.byref(ns), _p(recvs), C.byref(nr)), "corb_map_publish_messages")
    return sends[: ns.value].copy(), recvs[: nr.value].copy()


def map_push_plan(headers, root, kf_capacity, mp_capacity, kf_dst_first, mp_dst_first=None):
    """corb_map_push_plan: (verdict code, failing rank) of a push from what the ranks contributed to the header all-gather.  Pure host arithmetic."""
    h = np.ascontiguousarray(headers, PUSH_HEADER_DTYPE)
    kd = None if kf_dst_first is None else np.ascontiguousarray(kf_dst_first, np.int32); md = None if mp_dst_first is None else np.ascontiguousarray(mp_dst_first, np.int32)
    who = C.c_int(-1)
    rc = load().corb_map_push_plan(len(h), root, _p(h), kf_capacity, mp_capacity, _p(kd), _p(md), C.byref(who))
    return rc, who.value


def map_push_messages(headers, rank, root, kf_dst_first=None, mp_dst_first=None):
    """corb_map_push_messages: (sends, recvs) rank `rank` posts for a push with these gathered headers.  Pure host arithmetic."""
    h = np.ascontiguousarray(headers, PUSH_HEADER_DTYPE); W = len(h)
    kd = None if kf_dst_first is None else np.ascontiguousarray(kf_dst_first, np.int32); md = None if mp_dst_first is None else np.ascontiguousarray(mp_dst_first, np.int32)
    sends = np.zeros(2, PUSH_MSG_DTYPE); recvs = np.zeros(2 * W, PUSH_MSG_DTYPE); ns = C.c_int(0); nr = C.c_int(0)
    _chk(load().corb_map_push_messages(W, rank, root, _p(h), _p(kd), _p(md), _p(sends), C.byref(ns), _p(recvs), C.byref(nr)), "corb_map_push_messages")
    return sends[: ns.value].copy(), recvs[: nr.value].copy()


def rccl_exchange_with_fake(sends, recvs, fail_at=None):
    """corb_comm_test_rccl_exchange: the RCCL branch's posting loop on a recording fake of ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd (no GPU, no librccl).
    Returns (return code, call log); fail_at = index of the send / recv call (0-based, sends first) that returns an error."""
    log = []; n = [0]
    def gs(): log.append(("group_start",)); return 0
    def ge(): log.append(("group_end",)); return 0
    def snd(buf, count, dt, peer, comm, stream):
        log.append(("send", int(peer), int(count), int(dt))); n[0] += 1; return 1 if fail_at is not None and n[0] - 1 == fail_at else 0
    def rcv(buf, count, dt, peer, comm, stream):
        log.append(("recv", int(peer), int(count), int(dt))); n[0] += 1; return 1 if fail_at is not None and n[0] - 1 == fail_at else 0
    f = _RcclFns(); keep = (_RcclFns._fields_[0][1](gs), _RcclFns._fields_[1][1](ge), _RcclFns._fields_[2][1](snd), _RcclFns._fields_[3][1](rcv))
    f.group_start, f.group_end, f.send, f.recv = keep
    sm = np.ascontiguousarray(sends, PUSH_MSG_DTYPE); rm = np.ascontiguousarray(recvs, PUSH_MSG_DTYPE)
    rc = load().corb_comm_test_rccl_exchange(C.byref(f), _p(sm) if len(sm) else None, len(sm), _p(rm) if len(rm) else None, len(rm))
    return rc, log


def RebaseMapStore(To2n, kf, kf_slots, mp=None, mp_slots=()):
    """MapFusion::insertServerMapToGlobleMap on store records (in place on the device)"""
    T = np.ascontiguousarray(To2n, np.float32).reshape(16); ks = np.ascontiguousarray(kf_slots, np.int32); ms = np.ascontiguousarray(mp_slots, np.int32)
    _chk(load().corb_rebase_map_store(_p(T), kf.h if kf is not None else None, _p(ks) if len(ks) else None, len(ks), mp.h if mp is not None else None, _p(ms) if len(ms) else None, len(ms)),
         "corb_rebase_map_store")


def GlobalBundleAdjustemntStore(kf, kf_slots, mp, mp_slots, nIterations=10, bRobust=False, nLoopKF=0, solver=0, pcg_tol=0.0, pcg_max_iter=0, pc_block=0, fetch=True, pc_multilevel=0, scale_factor=0.0):
    """Optimizer::GlobalBundleAdjustemnt on store records (corb_ba_solve_store): graph built on the device, estimates written back into the records
    (scale_factor > 0 with nLoopKF == 0: UpdateNormalAndDepth on the records as well)"""
    ks = np.ascontiguousarray(kf_slots, np.int32); ms = np.ascontiguousarray(mp_slots, np.int32)
    oposes = np.zeros((len(ks), 16), np.float32) if fetch else None; opoints = np.zeros((len(ms), 3), np.float32) if fetch else None
    chi2 = np.zeros(nIterations + 1, np.float64); lam = np.zeros(max(nIterations, 1), np.float64)
    res = _BAResult(_p(oposes), _p(opoints), _p(chi2), _p(lam), 0, 0, 0, 0, 0, 0, 0, 0, 0)
    opt = BAOptions(solver, pcg_tol, pcg_max_iter, pc_block, pc_multilevel, scale_factor)
    _chk(load().corb_ba_solve_store(kf.h, _p(ks), len(ks), mp.h, _p(ms), len(ms), nIterations, bool(bRobust), None, nLoopKF, C.byref(res), C.byref(opt)), "corb_ba_solve_store")
    return dict(poses=None if oposes is None else oposes.reshape(-1, 4, 4), points=opoints, chi2=chi2[: res.iters_done + 1], lam=lam[: res.iters_done], iters_done=res.iters_done,
                trials=res.trials_total, solver=res.solver_used, pcg_iterations=res.pcg_iterations,
                structure=dict(free_poses=res.free_poses, free_points=res.free_points, active_edges=res.active_edges, nnz_blocks=res.nnz_blocks, schur_pairs=res.schur_pairs, pc_block=res.pc_block, pc_levels=res.pc_levels),
                certificate=dict(pcg_residual_max=res.pcg_residual_max, pcg_residual_last=res.pcg_residual_last, grad_inf=res.grad_inf, pcg_refined_trials=res.pcg_refined_trials),
                ms=dict(total=res.ms_total, build=res.ms_build, schur=res.ms_schur, solve=res.ms_solve, update=res.ms_update))


def LocalBundleAdjustmentStore(kf, kf_slots, n_local, mp, mp_slots, scale_factor=1.2, apply_erase=True, stages=None, stop=None, solver=0):
    """Optimizer::LocalBundleAdjustment on store records (corb_local_ba_store): kf_slots = lLocalKeyFrames (the first n_local) + lFixedCameras, mp_slots =
    lLocalMapPoints.  The records receive the poses / positions, vToErase (apply_erase) and UpdateNormalAndDepth; returns the estimates and the erased
    observations as (index into kf_slots, index into mp_slots) rows."""
    ks = np.ascontiguousarray(kf_slots, np.int32); ms = np.ascontiguousarray(mp_slots, np.int32)
    stages = LOCAL_BA_STAGES if stages is None else stages
    oposes = np.zeros((len(ks), 16), np.float32); opoints = np.zeros((len(ms), 3), np.float32)
    res = _BAResult(_p(oposes), _p(opoints), None, None, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    st = (BAStage * len(stages))(*[BAStage(*s) for s in stages])
    cap = max(1, len(ms) * max(1, len(ks)))
    pairs = np.zeros((cap, 2), np.int32); ne = C.c_int(0)
    one = C.c_int(1)
    sp = None if stop is None else (C.cast(C.byref(one), C.c_void_p) if stop == "before" else C.cast(C.byref(res, _BAResult.iters_done.offset), C.c_void_p))
    opt = BAOptions(solver, 0.0, 0, 0, 0)
    _chk(load().corb_local_ba_store(kf.h, _p(ks), n_local, len(ks), mp.h, _p(ms), len(ms), st, len(stages), scale_factor, bool(apply_erase), sp,
                                    C.byref(res), _p(pairs), cap, C.byref(ne), C.byref(opt)), "corb_local_ba_store")
    return dict(poses=oposes.reshape(-1, 4, 4), points=opoints, erase=pairs[: ne.value].copy(), iters_done=res.iters_done, trials=res.trials_total, ms_total=res.ms_total,
                structure=dict(free_poses=res.free_poses, free_points=res.free_points, active_edges=res.active_edges, nnz_blocks=res.nnz_blocks, schur_pairs=res.schur_pairs),
                device_route=bool(res.reserved0))


class Comm(_Handle):
    """RCCL communicator of the client / server ranks (corb_comm_*): rank 0 creates the 128-byte id, every rank gets it by the job's own means."""
    _destroy = "corb_comm_destroy"

    @staticmethod
    def unique_id():
        b = (C.c_char * 128)()
        _chk(load().corb_comm_unique_id(b), "corb_comm_unique_id")
        return bytes(b)

    def __init__(self, unique_id, rank, world, device=0):
        self.rank = rank; self.world = world
        self._create("corb_comm_create", (C.c_char * 128).from_buffer_copy(unique_id), rank, world, device)

    @classmethod
    def local(cls, world, devices=None):
        """corb_comm_create_local: `world` communicators over the in-process transport (one host thread per rank)"""
        arr = (C.c_void_p * world)()
        dv = None if devices is None else np.ascontiguousarray(devices, np.int32)
        _chk(load().corb_comm_create_local(world, _p(dv), arr), "corb_comm_create_local")
        return [cls._adopt(arr[r], rank=r, world=world) for r in range(world)]

    def map_push(self, store, slots, root=0, dst_first=None):
        """corb_map_push: every rank sends the records of `slots` to `root`, which files rank r's records from slot dst_first[r] on; returns the per-rank counts on the root"""
        sl = np.ascontiguousarray(slots, np.int32)
        df = None if dst_first is None else np.ascontiguousarray(dst_first, np.int32)
        cnt = np.zeros(self.world, np.int32)
        _chk(load().corb_map_push(self.h, store.h, _p(sl) if len(sl) else None, len(sl), root, _p(df), _p(cnt)), "corb_map_push")
        return cnt if self.rank == root else None

    def map_push_ex(self, kf, kf_slots, mp=None, mp_slots=(), root=0, kf_dst_first=None, mp_dst_first=None):
        """corb_map_push_ex: keyframe AND map-point records to the root; returns (kf counts, mp counts) on the root"""
        ks = np.ascontiguousarray(kf_slots, np.int32); ms = np.ascontiguousarray(mp_slots, np.int32)
        kd = None if kf_dst_first is None else np.ascontiguousarray(kf_dst_first, np.int32); md = None if mp_dst_first is None else np.ascontiguousarray(mp_dst_first, np.int32)
        kc = np.zeros(self.world, np.int32); mc = np.zeros(self.world, np.int32)
        p = _MapPush(kf.h if kf is not None else None, _p(ks) if len(ks) else None, len(ks), mp.h if mp is not None else None, _p(ms) if len(ms) else None, len(ms),
                     _p(kd), _p(md), _p(kc), _p(mc))
        _chk(load().corb_map_push_ex(self.h, C.byref(p), root), "corb_map_push_ex")
        return (kc, mc) if self.rank == root else None

    def map_publish(self, pub, root=0, pack=None, apply=None, max_counts=None):
        """corb_map_publish (collective).  The root passes pack = dict(kf, new_kf_slots, upd_kf_slots, mp, new_mp_slots, upd_mp_slots, trans) and gets None; every
        other rank passes apply = dict(client_id, kf, kf_first, kf_n, kf_free_first, kf_room, mp, mp_first, mp_n, mp_free_first, mp_room, apply) and max_counts =
        the largest (A, B, C, D) counts it expects, and gets corb_pub_apply's outputs as a dict (the kind arrays have max_counts entries)."""
        if pack is not None:
            ids, T, (a, c, b, d) = MapPublisher._pack_args(pack.get("kf"), pack.get("new_kf_slots", ()), pack.get("upd_kf_slots", ()), pack.get("mp"), pack.get("new_mp_slots", ()),
                                                           pack.get("upd_mp_slots", ()), pack.get("trans", ()))
            kf, mp = pack.get("kf"), pack.get("mp")
            p = _PublishPack(kf.h if kf is not None else None, _p(a) if len(a) else None, len(a), _p(c) if len(c) else None, len(c), mp.h if mp is not None else None,
                             _p(b) if len(b) else None, len(b), _p(d) if len(d) else None, len(d), _p(ids) if len(ids) else None, _p(T) if len(ids) else None, len(ids))
            _chk(load().corb_map_publish(self.h, pub.h, root, C.byref(p), None), "corb_map_publish")
            return None
        kf, mp = apply.get("kf"), apply.get("mp")
        r = _PublishResult(max_counts, apply.get("kf_room", 0) if kf is not None else 0, apply.get("mp_room", 0) if mp is not None else 0)
        q = _PublishApply(int(apply["client_id"]), kf.h if kf is not None else None, int(apply.get("kf_first", 0)), int(apply.get("kf_n", 0)), int(apply.get("kf_free_first", 0)),
                          int(apply.get("kf_room", 0)), mp.h if mp is not None else None, int(apply.get("mp_first", 0)), int(apply.get("mp_n", 0)), int(apply.get("mp_free_first", 0)),
                          int(apply.get("mp_room", 0)), bool(apply.get("apply", True)), C.pointer(r.c))
        rc = load().corb_map_publish(self.h, pub.h, root, None, C.byref(q))
        if rc != ERR_CAPACITY:
            _chk(rc, "corb_map_publish")
        return r.as_dict(capacity_error=rc == ERR_CAPACITY)

    def map_push_setup(self, root, kf=None, mp=None, kf_dst_first=None, mp_dst_first=None):
        """corb_map_push_setup (collective, once): the root's layout to every rank, for the asynchronous pushes"""
        kd = None if kf_dst_first is None else np.ascontiguousarray(kf_dst_first, np.int32); md = None if mp_dst_first is None else np.ascontiguousarray(mp_dst_first, np.int32)
        _chk(load().corb_map_push_setup(self.h, root, kf.h if kf is not None else None, mp.h if mp is not None else None, _p(kd), _p(md)), "corb_map_push_setup")

    def map_push_begin(self, kf, kf_slots, mp=None, mp_slots=(), root=0):
        """corb_map_push_begin: one header all-gather, records enqueued; returns at once (map_push_wait completes it and returns the counts on the root)"""
        ks = np.ascontiguousarray(kf_slots, np.int32); ms = np.ascontiguousarray(mp_slots, np.int32)
        kc = np.zeros(self.world, np.int32); mc = np.zeros(self.world, np.int32)
        p = _MapPush(kf.h if kf is not None else None, _p(ks) if len(ks) else None, len(ks), mp.h if mp is not None else None, _p(ms) if len(ms) else None, len(ms),
                     None, None, _p(kc), _p(mc))
        self._flight = (ks, ms, kc, mc, p, root)                # (the arrays the C side keeps pointers to until the wait)
        _chk(load().corb_map_push_begin(self.h, C.byref(p), root), "corb_map_push_begin")

    def map_push_wait(self):
        _chk(load().corb_map_push_wait(self.h), "corb_map_push_wait")
        fl = getattr(self, "_flight", None); self._flight = None
        return (fl[2], fl[3]) if fl is not None and self.rank == fl[5] else None

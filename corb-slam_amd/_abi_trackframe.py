"""The ninth header, include/corb_track_frame.h, for Python: its prototypes, its two structs and bind_trackframe(), which load() calls after _abi.bind(),
bind_fusion() and bind_tracklocal().

Like _abi_fusion.py and _abi_tracklocal.py this is a table of its own only because tests/test_abi_table.py pins _abi.PROTOTYPES to the six earlier headers and
their struct count; whoever next edits that test should fold the seventh, the eighth and the ninth table into _abi.py's single one.
tests/test_abi_trackframe_table.py gives this table the checks the six have.  The three exported functions forward to file-local *_call functions for the reason
corb_fusion.cpp's do (marked TO FOLD BACK in csrc/corb_trackframe.cpp)."""
import ctypes as C

from ._abi import CorbError, TrackCamera


class TrackFrameParams(C.Structure):
    """CorbTrackFrameParams: what Tracking holds beside the frames when TrackWithMotionModel / TrackReferenceKeyFrame runs"""
    _fields_ = [("frame_id", C.c_uint64), ("sensor", C.c_int32), ("only_tracking", C.c_int32), ("check_replaced", C.c_int32), ("check_orientation", C.c_int32),
                ("nnratio", C.c_float), ("th", C.c_float)]


class TrackFrameResult(C.Structure):
    """CorbTrackFrameResult: the counts of the chain's steps, its decisions, the function's return and the three poses"""
    _fields_ = [("n_matches_first", C.c_int32), ("searched_wide", C.c_int32), ("n_matches", C.c_int32), ("th_used", C.c_float), ("n_pose_inliers", C.c_int32),
                ("n_matches_kept", C.c_int32), ("n_matches_map", C.c_int32), ("vo", C.c_int32), ("ok", C.c_int32),
                ("Tlw", C.c_float * 16), ("Tcw_pred", C.c_float * 16), ("Tcw", C.c_float * 16)]


TRACKFRAME_STRUCTS = {"CorbTrackFrameParams": TrackFrameParams, "CorbTrackFrameResult": TrackFrameResult}


def _prototypes():
    P, I = C.c_void_p, C.c_int
    cam, par, res = C.POINTER(TrackCamera), C.POINTER(TrackFrameParams), C.POINTER(TrackFrameResult)
    return {"corb_track_frame.h": {
        "corb_track_with_motion_model": (I, [P, I, I, P, I, P, cam, P, P, par, P, P, res]),
        "corb_track_reference_keyframe": (I, [P, I, I, P, I, P, cam, P, par, P, P, res]),
        "corb_track_frame_finish": (I, [P, I, P, I, P, I, P]),
    }}


TRACKFRAME_PROTOTYPES = _prototypes()
TRACKFRAME_EXPORTS = tuple(TRACKFRAME_PROTOTYPES["corb_track_frame.h"])


def bind_trackframe(lib):
    """restype and argtypes of every TRACKFRAME_PROTOTYPES entry onto the opened library `lib`; CorbError names a missing function with its header"""
    for header, fns in TRACKFRAME_PROTOTYPES.items():
        for name, (restype, argtypes) in fns.items():
            if not hasattr(lib, name):
                raise CorbError("libcorb_accel.so lacks %s (include/%s): rebuild it" % (name, header))
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib


__all__ = ["TrackFrameParams", "TrackFrameResult", "TRACKFRAME_STRUCTS", "TRACKFRAME_PROTOTYPES", "TRACKFRAME_EXPORTS", "bind_trackframe"]

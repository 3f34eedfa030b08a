"""The eighth header, include/corb_track_local_map.h, for Python: its prototypes, its two structs and bind_tracklocal(), which load() calls after _abi.bind() and
bind_fusion().

Like _abi_fusion.py this is a table of its own only because tests/test_abi_table.py pins _abi.PROTOTYPES to the six earlier headers and their struct count; whoever
next edits that test should fold the seventh and the eighth table into _abi.py's single one.  tests/test_abi_tracklocal_table.py gives this table the checks the
six have.  The two exported functions forward to file-local *_call functions for the reason corb_fusion.cpp's do (marked TO FOLD BACK in csrc/corb_tracklocal.cpp)."""
import ctypes as C

from ._abi import CorbError, LocalMap, TrackCamera


class TrackLocalMapParams(C.Structure):
    """CorbTrackLocalMapParams: what Tracking holds beside the frame when TrackLocalMap runs"""
    _fields_ = [("frame_id", C.c_uint64), ("last_reloc_frame_id", C.c_uint64), ("max_frames", C.c_int32), ("sensor", C.c_int32), ("only_tracking", C.c_int32),
                ("log_scale_factor", C.c_float), ("nnratio", C.c_float), ("th", C.c_float)]


class TrackLocalMapResult(C.Structure):
    """CorbTrackLocalMapResult: CorbLocalMap, the counts of the three steps, mnMatchesInliers, TrackLocalMap's return, the threshold used and the pose"""
    _fields_ = [("local", LocalMap), ("n_in_view", C.c_int32), ("n_matches", C.c_int32), ("n_pose_inliers", C.c_int32), ("n_matches_inliers", C.c_int32),
                ("ok", C.c_int32), ("th_used", C.c_float), ("Tcw", C.c_float * 16)]


TRACKLOCAL_STRUCTS = {"CorbTrackLocalMapParams": TrackLocalMapParams, "CorbTrackLocalMapResult": TrackLocalMapResult}


def _prototypes():
    P, I, U64, PI = C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_int)
    return {"corb_track_local_map.h": {
        "corb_track_local_map": (I, [P, P, I, C.POINTER(TrackCamera), P, P, I, C.POINTER(TrackLocalMapParams), P, I, P, P, I, P, P, C.POINTER(TrackLocalMapResult)]),
        "corb_track_local_map_stats": (I, [P, I, P, I, I, U64, U64, I, C.POINTER(C.c_int32), PI]),
    }}


TRACKLOCAL_PROTOTYPES = _prototypes()
TRACKLOCAL_EXPORTS = tuple(TRACKLOCAL_PROTOTYPES["corb_track_local_map.h"])


def bind_tracklocal(lib):
    """restype and argtypes of every TRACKLOCAL_PROTOTYPES entry onto the opened library `lib`; CorbError names a missing function with its header"""
    for header, fns in TRACKLOCAL_PROTOTYPES.items():
        for name, (restype, argtypes) in fns.items():
            if not hasattr(lib, name):
                raise CorbError("libcorb_accel.so lacks %s (include/%s): rebuild it" % (name, header))
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib


__all__ = ["TrackLocalMapParams", "TrackLocalMapResult", "TRACKLOCAL_STRUCTS", "TRACKLOCAL_PROTOTYPES", "TRACKLOCAL_EXPORTS", "bind_tracklocal"]

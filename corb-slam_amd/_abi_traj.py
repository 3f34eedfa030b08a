"""The tenth header, include/corb_trajectory.h, for Python: its prototypes, its two structs and bind_traj(), which load() calls after _abi.bind(), bind_fusion(),
bind_tracklocal() and bind_trackframe().

Like _abi_fusion.py, _abi_tracklocal.py and _abi_trackframe.py this is a table of its own only because tests/test_abi_table.py pins _abi.PROTOTYPES to the six earlier
headers and their struct count; whoever next edits that test should fold the seventh to the tenth table into _abi.py's single one.
tests/test_abi_traj_table.py gives this table the checks the six have.  No call of this header opens a workspace lane, so its exported functions are what they
seem: there is no forwarder to fold back."""
import ctypes as C

import numpy as np

from ._abi import CorbError


class TrajEntry(C.Structure):
    """CorbTrajEntry: one frame of the log (mlRelativeFramePoses, mlpReferences, mlFrameTimes, mlbLost)"""
    _fields_ = [("Tcr", C.c_float * 16), ("ref_id", C.c_uint64), ("timestamp", C.c_double), ("ref_slot", C.c_int32), ("lost", C.c_int32)]


class TrajStats(C.Structure):
    """CorbTrajStats: what an export of the frames met"""
    _fields_ = [("n_entries", C.c_int32), ("n_rows", C.c_int32), ("n_lost_skipped", C.c_int32), ("n_ref_gone", C.c_int32), ("n_chain_broken", C.c_int32),
                ("max_chain", C.c_int32)]


TRAJ_STRUCTS = {"CorbTrajEntry": TrajEntry, "CorbTrajStats": TrajStats}
TRAJ_ENTRY_DTYPE = np.dtype([("Tcr", np.float32, 16), ("ref_id", np.uint64), ("timestamp", np.float64), ("ref_slot", np.int32), ("lost", np.int32)])
assert TRAJ_ENTRY_DTYPE.itemsize == C.sizeof(TrajEntry) == 88
TRAJ_KITTI, TRAJ_TUM, TRAJ_KEYFRAME_TUM = 0, 1, 2


def _prototypes():
    P, I, D, Z = C.c_void_p, C.c_int, C.c_double, C.c_size_t
    ent, st = C.POINTER(TrajEntry), C.POINTER(TrajStats)
    return {"corb_trajectory.h": {
        "corb_traj_create": (I, [P, I, P]),
        "corb_traj_destroy": (None, [P]),
        "corb_traj_reset": (I, [P]),
        "corb_traj_append": (I, [P, P, I, I, P, D, I]),
        "corb_traj_set_keyframe_time": (I, [P, I, D]),
        "corb_traj_get_keyframe_time": (I, [P, I, P]),
        "corb_traj_set_bad_pose": (I, [P, I]),
        "corb_traj_set_tcp": (I, [P, I, P]),
        "corb_traj_get_tcp": (I, [P, I, P]),
        "corb_traj_get_entries": (I, [P, ent, I, P]),
        "corb_traj_frames": (I, [P, I, I, P, P, P, I, P, st]),
        "corb_traj_keyframes": (I, [P, P, P, P, I, P]),
        "corb_traj_format_rows": (I, [I, P, P, I, P, Z, P]),
        "corb_traj_save": (I, [P, I, I, C.c_char_p]),
    }}


TRAJ_PROTOTYPES = _prototypes()
TRAJ_EXPORTS = tuple(TRAJ_PROTOTYPES["corb_trajectory.h"])


def bind_traj(lib):
    """restype and argtypes of every TRAJ_PROTOTYPES entry onto the opened library `lib`; CorbError names a missing function with its header"""
    for header, fns in TRAJ_PROTOTYPES.items():
        for name, (restype, argtypes) in fns.items():
            if not hasattr(lib, name):
                raise CorbError("libcorb_accel.so lacks %s (include/%s): rebuild it" % (name, header))
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib


__all__ = ["TrajEntry", "TrajStats", "TRAJ_STRUCTS", "TRAJ_ENTRY_DTYPE", "TRAJ_KITTI", "TRAJ_TUM", "TRAJ_KEYFRAME_TUM", "TRAJ_PROTOTYPES", "TRAJ_EXPORTS", "bind_traj"]

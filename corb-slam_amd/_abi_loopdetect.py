"""The eleventh header, include/corb_loop_detect.h, for Python: its prototypes, its struct and bind_loopdetect(), which load() calls after _abi.bind(), bind_fusion(),
bind_tracklocal(), bind_trackframe() and bind_traj().

Like _abi_fusion.py, _abi_tracklocal.py, _abi_trackframe.py and _abi_traj.py this is a table of its own only because tests/test_abi_table.py pins _abi.PROTOTYPES to
the six earlier headers and their struct count; whoever next edits that test should fold the seventh to the eleventh table into _abi.py's single one.
tests/test_abi_loopdetect_table.py gives this table the checks the six have.  No call of this header opens a workspace lane, so its exported functions are what
they seem: there is no forwarder to fold back."""
import ctypes as C

import numpy as np

from ._abi import CorbError


class LoopDetectResult(C.Structure):
    """CorbLoopDetectResult: one keyframe's DetectLoop"""
    _fields_ = [("outcome", C.c_int32), ("min_score_bits", C.c_uint32), ("n_candidates", C.c_int32), ("n_enough", C.c_int32), ("n_groups", C.c_int32)]


LOOPDETECT_STRUCTS = {"CorbLoopDetectResult": LoopDetectResult}
LOOP_RESULT_DTYPE = np.dtype([("outcome", np.int32), ("min_score_bits", np.uint32), ("n_candidates", np.int32), ("n_enough", np.int32), ("n_groups", np.int32)])
assert LOOP_RESULT_DTYPE.itemsize == C.sizeof(LoopDetectResult) == 20
LOOP_GAP, LOOP_NONE, LOOP_NOT_ENOUGH, LOOP_DETECTED = 0, 1, 2, 3
LOOP_DETECT_MAX_QUEUE = 64


def _prototypes():
    P, I = C.c_void_p, C.c_int
    res = C.POINTER(LoopDetectResult)
    return {"corb_loop_detect.h": {
        "corb_loop_detector_create": (I, [P, P, I, I, P]),
        "corb_loop_detector_destroy": (None, [P]),
        "corb_loop_detector_bind": (I, [P, P, P, I]),
        "corb_loop_detector_set_last_loop": (I, [P, C.c_uint64]),
        "corb_loop_detector_get_last_loop": (I, [P, P]),
        "corb_loop_detector_reset": (I, [P]),
        "corb_loop_detector_clear_groups": (I, [P]),
        "corb_loop_detector_drop_slot": (I, [P, I]),
        "corb_loop_detector_get_groups": (I, [P, P, P, P, I, I, P, P]),
        "corb_loop_detect": (I, [P, I, res, P, P, P]),
        "corb_loop_detect_queue": (I, [P, P, I, res, P, P, P, P]),
    }}


LOOPDETECT_PROTOTYPES = _prototypes()
LOOPDETECT_EXPORTS = tuple(LOOPDETECT_PROTOTYPES["corb_loop_detect.h"])


def bind_loopdetect(lib):
    """restype and argtypes of every LOOPDETECT_PROTOTYPES entry onto the opened library `lib`; CorbError names a missing function with its header"""
    for header, fns in LOOPDETECT_PROTOTYPES.items():
        for name, (restype, argtypes) in fns.items():
            if not hasattr(lib, name):
                raise CorbError("libcorb_accel.so lacks %s (include/%s): rebuild it" % (name, header))
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib


__all__ = ["LoopDetectResult", "LOOPDETECT_STRUCTS", "LOOP_RESULT_DTYPE", "LOOP_GAP", "LOOP_NONE", "LOOP_NOT_ENOUGH", "LOOP_DETECTED", "LOOP_DETECT_MAX_QUEUE",
           "LOOPDETECT_PROTOTYPES", "LOOPDETECT_EXPORTS", "bind_loopdetect"]

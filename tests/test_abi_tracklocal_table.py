"""CPU tests of the Python mirror of the eighth header (corb-slam_amd/_abi_tracklocal.py against include/corb_track_local_map.h): what tests/test_abi_table.py checks
for the six and tests/test_abi_fusion_table.py for the seventh -- prototypes in header order with the declarations' kinds, the two structs' layouts from a gcc-built
C11 program, the loaded library carrying the table, the symbols exported, the missing-symbol message -- that the earlier tables are untouched, and that the C++
mirror and the adapter compile with -Wall -Werror against the test doubles."""
import ctypes as C
import os
import re
import subprocess
import pytest
import test_abi_table as T

HEADER = "corb_track_local_map.h"
FUNCTIONS = ("corb_track_local_map", "corb_track_local_map_stats")
STRUCTS = ("CorbTrackLocalMapParams", "CorbTrackLocalMapResult")
CTYPE_OF = {"uint64_t": C.c_uint64, "int32_t": C.c_int32, "float": C.c_float}


def _declarations():
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(corb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", T._source(HEADER)):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        assert name not in out
        params = [a.strip() for a in args.split(",")]
        out[name] = (T._c_kind(ret, True), [T._c_kind(p) for p in params], params)
    return out


def _struct_fields(corb):
    """{struct: [(C type, field name, array length or 0)]} from the header, in declaration order"""
    structs = re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(Corb\w+)\s*;", T._source(HEADER))
    assert tuple(n for _, n in structs) == STRUCTS == tuple(corb.TRACKLOCAL_STRUCTS)
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
    assert tuple(corb.TRACKLOCAL_PROTOTYPES) == (HEADER,) and tuple(decl) == FUNCTIONS == corb.TRACKLOCAL_EXPORTS == tuple(corb.TRACKLOCAL_PROTOTYPES[HEADER])
    mirrors = dict(corb.TRACKLOCAL_STRUCTS, CorbTrackCamera=corb.TrackCamera)
    for name, (ret, kinds, params) in decl.items():
        restype, argtypes = corb.TRACKLOCAL_PROTOTYPES[HEADER][name]
        got = [T._ctypes_kind(t) for t in argtypes]
        assert ret == "i32" == T._ctypes_kind(restype) and got == kinds and not any(k.startswith("unknown") for k in kinds + got), (name, kinds, got)
        for p, t in zip(params, argtypes):                       # a typed pointer names the mirror of the struct declared at that position
            m = re.match(r"(?:const )?(Corb\w+)\s*\*", p)
            if m and m.group(1) in mirrors:
                assert t._type_ is mirrors[m.group(1)], (name, p)


def test_the_earlier_tables_are_untouched(corb):
    assert tuple(corb.PROTOTYPES) == T.HEADERS and HEADER not in corb.PROTOTYPES and HEADER not in corb.FUSION_PROTOTYPES
    earlier = set(n for fns in list(corb.PROTOTYPES.values()) + list(corb.FUSION_PROTOTYPES.values()) for n in fns)
    assert not set(FUNCTIONS) & earlier and not set(STRUCTS) & (set(corb.STRUCTS) | set(corb.DTYPES) | set(corb.FUSION_STRUCTS))
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
        cls = corb.TRACKLOCAL_STRUCTS[s]
        assert [f for _, f, _ in fields[s]] == [f for f, _ in cls._fields_]
        want[s + ".size"] = C.sizeof(cls)
        for ctype, f, length in fields[s]:
            want["%s.%s" % (s, f)] = getattr(cls, f).offset
            t = dict(cls._fields_)[f]
            base = corb.LocalMap if ctype == "CorbLocalMap" else CTYPE_OF[ctype]
            assert t is (base * length if length else base) or (length and t._type_ is base and t._length_ == length), (s, f)
    assert got == want


def test_the_loaded_library_carries_the_table(corb):
    L = corb.load()
    for name, (restype, argtypes) in corb.TRACKLOCAL_PROTOTYPES[HEADER].items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    raw = C.CDLL(corb.LIB_PATH)                                # the two symbols are exported: a plain dlsym finds them
    for name in FUNCTIONS:
        assert C.cast(getattr(raw, name), C.c_void_p).value, name


def test_bind_tracklocal_names_a_missing_function_and_its_header(corb):
    class Lib:
        pass
    with pytest.raises(corb.CorbError, match=r"libcorb_accel.so lacks corb_track_local_map \(include/corb_track_local_map.h\): rebuild it"):
        corb.bind_tracklocal(Lib())


def test_the_mirror_and_the_adapter_compile_against_the_test_doubles(tmp_path):
    """tests/host/tracklocal_adapter_main.cpp (run on the GPU by tests/test_gpu_tracklocal.py) compiles with -Wall -Werror; it is not linked here"""
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-c", "-I", os.path.join(T.ROOT, "include"), "-I", os.path.join(T.ROOT, "corb-slam_amd", "host"),
                           "-I", os.path.join(T.ROOT, "tests", "host"), os.path.join(T.ROOT, "tests", "host", "tracklocal_adapter_main.cpp"), "-o", str(tmp_path / "main.o")])

"""CPU tests of the Python mirror of the seventh header (corb-slam_amd/_abi_fusion.py against include/corb_map_fusion.h): what tests/test_abi_table.py checks for
the six -- prototype kinds against the declarations, CorbFusionRow's layout from a gcc-built C11 program, the loaded library carrying the table, the symbols
exported -- and that the six headers' own table is untouched."""
import ctypes as C
import os
import re
import subprocess
import pytest
import test_abi_table as T

HEADER = "corb_map_fusion.h"
FUNCTIONS = ("corb_kfdb_detect_batch", "corb_search_by_bow_slots_batch", "corb_map_fusion_candidates_store")


def _declarations():
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(corb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", T._source(HEADER)):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        assert name not in out
        params = [a.strip() for a in args.split(",")]
        out[name] = (T._c_kind(ret, True), [T._c_kind(p) for p in params])
    return out


def test_every_prototype_agrees_with_its_header_declaration(corb):
    decl = _declarations()
    assert tuple(corb.FUSION_PROTOTYPES) == (HEADER,) and tuple(decl) == FUNCTIONS == corb.FUSION_EXPORTS == tuple(corb.FUSION_PROTOTYPES[HEADER])
    for name, (ret, kinds) in decl.items():
        restype, argtypes = corb.FUSION_PROTOTYPES[HEADER][name]
        got = [T._ctypes_kind(t) for t in argtypes]
        assert ret == "i32" == T._ctypes_kind(restype) and got == kinds and not any(k.startswith("unknown") for k in kinds + got), (name, kinds, got)


def test_the_six_headers_table_is_untouched(corb):
    assert tuple(corb.PROTOTYPES) == T.HEADERS and HEADER not in corb.PROTOTYPES
    assert not set(FUNCTIONS) & set(n for fns in corb.PROTOTYPES.values() for n in fns) and not set(corb.FUSION_STRUCTS) & (set(corb.STRUCTS) | set(corb.DTYPES))
    assert corb.ABI_VERSION == 6 and re.search(r"#define\s+CORB_ABI_VERSION\s+6\b", open(os.path.join(T.ROOT, "include", "corb_accel.h")).read())


def test_fusion_row_has_the_compilers_layout(corb, tmp_path):
    structs = re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(Corb\w+)\s*;", T._source(HEADER))
    assert [n for _, n in structs] == ["CorbFusionRow"] == list(corb.FUSION_STRUCTS)
    d = corb.FUSION_STRUCTS["CorbFusionRow"]
    fields = [re.search(r"(\w+)$", part.strip()).group(1) for decl in structs[0][0].split(";") if decl.strip() for part in decl.split(",")]
    assert fields == list(d.names)
    lines = ['printf("size %zu\\n", sizeof(CorbFusionRow));'] + ['printf("%s %%zu\\n", offsetof(CorbFusionRow, %s));' % (f, f) for f in fields]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <%s>\nint main(void) {\n%s\nreturn 0; }\n" % (HEADER, "\n".join(lines)))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(T.ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = dict((k, int(v)) for k, v in (l.split() for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines()))
    assert got == dict([("size", d.itemsize)] + [(f, d.fields[f][1]) for f in fields])
    assert [d.fields[f][0].str for f in fields] == ["<i4"] * 5 + ["<i8"]


def test_the_loaded_library_carries_the_table(corb):
    L = corb.load()
    for name, (restype, argtypes) in corb.FUSION_PROTOTYPES[HEADER].items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    raw = C.CDLL(corb.LIB_PATH)                                # the three symbols are exported: a plain dlsym finds them
    for name in FUNCTIONS:
        assert C.cast(getattr(raw, name), C.c_void_p).value, name


def test_bind_fusion_names_a_missing_function_and_its_header(corb):
    class Lib:
        pass
    with pytest.raises(corb.CorbError, match=r"libcorb_accel.so lacks corb_kfdb_detect_batch \(include/corb_map_fusion.h\): rebuild it"):
        corb.bind_fusion(Lib())

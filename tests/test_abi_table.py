"""CPU tests of the Python mirror of the C ABI (corb-slam_amd/_abi.py): every prototype against the headers' declarations, every structure mirror and record dtype
against the compiler's layout, and the one handle owner of the package on a recording fake.  No GPU and, for the handle owner, no library."""
import ctypes as C
import os
import re
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("corb_accel.h", "corb_voc_train.h", "corb_keyframe_insert.h", "corb_map_publish.h", "corb_essential_graph.h", "corb_stereo_rectify.h")
N_FUNCTIONS = 199               # what the six headers declare today; a parse that finds another number has lost or invented declarations

N_STRUCTS = 57                  # the `typedef struct { ... } CorbX;` blocks of the six headers today; a parse that finds another number has dropped or invented one

C_KIND = {"int": "i32", "int32_t": "i32", "uint32_t": "u32", "unsigned": "u32", "unsigned int": "u32", "int64_t": "i64", "uint64_t": "u64", "size_t": "u64",
          "float": "f32", "double": "f64"}
CTYPES_KIND = {C.c_int32: "i32", C.c_uint32: "u32", C.c_int64: "i64", C.c_uint64: "u64", C.c_size_t: "u64", C.c_float: "f32", C.c_double: "f64",
               C.c_void_p: "ptr", C.c_char_p: "ptr", None: "void"}


def _source(header):
    """the header without comments and preprocessor lines"""
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return "\n".join(l for l in src.split("\n") if not l.lstrip().startswith("#"))


def _c_kind(decl, is_return=False):
    """kind of a parameter declaration `type name` (or of a return type); the pointed-to struct's name for a pointer to a Corb struct"""
    decl = " ".join(decl.split())
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in decl.split(" ") if w != "const"]
    if not is_return:
        words = words[:-1]                                   # the parameter's name
    t = " ".join(words)
    return "void" if t == "void" else C_KIND.get(t, "unknown: " + decl)


def _declarations():
    """{function: (header, return kind, [parameter kinds], [parameter declarations])} of the six headers"""
    out = {}
    for h in HEADERS:
        for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(corb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", _source(h)):
            ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
            assert name not in out, "%s is declared twice" % name
            params = [] if args in ("", "void") else [a.strip() for a in args.split(",")]
            out[name] = (h, _c_kind(ret, True), [_c_kind(p) for p in params], params)
    return out


def _ctypes_kind(t):
    if t in CTYPES_KIND:
        return CTYPES_KIND[t]
    return "ptr" if isinstance(t, type) and issubclass(t, C._Pointer) else "unknown: %r" % (t,)


def _table(corb):
    return dict((name, (h,) + tuple(proto)) for h, fns in corb.PROTOTYPES.items() for name, proto in fns.items())


def test_every_prototype_agrees_with_its_header_declaration(corb):
    decl = _declarations(); table = _table(corb)
    assert len(decl) == N_FUNCTIONS == len(table) == sum(len(f) for f in corb.PROTOTYPES.values())
    assert set(decl) == set(table)
    assert tuple(corb.PROTOTYPES) == HEADERS
    bad = []
    for name, (h, ret, kinds, params) in decl.items():
        th, restype, argtypes = table[name]
        got = [_ctypes_kind(t) for t in argtypes]
        assert ret in ("void", "i32", "ptr"), (name, ret)
        assert not any(k.startswith("unknown") for k in kinds + got + [_ctypes_kind(restype)]), (name, kinds, got)
        if th != h or _ctypes_kind(restype) != ret or got != kinds:
            bad.append((name, h, th, ret, _ctypes_kind(restype), kinds, got))
    assert not bad, bad


def test_typed_pointers_name_the_mirror_of_the_declared_struct(corb):
    """where a prototype says POINTER(T) and not void*, T is the mirror registered under the C struct the header names at that position"""
    decl = _declarations(); table = _table(corb); typed = 0
    for name, (h, ret, kinds, params) in decl.items():
        for p, t in zip(params, table[name][2]):
            m = re.match(r"(?:const\s+)?(Corb\w+)\s*\*", p)
            if m and isinstance(t, type) and issubclass(t, C._Pointer) and issubclass(t._type_, C.Structure):
                assert corb.STRUCTS.get(m.group(1)) is t._type_, (name, p, t)
                typed += 1
    in_table = sum(1 for h, restype, argtypes in table.values() for t in argtypes if isinstance(t, type) and issubclass(t, C._Pointer) and issubclass(t._type_, C.Structure))
    assert typed == in_table > 0                             # every typed pointer of the table met the struct name of its declaration


def test_the_loaded_library_carries_the_table(corb):
    L = corb.load()
    for name, (h, restype, argtypes) in _table(corb).items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # the export lists are views of the table: same members, types and grouping as the headers
    assert isinstance(corb.EXPORTS, list) and corb.EXPORTS == list(corb.PROTOTYPES["corb_accel.h"])
    for lst, h in ((corb.TRAIN_EXPORTS, "corb_voc_train.h"), (corb.KFINSERT_EXPORTS, "corb_keyframe_insert.h"), (corb.PUBLISH_EXPORTS, "corb_map_publish.h"),
                   (corb.ESSGRAPH_EXPORTS, "corb_essential_graph.h"), (corb.RECTIFY_EXPORTS, "corb_stereo_rectify.h")):
        assert isinstance(lst, tuple) and lst == tuple(corb.PROTOTYPES[h]) and not set(lst) & set(corb.EXPORTS)


def test_bind_names_a_missing_function_and_its_header(corb):
    class Lib:                                               # a library of the right layout version that exports nothing else
        def corb_abi_version(self):
            return corb.ABI_VERSION
    with pytest.raises(corb.CorbError, match=r"libcorb_accel.so lacks corb_last_error \(include/corb_accel.h\): rebuild it"):
        corb.bind(Lib())
    Lib.corb_abi_version = lambda self: corb.ABI_VERSION + 1
    with pytest.raises(corb.CorbError, match="struct layout version %d, this harness mirrors %d" % (corb.ABI_VERSION + 1, corb.ABI_VERSION)):
        corb.bind(Lib())


def _header_structs():
    """{C struct name: [field names]} of every `typedef struct ... { ... } CorbX;` of the six headers"""
    out = {}
    for h in HEADERS:
        for m in re.finditer(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(Corb\w+)\s*;", _source(h)):
            fields = []
            for d in m.group(1).split(";"):
                d = " ".join(d.split())
                if not d:
                    continue
                fp = re.search(r"\(\s*\*\s*(\w+)\s*\)", d)   # a function pointer member
                for part in ([fp.group(0)] if fp else d.split(",")):
                    fields.append(re.search(r"(\w+)\s*\)?\s*(\[[^\]]*\]\s*)*$", part.strip()).group(1))
            out[m.group(2)] = fields
    return out


def test_every_header_struct_is_mirrored_or_listed(corb):
    structs = _header_structs()
    assert len(structs) == N_STRUCTS and "CorbKeyPoint" in structs and "CorbRectifyConfig" in structs
    assert sum(len(re.findall(r"\}\s*Corb\w+\s*;", _source(h))) for h in HEADERS) == N_STRUCTS       # (no struct body the field parse cannot read, such as a nested one)
    listed = dict(corb.NOT_MIRRORED)
    assert all(isinstance(r, str) and r.strip() for r in listed.values())
    mirrored = set(corb.STRUCTS) | set(corb.DTYPES)
    assert not set(corb.STRUCTS) & set(corb.DTYPES) and not mirrored & set(listed)
    assert mirrored | set(listed) == set(structs), sorted((mirrored | set(listed)) ^ set(structs))
    # a struct that a prototype passes as POINTER(T) has its mirror: it cannot be listed as not mirrored
    for name, (h, ret, kinds, params) in _declarations().items():
        for p, t in zip(params, _table(corb)[name][2]):
            m = re.match(r"(?:const\s+)?(Corb\w+)\s*\*", p)
            if m and t is not C.c_void_p:
                assert m.group(1) not in listed, (name, p)


def test_mirrors_have_the_compilers_layout(corb, tmp_path):
    """sizeof of every mirror and offsetof of every field of it, from a C11 program built with gcc.  Every mirror names its fields as the header does, but for the two
    renamed ones below, so no mirror is checked by its size alone."""
    renamed = {("CorbBAResult", "lam"): "lambda", ("CorbBAEdge", "ur"): "u_right"}          # (mirror, its field) -> the header's field: a keyword, and a name callers use
    structs = _header_structs(); lines = []; want = {}
    mirrors = [(n, [f[0] for f in t._fields_], C.sizeof(t), lambda f, t=t: getattr(t, f).offset) for n, t in corb.STRUCTS.items()] + \
              [(n, list(d.names), d.itemsize, lambda f, d=d: d.fields[f][1]) for n, d in corb.DTYPES.items()]
    for name, fields, size, offset in mirrors:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name)); want[name] = size
        c_fields = [renamed.get((name, f), f) for f in fields]
        assert sorted(c_fields) == sorted(structs[name]), (name, fields, structs[name])       # (order is the offsets' business: a reordered mirror fails below)
        for f, cf in zip(fields, c_fields):
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, cf)); want["%s.%s" % (name, f)] = offset(f)
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n" + "".join("#include <%s>\n" % h for h in HEADERS) + "int main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = dict((k, int(v)) for k, v in (l.split() for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines()))
    assert set(got) == set(want)
    assert got == want, sorted((k, got[k], want[k]) for k in want if got[k] != want[k])


# ---- the handle owner, on a recording fake in the place of the library ----
class _FakeLib:
    def __init__(self, fail=False):
        self.destroyed = []; self.fail = fail

    def fake_create(self, a, b, out):
        out._obj.value = 1000 + a + b
        return 0

    def fake_destroy(self, h):
        self.destroyed.append(h.value)
        if self.fail:
            raise RuntimeError("destroy failed")


@pytest.fixture
def owner(corb, monkeypatch):
    lib = _FakeLib()
    monkeypatch.setattr(corb, "load", lambda: lib)           # (the package looks `load` up at every call)

    class Owner(corb._Handle):
        _destroy = "fake_destroy"
    return Owner, lib


def test_handle_close_destroys_once(owner):
    Owner, lib = owner
    o = Owner(); o._create("fake_create", 2, 3)
    assert o.h.value == 1005 and o.h
    o.close()
    assert lib.destroyed == [1005] and not o.h
    o.close(); o.__del__()
    assert lib.destroyed == [1005] and not o.h
    with Owner._adopt(77, tag="x") as p:
        assert p.h.value == 77 and p.tag == "x" and lib.destroyed == [1005]
    assert lib.destroyed == [1005, 77] and not p.h


def test_handle_borrowed_is_never_destroyed(owner, corb):
    Owner, lib = owner
    b = Owner._adopt(55, owned=False)
    assert b.h.value == 55
    b.close(); b.__del__()
    assert lib.destroyed == [] and not b.h
    orb = corb.ORBextractor(_handle=66)                      # a front-end's extractor
    assert orb.h.value == 66
    orb.close(); orb.__del__()
    assert lib.destroyed == [] and not orb.h
    never = Owner()                                          # an object whose create never ran owns nothing
    never.close(); never.__del__()
    assert lib.destroyed == [] and not never.h


def test_handle_del_swallows_a_destroy_that_raises(owner):
    Owner, lib = owner
    lib.fail = True
    o = Owner._adopt(9)
    with pytest.raises(RuntimeError):
        o.close()                                            # close reports it ...
    assert lib.destroyed == [9] and not o.h
    q = Owner._adopt(10)
    q.__del__()                                              # ... __del__ does not
    assert lib.destroyed == [9, 10] and not q.h


def test_orb_profile_mode_reaches_the_library_unchanged(owner, corb):
    """corb_orb_profile's `enable` is a mode (0 off, 1 the product sequence, 2 every kernel unsplit on one stream): 2 must not collapse to 1"""
    Owner, lib = owner
    lib.modes = []
    lib.corb_orb_profile = lambda h, mode: lib.modes.append(mode) or 0
    orb = corb.ORBextractor(_handle=66)
    for m in (2, 1, 0, True, False):
        orb.profile(m)
    assert lib.modes == [2, 1, 0, 1, 0] and all(type(m) is int for m in lib.modes)


def test_the_twelve_handle_classes_share_the_owner(corb):
    classes = [corb.ORBextractor, corb.StereoFrontend, corb.StereoRectifier, corb.RgbdFrontend, corb.Vocabulary, corb.KeyFrameDatabase, corb.Covisibility, corb.KeyFrameStore,
               corb.MapPointStore, corb.KeyframeInserter, corb.MapPublisher, corb.Comm]
    table = _table(corb)
    for c in classes:
        assert issubclass(c, corb._Handle) and not {"close", "__del__", "__enter__", "__exit__"} & set(vars(c)), c
        assert table[c._destroy][1:] == (None, [C.c_void_p]), c
    assert len(set(c._destroy for c in classes)) == 12

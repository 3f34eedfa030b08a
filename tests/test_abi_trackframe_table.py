"""CPU tests of the Python mirror of the ninth header (corb-slam_amd/_abi_trackframe.py against include/corb_track_frame.h): what tests/test_abi_table.py checks for the
six, tests/test_abi_fusion_table.py for the seventh and tests/test_abi_tracklocal_table.py for the eighth -- prototypes in header order with the declarations'
kinds, the two structs' layouts from a gcc-built C11 program, the loaded library carrying the table, the symbols exported, the missing-symbol message -- that the
earlier tables are untouched, that the shared pose arithmetic (csrc/trackframe_math.h) is plain C++ and agrees with the definition, and that the C++ mirror's
program compiles with -Wall -Werror."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import test_abi_table as T
import trackframe_reference as R

HEADER = "corb_track_frame.h"
FUNCTIONS = ("corb_track_with_motion_model", "corb_track_reference_keyframe", "corb_track_frame_finish")
STRUCTS = ("CorbTrackFrameParams", "CorbTrackFrameResult")
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
    assert tuple(n for _, n in structs) == STRUCTS == tuple(corb.TRACKFRAME_STRUCTS)
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
    assert tuple(corb.TRACKFRAME_PROTOTYPES) == (HEADER,) and tuple(decl) == FUNCTIONS == corb.TRACKFRAME_EXPORTS == tuple(corb.TRACKFRAME_PROTOTYPES[HEADER])
    mirrors = dict(corb.TRACKFRAME_STRUCTS, CorbTrackCamera=corb.TrackCamera)
    for name, (ret, kinds, params) in decl.items():
        restype, argtypes = corb.TRACKFRAME_PROTOTYPES[HEADER][name]
        got = [T._ctypes_kind(t) for t in argtypes]
        assert ret == "i32" == T._ctypes_kind(restype) and got == kinds and not any(k.startswith("unknown") for k in kinds + got), (name, kinds, got)
        for p, t in zip(params, argtypes):                       # a typed pointer names the mirror of the struct declared at that position
            m = re.match(r"(?:const )?(Corb\w+)\s*\*", p)
            if m and m.group(1) in mirrors:
                assert t._type_ is mirrors[m.group(1)], (name, p)


def test_the_earlier_tables_are_untouched(corb):
    assert tuple(corb.PROTOTYPES) == T.HEADERS and all(HEADER not in t for t in (corb.PROTOTYPES, corb.FUSION_PROTOTYPES, corb.TRACKLOCAL_PROTOTYPES))
    assert tuple(corb.TRACKLOCAL_PROTOTYPES) == ("corb_track_local_map.h",) and corb.TRACKLOCAL_EXPORTS == ("corb_track_local_map", "corb_track_local_map_stats")
    earlier = set(n for fns in list(corb.PROTOTYPES.values()) + list(corb.FUSION_PROTOTYPES.values()) + list(corb.TRACKLOCAL_PROTOTYPES.values()) for n in fns)
    assert not set(FUNCTIONS) & earlier and not set(STRUCTS) & (set(corb.STRUCTS) | set(corb.DTYPES) | set(corb.FUSION_STRUCTS) | set(corb.TRACKLOCAL_STRUCTS))
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
        cls = corb.TRACKFRAME_STRUCTS[s]
        assert [f for _, f, _ in fields[s]] == [f for f, _ in cls._fields_]
        want[s + ".size"] = C.sizeof(cls)
        for ctype, f, length in fields[s]:
            want["%s.%s" % (s, f)] = getattr(cls, f).offset
            t = dict(cls._fields_)[f]
            base = CTYPE_OF[ctype]
            assert t is (base * length if length else base) or (length and t._type_ is base and t._length_ == length), (s, f)
    assert got == want


def test_the_loaded_library_carries_the_table(corb):
    L = corb.load()
    for name, (restype, argtypes) in corb.TRACKFRAME_PROTOTYPES[HEADER].items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    raw = C.CDLL(corb.LIB_PATH)                                # the three symbols are exported: a plain dlsym finds them
    for name in FUNCTIONS:
        assert C.cast(getattr(raw, name), C.c_void_p).value, name


def test_bind_trackframe_names_a_missing_function_and_its_header(corb):
    class Lib:
        pass
    with pytest.raises(corb.CorbError, match=r"libcorb_accel.so lacks corb_track_with_motion_model \(include/corb_track_frame.h\): rebuild it"):
        corb.bind_trackframe(Lib())


def test_the_wrappers_exist_on_the_keyframe_store(corb):
    for name in ("TrackWithMotionModel", "TrackReferenceKeyFrame", "TrackFrameFinish"):
        assert callable(getattr(corb.KeyFrameStore, name))


def test_the_shared_pose_arithmetic_is_plain_cxx_and_equals_the_definition(tmp_path):
    """csrc/trackframe_math.h in a host program built without contraction: the products, GetPoseInverse and the forward / backward test, bit for bit against
    tests/trackframe_reference.py on poses whose sums round"""
    src = tmp_path / "tfm.cpp"
    src.write_text('#include <cstdio>\n#include <cstring>\n#include <cstdint>\n#include "trackframe_math.h"\n'
                   "int main() { float A[16], B[16], C[16], D[16], E[16]; for (int i = 0; i < 16; i++) if (scanf(\"%a\", &A[i]) != 1) return 2;\n"
                   "for (int i = 0; i < 16; i++) if (scanf(\"%a\", &B[i]) != 1) return 2;\n"
                   "tfm_gemm4(A, B, C); tfm_pose_inverse(B, D); tfm_gemm4(A, D, E); int fw, bw; tfm_motion_direction(A, B, 0.25f, 0, &fw, &bw);\n"
                   "const float* M[3] = {C, D, E}; for (int k = 0; k < 3; k++) { for (int i = 0; i < 16; i++) { uint32_t u; memcpy(&u, &M[k][i], 4); printf(\"%08x \", u); } printf(\"\\n\"); }\n"
                   "printf(\"%d %d\\n\", fw, bw); return 0; }\n")
    exe = tmp_path / "tfm"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(T.ROOT, "corb-slam_amd", "csrc"), str(src), "-o", str(exe)])
    rng = np.random.default_rng(17)

    def pose(shift):
        a = rng.normal(0, 0.3, 3); th = np.linalg.norm(a); k = a / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        Rm = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        P = np.eye(4); P[:3, :3] = Rm; P[:3, 3] = rng.normal(0, 2, 3) + shift
        return P.astype(np.float32)

    for z in (0.0, 3.0, -3.0):
        A, B = pose(0), pose(np.array([0, 0, z]))
        text = " ".join(float(x).hex() for x in np.concatenate([A.reshape(16), B.reshape(16)]))
        out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
        got = [np.array([int(w, 16) for w in out[k].split()], np.uint32).view(np.float32).reshape(4, 4) for k in range(3)]
        assert got[0].tobytes() == R.gemm4(A, B).tobytes() and got[1].tobytes() == R.pose_inverse(B).tobytes() and got[2].tobytes() == R.relative_pose(A, B).tobytes()
        twc = R.camera_centre(A)
        s = np.float64(0.0)
        for k in range(3):
            s = s + np.float64(B[2, k]) * np.float64(twc[k])
        zc = np.float32(s + np.float64(B[2, 3]))
        assert out[3] == "%d %d" % (zc > 0.25, -zc > 0.25)


def test_the_mirror_program_compiles(tmp_path):
    """tests/host/trackframe_main.cpp (run on the GPU by tests/test_gpu_trackframe.py) compiles with -Wall -Werror; it is not linked here"""
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-c", "-I", os.path.join(T.ROOT, "include"), "-I", os.path.join(T.ROOT, "corb-slam_amd", "host"),
                           os.path.join(T.ROOT, "tests", "host", "trackframe_main.cpp"), "-o", str(tmp_path / "main.o")])

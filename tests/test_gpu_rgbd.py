"""GPU tests of the RGB-D / monocular front-end (corb_rgbd_*): bit-exact against the CPU restatement (tests/cam_reference.py) with the oracle's
extractor on the restated grey image."""
import ctypes
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cam_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _fe(corb, cam, max_frames=2, nfeatures=1000, **kw):
    args = {k: cam[k] for k in R.CAM_KEYS}
    args.update(kw)
    return corb.RgbdFrontend(nfeatures=nfeatures, width=cam["width"], height=cam["height"], max_frames=max_frames, **args)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, ref, what=""):
    n = len(ref["keys"])
    assert len(got["keys"]) == n > 0, what
    assert got["keys"].tobytes() == ref["keys"].tobytes(), what + ": keypoints"
    assert np.array_equal(got["desc"], ref["desc"]), what + ": descriptors"
    assert got["keys_un"].tobytes() == ref["keys_un"].tobytes(), what + ": keys_un"
    assert np.array_equal(_bits(got["u_right"]), _bits(ref["u_right"])), what + ": u_right"
    assert np.array_equal(_bits(got["depth"]), _bits(ref["depth"])), what + ": depth"


@pytest.fixture(scope="module")
def ex(pyorc):
    return pyorc.Extractor(nfeatures=1000)


CASES = [("tum1_rgb", R.TUM1, 3, 1), ("tum2_bgr", R.TUM2, 3, 0), ("tum3_rgba", R.TUM3, 4, 1), ("tum1_bgra", R.TUM1, 4, 0), ("tum2_grey", R.TUM2, 1, 1),
         ("quirk_rgb", R.QUIRK, 3, 1)]


@pytest.mark.parametrize("name,cam,channels,rgb", CASES, ids=[c[0] for c in CASES])
def test_rgbd_frames_equal_the_restatement(corb, synth, ex, name, cam, channels, rgb):
    fe = _fe(corb, cam, channels=channels, rgb=rgb)
    fr = [synth.rgbd_frame(10 + i, channels=channels) for i in range(2)]
    refs = [R.frame(ex, c, d, cam, rgb) for c, d in fr]
    packed = fe.pack_input(fr)
    fe.upload_batch(0, packed); fe.run(2); fe.sync()
    for i in range(2):
        assert np.array_equal(fe.orb.pyramid_level(i, 0), refs[i]["grey"]), "level-0 plane of frame %d" % i
        _same(fe.fetch(i), refs[i], "%s batched frame %d" % (name, i))
    one = fe.unpack_frame(fe.frames(np.ascontiguousarray(packed[1:2])))
    assert one["status"] == 0
    _same(one, refs[1], name + " corb_rgbd_frames")
    assert np.array_equal(_bits(fe.bounds()), _bits(R.image_bounds(cam)))
    if cam is R.TUM1 or cam is R.TUM2:
        d = np.concatenate([r["depth"] for r in refs])
        assert (d == -1).sum() > 10 and (d > 0).sum() > 500          # holes and valid depths both met
        raw = np.concatenate([fr[i][1][r["keys"]["y"].astype(int), r["keys"]["x"].astype(int)] for i, r in enumerate(refs)])
        assert (raw == 65535).any() and (raw == 0).any()
    if cam is R.QUIRK:
        assert one["keys_un"].tobytes() == one["keys"].tobytes()
    fe.close()


def test_batched_and_one_call_paths_agree(corb, synth, ex):
    cam = R.TUM1
    fe = _fe(corb, cam, max_frames=8)
    fr = [synth.rgbd_frame(40 + i) for i in range(8)]
    packed = fe.pack_input(fr)
    fe.upload_batch(0, packed); fe.run(8); fe.sync()
    batch = [fe.fetch(i) for i in range(8)]
    for i in (0, 5):
        _same(batch[i], R.frame(ex, *fr[i], cam), "batched frame %d" % i)
    for n in (1, 2, 3, 8, 2):
        res = fe.frames(np.ascontiguousarray(packed[8 - n:]))          # other frames in the slots than the batched run had
        for f in range(n):
            _same(fe.unpack_frame(res, f), batch[8 - n + f], "n = %d frame %d" % (n, f))
    # a batched run after the one-call path: uploads at an offset, the run covers frames 0 .. n-1
    fe.upload_batch(2, np.ascontiguousarray(packed[:3])); fe.run(5); fe.sync()
    for f in range(3):
        _same(fe.fetch(2 + f), batch[f], "offset upload frame %d" % f)
    fe.close()


def test_depth_edge_cases(corb, synth, ex):
    """f32 depth with DepthMapFactor 1 (used as it is) and 2.5 (converted), NaN, negative values, +-inf, 0, tiny and huge values at keypoint pixels"""
    c, d16 = synth.rgbd_frame(60)
    ref = R.frame(ex, c, d16, R.TUM1)
    kx, ky = ref["keys"]["x"].astype(int), ref["keys"]["y"].astype(int)
    dep = d16.astype(np.float32) * np.float32(0.0002)
    specials = [np.nan, -1.5, np.inf, 0.0, -np.inf, 1e-6, 3.0e38]
    for j, v in enumerate(specials):
        dep[ky[j::len(specials) * 3], kx[j::len(specials) * 3]] = v
    for factor in (1.0, 2.5, 1.000001):
        cam = dict(R.TUM1, depth_map_factor=factor)
        fe = _fe(corb, cam, max_frames=1, depth_format=corb.DEPTH_F32)
        r = R.frame(ex, c, dep, cam)
        got = fe.unpack_frame(fe.frames(fe.pack_input([(c, dep)])))
        _same(got, r, "f32 depth, factor %g" % factor)
        assert (r["depth"] == -1).sum() > 10 and np.isinf(r["depth"]).any()
        if factor == 1.0:                          # no conversion: the depth is the input value itself
            ok = r["depth"] > 0
            assert np.array_equal(_bits(r["depth"][ok]), _bits(dep[ky, kx][ok]))
        fe.close()


def test_monocular_euroc_and_the_initialiser_handle(corb, synth, pyorc):
    cam = R.EUROC
    fr = [synth.mono_frame(i) for i in range(2)]
    for nf in (1000, 2000):                        # Tracking::mpIniORBextractor: 2 * nFeatures until the map is initialised
        fe = _fe(corb, cam, nfeatures=nf, sensor=corb.SENSOR_MONOCULAR, channels=1)
        ex = pyorc.Extractor(nfeatures=nf)
        fe.upload_batch(0, fe.pack_input([(f, None) for f in fr])); fe.run(2); fe.sync()
        for i in range(2):
            ref = R.frame(ex, fr[i], None, cam)
            got = fe.fetch(i)
            _same(got, ref, "monocular nfeatures %d frame %d" % (nf, i))
            assert (got["u_right"] == -1).all() and (got["depth"] == -1).all()
            assert len(got["keys"]) > 0.8 * nf
        one = fe.unpack_frame(fe.frames(fe.pack_input([(fr[0], None)])))
        _same(one, R.frame(ex, fr[0], None, cam), "monocular corb_rgbd_frames")
        assert np.array_equal(_bits(fe.bounds()), _bits(R.image_bounds(cam)))
        fe.close()
    # colour monocular input (mono_tum with Camera.RGB = 1)
    col = synth.mono_frame(3, channels=3)
    fe = _fe(corb, cam, sensor=corb.SENSOR_MONOCULAR, channels=3, rgb=1)
    _same(fe.unpack_frame(fe.frames(fe.pack_input([(col, None)]))), R.frame(pyorc.Extractor(nfeatures=1000), col, None, cam, 1), "colour monocular")
    fe.close()


def test_errors(corb, synth):
    fe = _fe(corb, R.TUM1, max_frames=2)
    flat = (np.full((480, 640, 3), 128, np.uint8), np.full((480, 640), 5000, np.uint16))
    packed = fe.pack_input([flat, flat])
    o = fe.unpack_frame(fe.frames(packed), 1)
    assert len(o["keys"]) == 0 and o["status"] == 0
    fe.upload_batch(0, packed); fe.run(2); fe.sync()
    assert len(fe.fetch(0)["keys"]) == 0
    L = corb.load()
    res = np.zeros(3 * fe.layout.frame_bytes, np.uint8); big = np.zeros((3, fe.layout.input_bytes), np.uint8)
    assert L.corb_rgbd_frames(fe.h, 3, big.ctypes.data_as(ctypes.c_void_p), res.ctypes.data_as(ctypes.c_void_p), None) == -1      # CORB_ERR_ARG
    assert L.corb_rgbd_run(fe.h, 3) == -1 and L.corb_rgbd_upload_batch(fe.h, 1, 2, big.ctypes.data_as(ctypes.c_void_p)) == -1
    with pytest.raises(corb.CorbError):
        _fe(corb, R.TUM1, channels=2)
    with pytest.raises(corb.CorbError):
        _fe(corb, R.TUM1, depth_format=7)
    fe.close()


def test_store_slots_from_the_front_end(corb, synth, ex):
    """corb_kf_store_put_from_rgbd fills slots with mvKeysUn / descriptors / mvuRight / mvDepth bit for bit, and a matcher on those slots equals the same
    call on slots filled from the host with the restated arrays"""
    cam = R.TUM1
    fe = _fe(corb, cam, max_frames=2)
    c0, d0 = synth.rgbd_frame(80)
    c1 = np.ascontiguousarray(np.roll(c0, 3, axis=1)); d1 = np.ascontiguousarray(np.roll(d0, 3, axis=1))
    fr = [(c0, d0), (c1, d1)]
    fe.upload_batch(0, fe.pack_input(fr)); fe.run(2)
    cap = fe.layout.capacity
    A = corb.KeyFrameStore(4, cap); B = corb.KeyFrameStore(4, cap)
    A.put_from_rgbd(1, fe, 0, keyframe_id=501); A.put_from_rgbd(3, fe, 1, keyframe_id=502)
    fe.sync()
    refs = [R.frame(ex, c, d, cam) for c, d in fr]
    rng = np.random.default_rng(5)
    for slot, r, kid in ((1, refs[0], 501), (3, refs[1], 502)):
        g = A.get(slot)
        assert g["id"] == kid and g["kp"].tobytes() == r["keys_un"].tobytes() and np.array_equal(g["desc"], r["desc"])
        assert np.array_equal(_bits(g["u_right"]), _bits(r["u_right"])) and np.array_equal(_bits(g["depth"]), _bits(r["depth"]))
        B.put(slot, r["keys_un"], r["desc"], r["u_right"], r["depth"], keyframe_id=kid)
        fv = synth.feature_vector(len(r["keys"]), 6, rng)
        A.set_bow(slot, fv); B.set_bow(slot, fv)
        A.set_flags(slot, np.ones(len(r["keys"]), np.uint8)); B.set_flags(slot, np.ones(len(r["keys"]), np.uint8))
    ma, na = A.SearchByBoW(1, A, 3)
    mb, nb = B.SearchByBoW(1, B, 3)
    assert na == nb > 20 and np.array_equal(ma, mb)
    A.close(); B.close(); fe.close()


def test_a_run_issued_as_part_batches_equals_the_one_call_results(corb, synth):
    """32 frames: corb_rgbd_run splits the run into part-batches on two streams (as corb_orb_run does); every frame equals its corb_rgbd_frames result"""
    fe = _fe(corb, R.TUM2, max_frames=32)
    fr = [synth.rgbd_frame(90 + i) for i in range(4)]
    packed = fe.pack_input([fr[i % 4] for i in range(32)])
    one = [fe.unpack_frame(fe.frames(np.ascontiguousarray(packed[i:i + 1]))) for i in range(4)]
    one = [dict((k, v.copy() if hasattr(v, "copy") else v) for k, v in o.items()) for o in one]
    fe.upload_batch(0, packed)
    for _ in range(2):
        fe.run(32)
    fe.sync()
    o = fe.fetch_batch(0, 32)
    for f in range(32):
        n = int(o["counts"][f])
        got = dict(keys=o["keys"][f, :n], keys_un=o["keys_un"][f, :n], desc=o["desc"][f, :n], u_right=o["u_right"][f, :n], depth=o["depth"][f, :n])
        _same(got, one[f % 4], "frame %d of the split run" % f)
    fe.close()

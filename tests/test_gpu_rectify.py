"""GPU tests (pytest -m gpu) of the stereo rectifier (include/corb_stereo_rectify.h) against its definition (tests/rectify_reference.py) on the seeded inputs of
tests/rectify_cases.py, whose coverage tests/test_rectify_reference.py proves on the CPU.  Every comparison is byte for byte."""
import ctypes as C

import numpy as np
import pytest

import rectify_cases as G
import rectify_reference as R

pytestmark = pytest.mark.gpu
S = G.SMALL
ERR_ARG = -1
# a plain calibration for the small shapes (the tests that need special maps set their own)
K_S = [120, 0, 70, 0, 120, 51, 0, 0, 1]; D_S = [-0.05, 0.01, 0, 0, 0]; R_S = np.eye(3).reshape(9)
PL_S = [110, 0, 64, 0, 0, 110, 48, 0, 0, 0, 1, 0]; PR_S = [110, 0, 64, -12, 0, 110, 48, 0, 0, 0, 1, 0]


def small_handles(corb, maps=True):
    sf = corb.StereoFrontend(nfeatures=S["nfeatures"], nlevels=S["nlevels"], width=S["width"], height=S["height"], max_frames=S["max_frames"], fx=110.0, bf=12.0)
    rect = corb.StereoRectifier(sf, (K_S, D_S, R_S, PL_S), (K_S, D_S, R_S, PR_S), S["raw_width"], S["raw_height"])
    if maps:
        for eye in range(2):
            rect.set_maps(eye, *G.small_maps(eye))
    return sf, rect


@pytest.fixture(scope="module")
def small():
    raw = np.ascontiguousarray(np.stack([G.small_raw(f) for f in range(2)]))
    want = np.ascontiguousarray(np.stack([G.small_expected(f)[0] for f in range(2)]))
    return raw, want


def written(sf, res, f):
    """the header and the written part of every section of frame f's block"""
    lay = sf.frame_layout(); b = res[f * lay.frame_bytes: (f + 1) * lay.frame_bytes]
    nl, nr = (int(x) for x in b[:8].view(np.int32))
    parts = [b[:64], b[lay.off_kp_left: lay.off_kp_left + 28 * nl], b[lay.off_kp_right: lay.off_kp_right + 28 * nr], b[lay.off_desc_left: lay.off_desc_left + 32 * nl],
             b[lay.off_desc_right: lay.off_desc_right + 32 * nr], b[lay.off_u_right: lay.off_u_right + 4 * nl], b[lay.off_depth: lay.off_depth + 4 * nl]]
    return b"".join(p.tobytes() for p in parts), nl, nr


def planes(sf, n_frames):
    return np.stack([np.stack([sf.orb.pyramid_level(2 * f + e, 0) for e in range(2)]) for f in range(n_frames)])


def test_small_shapes_every_kind_byte_for_byte(corb, small):
    """129 x 97 from 141 x 103 (no width a multiple of 4), two frames, different maps per eye that hold all thirteen kinds, both ties, a negative fraction,
    fraction 31 and saturating coordinates: after upload_batch the level-0 planes of all four slots equal the definition"""
    raw, want = small
    sf, rect = small_handles(corb)
    for eye in range(2):
        mx, my = rect.maps(eye); wx, wy = G.small_maps(eye)
        assert np.array_equal(mx.view(np.uint32), wx.view(np.uint32)) and np.array_equal(my.view(np.uint32), wy.view(np.uint32))
    rect.upload_batch(0, raw)
    got = planes(sf, 2)
    assert got.shape == want.shape
    for f in range(2):
        for e in range(2):
            bad = np.argwhere(got[f, e] != want[f, e])
            assert len(bad) == 0, (f, e, len(bad), bad[:5].tolist())
    # frame 1 alone, into its own slots, from the front of the caller's block
    rect.upload_batch(1, raw[:1])
    assert np.array_equal(planes(sf, 2), np.stack([want[0], want[0]]))
    rect.close(); sf.close()


def test_the_call_equals_stereo_frames_on_the_definitions_images(corb, small):
    """corb_rect_frames on raw input = corb_stereo_frames (oracle-tested) on the same handle fed the definition's rectified images, for n = 1 and n = 2; and
    upload_batch + run + fetch = the one-call path"""
    raw, want = small
    sf, rect = small_handles(corb)
    for n in (1, 2, 1):
        a = rect.frames(raw[:n]).copy()
        assert np.array_equal(planes(sf, n), want[:n])
        b = sf.frames(want[:n]).copy()
        for f in range(n):
            wa, nl, nr = written(sf, a, f); wb, _, _ = written(sf, b, f)
            assert nl > 20 and nr > 20 and wa == wb, (n, f, nl, nr)
    kl_one = sf.unpack_frame(a, 0)["kl"].tobytes()                          # (n = 1 was the last of the loop)
    rect.upload_batch(0, raw); sf.run(2); sf.sync()
    two = rect.frames(raw)
    for f in range(2):
        o = sf.fetch(f); u = sf.unpack_frame(two, f)
        for k in ("kl", "kr", "dl", "dr", "u_right", "depth"):
            assert o[k].tobytes() == u[k].tobytes(), (f, k)
        assert o["n_matched"] == u["n_matched"] and u["status"] == 0
    assert kl_one == sf.unpack_frame(two, 0)["kl"].tobytes()
    tm = corb.StereoFrameTiming(); rect.frames(raw, timing=tm)
    assert tm.ms_upload > 0 and tm.ms_kernels > 0 and tm.ms_download > 0
    rect.close(); sf.close()


def test_euroc_settings_maps_planes_and_oracle(corb, pyorc):
    """from_settings on the EuRoC fixture, 752 x 480, 1200 features: the maps equal the definition bit for bit, the planes equal the definition, and keypoints,
    descriptors, u_right and depth equal the oracle's extractor and stereo matcher run on the definition's rectified images"""
    s = R.parse_settings(G.EUROC)
    fx, bf = s["Camera.fx"], s["Camera.bf"]
    sf = corb.StereoFrontend(nfeatures=int(s["ORBextractor.nFeatures"]), width=752, height=480, max_frames=1, fx=fx, bf=bf)
    rect = corb.StereoRectifier.from_settings(sf, G.EUROC)
    assert (rect.raw_width, rect.raw_height) == (752, 480)
    for eye in range(2):
        mx, my = rect.maps(eye); wx, wy = G.euroc_maps(eye)
        assert np.array_equal(mx.view(np.uint32), wx.view(np.uint32)) and np.array_equal(my.view(np.uint32), wy.view(np.uint32))
    raw = G.euroc_raw(); want, _ = G.euroc_expected()
    o = sf.unpack_frame(rect.frames(raw[None]))
    assert np.array_equal(planes(sf, 1)[0], want)
    el, er = pyorc.Extractor(1200, 1.2, 8, 20, 7), pyorc.Extractor(1200, 1.2, 8, 20, 7)
    kl, dl = el.extract(want[0]); kr, dr = er.extract(want[1]); tb = el.tables()
    ur, dp, nm = pyorc.stereo_match(el, er, kl, dl, kr, dr, bf, fx, tb["scale"], tb["inv_scale"])
    assert nm >= 50 and len(kl) > 1000, (nm, len(kl))                      # the seed was picked so: the comparison cannot pass empty
    assert o["kl"].tobytes() == kl.tobytes() and o["kr"].tobytes() == kr.tobytes() and np.array_equal(o["dl"], dl) and np.array_equal(o["dr"], dr)
    assert np.array_equal(o["u_right"].view(np.uint32), ur.view(np.uint32)) and np.array_equal(o["depth"].view(np.uint32), dp.view(np.uint32)) and o["n_matched"] == nm
    rect.close(); sf.close()


def test_reused_slots_and_replayed_chain(corb, small):
    """image A through maps that stay inside, then image B through the maps with outside regions on the same handle: B's bytes are those of a fresh handle (the
    remap writes the whole plane, zeros included; set_maps reaches the captured chain); a second call with the same n replays the chain"""
    raw, want = small
    j, i = np.meshgrid(np.arange(S["width"], dtype=np.float32), np.arange(S["height"], dtype=np.float32))
    sf, rect = small_handles(corb, maps=False)
    for eye in range(2):
        rect.set_maps(eye, j + np.float32(3.25 + eye), i + np.float32(2.5))
    a = rect.frames(raw[:1])
    inside = np.stack([R.remap(raw[0, e], j + np.float32(3.25 + e), i + np.float32(2.5))[0] for e in range(2)])
    assert np.array_equal(planes(sf, 1)[0], inside) and (inside[:, :4, :4] != 0).any()
    for eye in range(2):
        rect.set_maps(eye, *G.small_maps(eye))
    b1 = rect.frames(raw[1:2]).copy(); p1 = planes(sf, 1)
    b2 = rect.frames(raw[1:2]).copy(); p2 = planes(sf, 1)
    sf2, rect2 = small_handles(corb)
    c = rect2.frames(raw[1:2]); pc = planes(sf2, 1)
    assert np.array_equal(p1, want[1:2]) and np.array_equal(p2, p1) and np.array_equal(pc, p1)
    assert written(sf, b1, 0) == written(sf, b2, 0) == written(sf2, c, 0) and written(sf, a, 0)[0] != written(sf, b1, 0)[0]
    rect2.close(); sf2.close(); rect.close(); sf.close()


def test_refusals(corb, small):
    raw, want = small
    sf, rect = small_handles(corb)
    rect.upload_batch(0, raw)
    L = corb.load()
    good = dict(left=(K_S, D_S, R_S, PL_S), right=(K_S, D_S, R_S, PR_S), raw_width=S["raw_width"], raw_height=S["raw_height"])

    def refused(msg=None, **kw):
        a = dict(good); a.update(kw)
        with pytest.raises(corb.CorbError) as e:
            corb.StereoRectifier(sf, a["left"], a["right"], a["raw_width"], a["raw_height"])
        assert "(%d)" % ERR_ARG in str(e.value) and (msg is None or msg in str(e.value)), str(e.value)
    Z9 = np.zeros(9); Z12 = np.zeros(12)
    refused("zero image size", raw_width=0); refused("zero image size", raw_height=0)                       # stereo_euroc.cc:88-93
    refused("missing", left=(Z9, D_S, R_S, PL_S)); refused("missing", right=(K_S, D_S, Z9, PR_S)); refused("missing", left=(K_S, D_S, R_S, Z12))
    refused("no inverse", left=(K_S, D_S, [1, 0, 0, 0, 1, 0, 1, 1, 0], PL_S))                             # det(P3x3 R) == 0
    refused("not finite", right=(K_S, [0, 0, 0, 0, 0, np.nan, 0, 0], R_S, PR_S))                          # a map entry that is not finite
    refused("2^26", left=(np.array(K_S) * 1e9, np.zeros(5), R_S, PL_S))                                   # |entry| >= 2^26
    refused("32767", raw_width=32768); refused("32767", raw_height=40000)
    j, i = np.meshgrid(np.arange(S["width"], dtype=np.float32), np.arange(S["height"], dtype=np.float32))
    for badv in (np.nan, np.inf, 2.0 ** 26):
        bx = j.copy(); bx[5, 7] = badv
        with pytest.raises(corb.CorbError) as e:
            rect.set_maps(0, bx, i)
        assert "(%d)" % ERR_ARG in str(e.value)
    res = np.zeros(3 * sf.frame_layout().frame_bytes, np.uint8)
    three = np.ascontiguousarray(np.concatenate([raw, raw[:1]]))
    assert L.corb_rect_frames(rect.h, 3, three.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p), None) == ERR_ARG          # n > max_frames
    assert L.corb_rect_frames(rect.h, 0, three.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p), None) == ERR_ARG
    assert L.corb_rect_frames(rect.h, 1, None, res.ctypes.data_as(C.c_void_p), None) == ERR_ARG and L.corb_rect_frames(rect.h, 1, three.ctypes.data_as(C.c_void_p), None, None) == ERR_ARG
    assert L.corb_rect_upload_batch(rect.h, 1, 2, three.ctypes.data_as(C.c_void_p)) == ERR_ARG and L.corb_rect_upload_batch(rect.h, 0, 1, None) == ERR_ARG
    assert not res.any()
    # nothing was launched or changed by any refusal: the eye kept its maps and the planes are those of the upload
    assert np.array_equal(rect.maps(0)[0].view(np.uint32), G.small_maps(0)[0].view(np.uint32)) and np.array_equal(planes(sf, 2), want)
    rect.close(); sf.close()

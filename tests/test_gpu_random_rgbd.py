"""GPU parity of the RGB-D / monocular front-end (corb_rgbd_*) at odd geometries and random calibrations, bit-exact against tests/cam_reference.py with the
oracle's extractor as tests/test_gpu_rgbd.py checks it: widths of every residue mod 4 (cam_ingest_kernel's 4-pixel groups end in a partial group and rows
start at odd byte offsets), depth planes at unaligned offsets, frame 1 of a packed batch at an unaligned offset, 1 / 3 / 4 channels in RGB and BGR order,
u16 and f32 depth, barrel and pincushion Brown calibrations with and without k3, the tangential-only k1 = 0 pass-through, depth factors 1, 2.5 and 5000."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cam_reference as R  # noqa: E402
from test_gpu_rgbd import _bits, _same  # noqa: E402

pytestmark = pytest.mark.gpu

# the extractor configurations tests/test_gpu_orb.py::test_other_configurations proves at these sizes, and widths of the other residues mod 4
ORB_CFG = {(129, 97): dict(nfeatures=300, scaleFactor=1.2, nlevels=3, iniThFAST=20, minThFAST=7),
           (403, 263): dict(nfeatures=800, scaleFactor=1.3, nlevels=5, iniThFAST=15, minThFAST=5),
           (1283, 381): dict(nfeatures=1500, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7),
           (322, 241): dict(nfeatures=500, scaleFactor=1.2, nlevels=4, iniThFAST=20, minThFAST=7),
           (640, 479): dict(nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7)}
SIZES = list(ORB_CFG)


def _calib(rng, kind, w, h):
    """a random Brown calibration of a w x h camera: barrel (k1 < 0), pincushion (k1 > 0), with k3 or without, or tangential terms only (k1 = 0)"""
    f = float(rng.uniform(0.75, 1.1) * w)
    cam = dict(fx=f, fy=float(f * rng.uniform(0.98, 1.02)), cx=float(w / 2 + rng.uniform(-8, 8)), cy=float(h / 2 + rng.uniform(-6, 6)),
               k1=0.0, k2=0.0, p1=float(rng.uniform(-0.004, 0.004)), p2=float(rng.uniform(-0.004, 0.004)), k3=0.0, bf=40.0, width=w, height=h)
    if kind != "tangential":
        cam["k1"] = float(rng.uniform(-0.3, -0.05) if kind.startswith("barrel") else rng.uniform(0.05, 0.3))
        cam["k2"] = float(rng.uniform(-0.2, 0.2))
    if kind.endswith("k3"):
        cam["k3"] = float(rng.uniform(-0.5, 0.5))
    return cam


def _case(i, size, kind, channels, rgb, depth, factor, sensor="rgbd"):
    rng = np.random.default_rng(47000 + i)
    w, h = size
    cam = _calib(rng, kind, w, h)
    cam["depth_map_factor"] = float(factor) if sensor == "rgbd" else 0.0
    if sensor == "mono":
        cam["bf"] = 0.0
    return dict(i=i, w=w, h=h, kind=kind, channels=channels, rgb=rgb, depth=depth if sensor == "rgbd" else "none", sensor=sensor, cam=cam, frame0=int(rng.integers(0, 1000)))


RGBD_CASES = [_case(0, (129, 97), "barrel", 3, 1, "u16", 5000.0),
              _case(1, (129, 97), "pincushion-k3", 1, 1, "f32", 1.0),
              _case(2, (403, 263), "barrel-k3", 4, 0, "u16", 2.5),
              _case(3, (403, 263), "tangential", 3, 0, "f32", 2.5),
              _case(4, (1283, 381), "pincushion", 4, 1, "f32", 5000.0),
              _case(5, (1283, 381), "barrel", 3, 1, "u16", 1.0),
              _case(6, (322, 241), "pincushion", 3, 1, "u16", 5000.0),
              _case(7, (322, 241), "barrel-k3", 4, 1, "u16", 1.0),
              _case(8, (640, 479), "tangential", 1, 1, "u16", 5000.0),
              _case(9, (640, 479), "barrel", 3, 0, "f32", 5000.0),
              _case(10, (403, 263), "barrel", 1, 1, None, None, sensor="mono"),
              _case(11, (1283, 381), "pincushion-k3", 3, 0, None, None, sensor="mono")]


def rgbd_case_id(c):
    return "rgbd-%03d-%dx%d-%s-c%d%s-%s%s" % (c["i"], c["w"], c["h"], c["kind"], c["channels"], "" if c["channels"] == 1 else ("-rgb" if c["rgb"] else "-bgr"),
                                             c["sensor"], "" if c["sensor"] == "mono" else "-%s-f%g" % (c["depth"], c["cam"]["depth_map_factor"]))


def rgbd_case_frames(synth, c):
    out = []
    for k in range(2):
        idx = c["frame0"] + k
        if c["sensor"] == "mono":
            out.append((synth.mono_frame(idx, w=c["w"], h=c["h"], channels=c["channels"]), None))
            continue
        col, d16 = synth.rgbd_frame(idx, w=c["w"], h=c["h"], channels=c["channels"])
        out.append((col, d16 if c["depth"] == "u16" else d16.astype(np.float32) * np.float32(0.0002)))
    return out


@pytest.mark.parametrize("c", RGBD_CASES, ids=[rgbd_case_id(c) for c in RGBD_CASES])
def test_rgbd_front_end_random_case(corb, synth, pyorc, c):
    cfg = ORB_CFG[(c["w"], c["h"])]
    cam = c["cam"]
    args = {k: cam[k] for k in R.CAM_KEYS}
    fe = corb.RgbdFrontend(width=c["w"], height=c["h"], max_frames=2, channels=c["channels"], rgb=c["rgb"],
                           sensor=corb.SENSOR_MONOCULAR if c["sensor"] == "mono" else corb.SENSOR_RGBD,
                           depth_format=corb.DEPTH_F32 if c["depth"] == "f32" else corb.DEPTH_U16, **cfg, **args)
    ex = pyorc.Extractor(cfg["nfeatures"], cfg["scaleFactor"], cfg["nlevels"], cfg["iniThFAST"], cfg["minThFAST"])
    fr = rgbd_case_frames(synth, c)
    refs = [R.frame(ex, col, dep, cam, c["rgb"]) for col, dep in fr]
    packed = fe.pack_input(fr)
    fe.upload_batch(0, packed); fe.run(2); fe.sync()
    for i in range(2):
        assert np.array_equal(fe.orb.pyramid_level(i, 0), refs[i]["grey"]), "level-0 plane of frame %d" % i
        _same(fe.fetch(i), refs[i], "batched frame %d" % i)
    res = fe.frames(packed)                                   # both frames in one call: frame 1's input starts at input_bytes, an odd offset here
    for i in range(2):
        one = fe.unpack_frame(res, i)
        assert one["status"] == 0
        _same(one, refs[i], "corb_rgbd_frames frame %d" % i)
    assert np.array_equal(_bits(fe.bounds()), _bits(R.image_bounds(cam)))
    if c["sensor"] == "mono":
        assert all((r["depth"] == -1).all() for r in refs)
    else:
        assert any((r["depth"] > 0).any() for r in refs)
    if cam["k1"] == 0:
        assert all(r["keys_un"].tobytes() == r["keys"].tobytes() for r in refs)
    fe.close()

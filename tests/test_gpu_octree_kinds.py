"""orb_octree_kernel by branch kind: every case of tests/octree_cases.py is classified on the CPU ORACLE's candidates (tests/octree_reference.py, pinned to
pyorc.distribute_octree by tests/test_octree_reference.py), a kind that no case holds fails the unmarked test, and the GPU's final keypoints -- which carry the
quadtree's result: which keys a level keeps, and in which order -- are compared with the oracle's as bytes, per level and as a whole, with the descriptors.

Launch shapes.  The kernel is instantiated with 512 threads per (image, level) for launches of up to 16 images and with 256 above that (unless the node tables
need more than 48 KiB of LDS: asserted below not to be so), and a level keeps its keys in registers up to 16 per thread.  So every case runs alone (512) and as a
run of 17 images (256); the uniform-noise case holds > 8192 candidates on level 0 (chunked at both widths) and 4097 .. 8192 on level 1 (chunked at 256, in
registers at 512), and also runs as 17 stereo frames: 34 images, which a run splits into two unequal part-batches.

ini_clamp is the one kind no image can hold: FAST leaves a 3-px ring inside the detection area, so a candidate's x is at most W - 4 and x / hX stays below nIni
(asserted per level by tests/test_octree_reference.py, which pins the clamp to the oracle on key sets of its own)."""
import numpy as np
import pytest

import octree_cases as OC
import octree_reference as OR

REG_KEYS = 16                      # keys per thread a level holds in registers
T_ALONE, T_RUN = 512, 256          # threads per (image, level): launches of <= 16 images / larger ones
WIDE_LDS = 48 * 1024
NEEDED = [k for k in OR.KIND_NAMES if k not in ("n", "nIni", "ini_clamp")]


def octree_lds_bytes(c):
    """LDS of the case's quadtree launch: 88 bytes per node of the largest node table (+ 4), a word per FAST cell (+ 1) and 256 bytes of scratch."""
    cap = ncell = 0
    for l, (w, h) in enumerate(c.sizes):
        W, H = w - 32, h - 32
        cap = max(cap, (max(int(c.quota[l]) + 3, 4 * c.kinds[l]["nIni"]) + 1 + 3) & ~3)
        ncell = max(ncell, int(np.float32(W) / np.float32(30)) * int(np.float32(H) / np.float32(30)))
    return (cap + 4) * 88 + (ncell + 1) * 4 + 256


def test_octree_kinds_present(pyorc):
    """CPU only: the table of kinds per case and level; every kind occurs; the empty and the single-key level lie between populated levels."""
    lines, total = OC.kinds_table(pyorc)
    print("\n" + "\n".join(lines))
    print("quadtree kinds over all cases:", {k: total[k] for k in OR.KIND_NAMES})
    for kd in NEEDED:
        assert total[kd] > 0, "no level of any case is of kind '%s'" % kd
    assert total["ini_clamp"] == 0
    for kd in ("empty", "single_key"):
        assert any(c.kinds[l][kd] and c.kinds[l - 1]["n"] > 1 and c.kinds[l + 1]["n"] > 1 for c in (OC.classified(pyorc, n) for n in OC.CASES) for l in range(1, c.nlevels - 1)), \
            "kind '%s' does not occur on a level between two populated levels" % kd
    assert any(c.kinds[0]["nIni"] == 1 for c in (OC.classified(pyorc, n) for n in OC.CASES)), "no case with a single initial node"
    w = OC.classified(pyorc, "wide_strip")
    assert w.kinds[0]["nIni"] >= 3 and w.kinds[0]["empty_ini"] > 0, "wide_strip: no empty initial node among >= 3"
    c = OC.classified(pyorc, "noise_403")
    n0, n1 = c.kinds[0]["n"], c.kinds[1]["n"]
    assert c.img.shape == (263, 403) and n0 > 8192 and 4097 <= n1 <= 8192, (n0, n1)
    assert n0 > REG_KEYS * T_ALONE and n0 > REG_KEYS * T_RUN                    # level 0: chunked at both widths
    assert REG_KEYS * T_RUN < n1 <= REG_KEYS * T_ALONE                         # level 1: chunked at 256 threads, in registers at 512
    for name in OC.CASES:
        assert octree_lds_bytes(OC.classified(pyorc, name)) <= WIDE_LDS, "%s: node tables this large take the 512-thread kernel at every launch size" % name


def _first_diff(g, r):
    for i in range(min(len(g), len(r))):
        if g[i].tobytes() != r[i].tobytes():
            return "first difference at index %d: got %s, want %s" % (i, g[i], r[i])
    return "the first %d agree" % min(len(g), len(r))


def compare(c, kps, desc, k, d, what):
    """GPU (k, d) against the oracle's (kps, desc) of case c: per level the count and the keypoints in order, then everything as bytes."""
    for l in range(c.nlevels):
        g, r = k[k["octave"] == l], kps[kps["octave"] == l]
        assert len(g) == len(r), "%s level %d: %d keypoints, the oracle has %d" % (what, l, len(g), len(r))
        assert g.tobytes() == r.tobytes(), "%s level %d (quota %d): %s" % (what, l, c.quota[l], _first_diff(g, r))
    assert k.tobytes() == kps.tobytes(), "%s: keypoints differ" % what
    assert np.array_equal(d, desc), "%s: descriptors differ, first at keypoint %d" % (what, int(np.nonzero((d != desc).any(1))[0][0]))


def mirror_reference(pyorc, c):
    ref = pyorc.Extractor(c.nfeatures, OC.SCALE, c.nlevels, OC.INI_TH, OC.MIN_TH)
    return ref.extract(np.ascontiguousarray(c.img[:, ::-1]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OC.CASES))
def test_alone_and_in_a_run_of_17(corb, pyorc, name):
    c = OC.classified(pyorc, name)
    assert [int((c.kps["octave"] == l).sum()) for l in range(c.nlevels)] == c.counts
    h, w = c.img.shape
    cfg = dict(nfeatures=c.nfeatures, scaleFactor=OC.SCALE, nlevels=c.nlevels, iniThFAST=OC.INI_TH, minThFAST=OC.MIN_TH, width=w, height=h)
    e = corb.ORBextractor(**cfg)
    try:
        k, d = e(c.img)
        compare(c, c.kps, c.desc, k, d, "%s alone" % name)
    finally:
        e.close()
    # 17 images in one launch: the case in slots 0 and 16, its horizontal mirror in between
    mir = np.ascontiguousarray(c.img[:, ::-1])
    mk, md = mirror_reference(pyorc, c)
    e = corb.ORBextractor(max_images=17, **cfg)
    try:
        for s in range(17):
            e.upload(s, c.img if s in (0, 16) else mir)
        e.run(17); e.sync()
        out = [e.fetch(s) for s in range(17)]
    finally:
        e.close()
    for s in (0, 16):
        compare(c, c.kps, c.desc, out[s][0], out[s][1], "%s in slot %d of 17" % (name, s))
    for s in range(2, 16):
        assert out[s][0].tobytes() == out[1][0].tobytes() and out[s][1].tobytes() == out[1][1].tobytes(), "%s: slots 1 and %d hold the same image and differ" % (name, s)
    compare(c, mk, md, out[1][0], out[1][1], "%s mirrored in slot 1 of 17" % name)


@pytest.mark.gpu
def test_noise_in_a_stereo_run_of_17_frames(corb, pyorc):
    """34 images in one run (two part-batches of unequal size): the noise case in the first and the last image of the run and on both sides of the middle."""
    c = OC.classified(pyorc, "noise_403")
    h, w = c.img.shape
    mir = np.ascontiguousarray(c.img[:, ::-1])
    mk, md = mirror_reference(pyorc, c)
    held = (0, 16, 17, 33)
    sf = corb.StereoFrontend(nfeatures=c.nfeatures, scaleFactor=OC.SCALE, nlevels=c.nlevels, iniThFAST=OC.INI_TH, minThFAST=OC.MIN_TH, width=w, height=h, max_frames=17)
    try:
        for f in range(17):
            sf.upload(f, c.img if 2 * f in held else mir, c.img if 2 * f + 1 in held else mir)
        sf.run(17); sf.sync()
        out = [sf.orb.fetch(i) for i in range(34)]
    finally:
        sf.close()
    for i in held:
        compare(c, c.kps, c.desc, out[i][0], out[i][1], "noise_403 as image %d of 34" % i)
    others = [i for i in range(34) if i not in held]
    for i in others[1:]:
        assert out[i][0].tobytes() == out[others[0]][0].tobytes() and out[i][1].tobytes() == out[others[0]][1].tobytes(), "images %d and %d hold the same image and differ" % (others[0], i)
    compare(c, mk, md, out[others[0]][0], out[others[0]][1], "noise_403 mirrored as image %d of 34" % others[0])

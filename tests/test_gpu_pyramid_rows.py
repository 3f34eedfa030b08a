"""orb_pyramid_kernel on random-byte images: every level of the pyramid against the CPU oracle, bit-exact (tolerance 0).

The kernel walks consecutive output rows and keeps the horizontal pass of the lower source row for the next output row whenever
ys0[y] == ys1[y - 1]; a noise image exposes any wrong row, tap or coefficient that a smooth synthetic scene can hide.  The cases drive
that decision through its branches (checked without a GPU by test_cases_reach_the_reuse_branches from the same row tables the library builds):
  * scale 1.05: nearly every row reuses; 1.2, 1.3, 1.5: a source step of 2 every few rows; 2.0: ys0 always steps by 2, nothing is reused, and it
    is the last scale of the 12-byte (`wide`) path; 2.5: the byte-gather path for scales above 2;
  * widths that are no multiple of 4 (partial last group) on every case but one, tiles of 16 .. 67 column groups (one and several row runs per
    wavefront, chunk boundaries), the workload's 1241 x 376 geometry, and a batch of three different images in one run.
Sizes the issue names that corb_orb_create refuses, and what stands in for them:
  * 160 x 120 with 8 levels and any image whose top level is below 16 rows (the per-level fallback kernel): create refuses every level below 62 x 62
    (no 30-px FAST cell fits), so the fallback kernel is reachable with no accepted size.  Nearest accepted: 160 x 120 with 4 levels (top level
    93 x 69: wavefront row quarters of 4 .. 5 rows, runs of 1 .. 3 rows) and 300 x 224 with 8 levels (top level 84 x 63, the smallest 8-level pyramid).
  * a last output row whose ys1 is clamped onto ys0: cv::resize's tables never produce it when shrinking by less than 3 (the last row's upper source
    row is sh - 2); test_cases_reach_the_reuse_branches asserts that, so the kernel's handling of it stays covered by construction (it recomputes)."""
import numpy as np
import pytest

#        name              w     h   scale levels
CASES = [("s105",          403, 263, 1.05, 8),
         ("kitti_s12",    1241, 376, 1.2,  8),
         ("s13_odd",       403, 263, 1.3,  5),
         ("s15_odd",       321, 243, 1.5,  4),
         ("s20_wide_edge", 642, 480, 2.0,  3),
         ("s25_gather",    641, 479, 2.5,  3),
         ("small_4lv",     160, 120, 1.2,  4),
         ("small_8lv",     300, 224, 1.2,  8),
         ("odd_s12",      1283, 381, 1.2,  8)]
IDS = [c[0] for c in CASES]


def _image(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _rows(sh, dh):
    """ys0, ys1 of cv::resize INTER_LINEAR (the row part of build_resize_tables in corb_orb.cpp)"""
    dy = np.arange(dh, dtype=np.float64)
    fy = ((dy + 0.5) * (1.0 / (dh / sh)) - 0.5).astype(np.float32)
    sy = np.floor(fy).astype(np.int64)
    return np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)


_REF = {}


def _oracle_levels(pyorc, name):
    """every level of the case's image from the oracle alone, computed once and shared"""
    if name not in _REF:
        _, w, h, scale, nl = CASES[IDS.index(name)]
        ref = pyorc.Extractor(500, scale, nl, 20, 7)
        ref.extract(_image(1000 + IDS.index(name), w, h))
        lv = [np.array(ref.level(l), copy=True) for l in range(nl)]
        for a in lv: a.setflags(write=False)
        _REF[name] = lv
    return _REF[name]


@pytest.mark.parametrize("name", IDS)
def test_cases_reach_the_reuse_branches(pyorc, name):
    _, w, h, scale, nl = CASES[IDS.index(name)]
    lv = _oracle_levels(pyorc, name)
    assert len(lv) == nl and lv[0].shape == (h, w)
    reuse = step2 = clamp = rows = 0
    for l in range(1, nl):
        assert lv[l] is not None and min(lv[l].shape) >= 62, "corb_orb_create refuses levels below 62 x 62"
        ys0, ys1 = _rows(lv[l - 1].shape[0], lv[l].shape[0])
        reuse += int(np.sum(ys0[1:] == ys1[:-1])); step2 += int(np.sum(ys0[1:] > ys1[:-1])); clamp += int(np.sum(ys1 == ys0)); rows += len(ys0) - 1
    assert clamp == 0                                      # see the module docstring
    if scale == 1.05: assert reuse > 0.9 * rows and step2 > 0
    elif scale < 2.0: assert reuse > 0.4 * rows and step2 > 0.1 * rows
    else: assert reuse == 0 and step2 == rows
    if name != "s20_wide_edge": assert any(a.shape[1] % 4 for a in lv[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_every_level_bit_exact_on_noise(corb, pyorc, name):
    _, w, h, scale, nl = CASES[IDS.index(name)]
    lv = _oracle_levels(pyorc, name)
    e = corb.ORBextractor(nfeatures=500, scaleFactor=scale, nlevels=nl, iniThFAST=20, minThFAST=7, width=w, height=h)
    try:
        e(_image(1000 + IDS.index(name), w, h))
        for l in range(nl):
            g = e.pyramid_level(0, l)
            assert g.shape == lv[l].shape, "level %d shape" % l
            bad = np.argwhere(g != lv[l])
            assert len(bad) == 0, "level %d: %d bytes differ, first at (y, x) = %s" % (l, len(bad), tuple(bad[0]))
    finally:
        e.close()


@pytest.mark.gpu
def test_batch_of_three_images_in_one_run(corb, pyorc):
    """three different noise images through one launch: anything carried in registers or scalars from one image or run to the next would show"""
    w, h, scale, nl = 403, 263, 1.2, 6
    imgs = [_image(2000 + i, w, h) for i in range(3)]
    refs = []
    for im in imgs:
        ref = pyorc.Extractor(500, scale, nl, 20, 7); ref.extract(im)
        refs.append([np.array(ref.level(l), copy=True) for l in range(nl)])
    e = corb.ORBextractor(nfeatures=500, scaleFactor=scale, nlevels=nl, iniThFAST=20, minThFAST=7, width=w, height=h, max_images=3)
    try:
        for rep in range(2):                               # the second run writes over the first one's planes in another slot order
            for i in range(3): e.upload((i + rep) % 3, imgs[i])
            e.run(3); e.sync()
            for i in range(3):
                for l in range(nl):
                    assert np.array_equal(e.pyramid_level((i + rep) % 3, l), refs[i][l]), "run %d image %d level %d" % (rep, i, l)
    finally:
        e.close()

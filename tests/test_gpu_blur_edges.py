"""orb_blur_kernel at its edges: the blurred plane of EVERY level (the GPU blurs all of them; the oracle's extractor only those with keypoints, so the
reference here is pyorc.gaussian_blur7 on the oracle's level) byte for byte, on uniform byte noise, where a wrong reflected column or row, a wrong
partial store or a missing saturation changes bytes instead of landing on flat grey.

The kernel gives a lane a 4-px column group of a 32-row strip, 64 (strip, group) items per wave in row-major order, rows in chunks of 8, output
rows in pairs; a wave whose live lanes all hold their 12 bytes inside the row takes the path without column reflection.  The kinds below are the
sizes at which that goes different ways.  They are counted from the oracle's level sizes and planes (never from GPU output) by the unmarked test,
and a kind that no case holds fails it; the parity tests carry the gpu marker.

Saturation: the 8-bit taps {18,34,49,55,49,34,18} sum to 257 per axis, so a window of 255s gives (257*257*255 + 2^15) >> 16 = 257 and one of 254s
gives 256: only the final saturation brings these back to 255.  `presat` restates the two integer passes in numpy; it is first checked against
pyorc.gaussian_blur7 on every plane, then used to count the pixels above 255."""
import numpy as np
import pytest

TAPS = np.array([18, 34, 49, 55, 49, 34, 18], np.int64)
B = 12                                                    # side of a pasted block (>= 9: a 7 x 7 window fits with room to spare)
# name: (width, height, levels, seed); scale 1.2, every level >= 62 px per axis
CASES = {
    "wide_403x263": (403, 263, 2, 11),
    "pitch_320x96": (320, 96, 3, 12),
    "low_130x76": (130, 76, 2, 13),
    "odd_257x103": (257, 103, 3, 14),
    "narrow_98x161": (98, 161, 2, 15),
}
BLOCK_BASE = "wide_403x263"
KINDS = ("w_mod4_0", "w_mod4_1", "w_mod4_2", "w_mod4_3", "pitch_eq_width", "groups_le_64", "wave_interior", "wave_straddle",
         "h_last_1_7", "h_last_9_31", "h_mult_32", "h_odd", "h_lt_70")


def noise(name):
    w, h, _, seed = CASES[name]
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def block_boxes(w, h):
    """(x0, y0) of the three pasted blocks: touching the left border, touching the bottom border, interior."""
    return {"left": (0, 40), "bottom": (100, h - B), "interior": (150, 20)}


def block_image():
    img = noise(BLOCK_BASE).copy()
    h, w = img.shape
    bx = block_boxes(w, h)
    img[bx["left"][1]:bx["left"][1] + B, 0:B] = 255
    img[h - B:h, bx["bottom"][0]:bx["bottom"][0] + B] = 254
    x, y = bx["interior"]
    img[y:y + B, x:x + B] = np.random.default_rng(99).choice(np.array([254, 255], np.uint8), (B, B))
    return img


def images():
    """name -> (image, levels); the block case and a second noise image share the geometry of BLOCK_BASE (the three run as one batch)."""
    out = {n: (noise(n), CASES[n][2]) for n in CASES}
    w, h, nl, _ = CASES[BLOCK_BASE]
    out["blocks"] = (block_image(), nl)
    out["wide_second"] = (np.random.default_rng(21).integers(0, 256, (h, w), dtype=np.uint8), nl)
    return out


def presat(a):
    """The two integer passes of the 7 x 7 blur (BORDER_REFLECT_101) up to (sum + 2^15) >> 16, BEFORE saturation."""
    h, w = a.shape
    p = np.pad(a.astype(np.int64), 3, mode="reflect")
    hs = sum(TAPS[k] * p[:, k:k + w] for k in range(7))
    vs = sum(TAPS[k] * hs[k:k + h] for k in range(7))
    return (vs + (1 << 15)) >> 16


def size_kinds(w, h):
    """Kinds of one level from its size alone (64 items per wave, items = (strip, group) row-major)."""
    groups, strips = (w + 3) // 4, (h + 31) // 32
    k = dict.fromkeys(KINDS, 0)
    k["w_mod4_%d" % (w % 4)] = 1
    k["pitch_eq_width"] = int(w % 64 == 0)
    k["groups_le_64"] = int(groups <= 64)
    items = groups * strips
    for w0 in range(0, items, 64):
        it = np.arange(w0, min(w0 + 64, items))
        xg, st = it % groups, it // groups
        if np.all((4 * xg >= 4) & (4 * xg + 8 <= w)):
            k["wave_interior"] += 1
        if st.min() != st.max():
            k["wave_straddle"] += 1
    assert (k["wave_straddle"] > 0) <= (groups % 64 != 0)
    k["h_last_1_7"] = int(1 <= h % 32 <= 7)
    k["h_last_9_31"] = int(9 <= h % 32 <= 31)
    k["h_mult_32"] = int(h % 32 == 0)
    k["h_odd"] = h & 1
    k["h_lt_70"] = int(h < 70)
    return k


def oracle_levels(pyorc, img, nlevels):
    ref = pyorc.Extractor(500, 1.2, nlevels, 20, 7)
    ref.extract(img)
    return [ref.level(l) for l in range(nlevels)]


_cache = {}


def reference(pyorc, name):
    """(image, oracle levels, pyorc.gaussian_blur7 of each) of a case, computed once per session."""
    if name not in _cache:
        img, nl = images()[name]
        lv = oracle_levels(pyorc, img, nl)
        _cache[name] = (img, lv, [pyorc.gaussian_blur7(a) for a in lv])
    return _cache[name]


def test_blur_kinds_present(pyorc):
    """CPU only: the numpy restatement equals the oracle's blur on every plane; every kind occurs on some level of some case."""
    tot = dict.fromkeys(KINDS, 0)
    over = {}
    print()
    for name in images():
        img, lv, bl = reference(pyorc, name)
        for l, (a, b) in enumerate(zip(lv, bl)):
            assert min(a.shape) >= 62, (name, l, a.shape)
            ps = presat(a)
            assert ps.min() >= 0 and np.array_equal(np.minimum(ps, 255).astype(np.uint8), b), "the numpy restatement of the blur disagrees with the oracle: %s level %d" % (name, l)
            k = size_kinds(a.shape[1], a.shape[0])
            n_over = int((ps > 255).sum())
            assert ps.max() <= 257
            over[name] = over.get(name, 0) + n_over
            print("%-16s level %d %4d x %-4d groups %3d strips %2d presat_over_255 %4d  %s" % (name, l, a.shape[1], a.shape[0], (a.shape[1] + 3) // 4, (a.shape[0] + 31) // 32,
                                                                                           n_over, " ".join(kd for kd in KINDS if k[kd])))
            for kd in KINDS:
                tot[kd] += k[kd]
    print("blur kinds over all cases:", tot)
    for kd in KINDS:
        assert tot[kd] > 0, "no level of any case is of kind '%s'" % kd
    # saturation: the block case as a whole, and each of its three blocks on level 0 (where the blocks are exact)
    img, lv, _ = reference(pyorc, "blocks")
    assert over["blocks"] > 0, "kind 'presat_over_255': the block case holds no pixel that exceeds 255 before saturation"
    ps = presat(lv[0])
    h, w = img.shape
    for pos, (x, y) in block_boxes(w, h).items():
        n = int((ps[y:y + B, x:x + B] > 255).sum())
        print("presat_over_255 in the %s block: %d (values %s)" % (pos, n, sorted(set(ps[y:y + B, x:x + B][ps[y:y + B, x:x + B] > 255].tolist()))))
        assert n > 0, "kind 'presat_over_255': none in the %s block of the block case" % pos
    assert int((presat(reference(pyorc, BLOCK_BASE)[1][0]) > 255).sum()) == 0          # the noise under the blocks never gets there by itself


def first_diff(got, want):
    ys, xs = np.nonzero(got != want)
    return "%d bytes differ, first at x = %d, y = %d: got %d, want %d" % (len(ys), xs[0], ys[0], got[ys[0], xs[0]], want[ys[0], xs[0]])


def check_slot(e, slot, levels, blurred, what):
    for l, (a, b) in enumerate(zip(levels, blurred)):
        assert np.array_equal(e.pyramid_level(slot, l), a), "%s: pyramid level %d" % (what, l)
        g = e.pyramid_level(slot, l, True)
        assert g.shape == b.shape and np.array_equal(g, b), "%s: blurred level %d (%d x %d): %s" % (what, l, b.shape[1], b.shape[0], first_diff(g, b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES) + ["blocks"])
def test_blurred_levels_bit_exact(corb, pyorc, name):
    img, lv, bl = reference(pyorc, name)
    e = corb.ORBextractor(nfeatures=500, scaleFactor=1.2, nlevels=len(lv), iniThFAST=20, minThFAST=7, width=img.shape[1], height=img.shape[0])
    try:
        e(img)
        check_slot(e, 0, lv, bl, name)
    finally:
        e.close()


@pytest.mark.gpu
def test_three_images_in_one_run(corb, pyorc):
    """Three different images of one geometry in one launch (noise, the block case, other noise): each slot against its own reference."""
    names = [BLOCK_BASE, "blocks", "wide_second"]
    refs = [reference(pyorc, n) for n in names]
    h, w = refs[0][0].shape
    e = corb.ORBextractor(nfeatures=500, scaleFactor=1.2, nlevels=len(refs[0][1]), iniThFAST=20, minThFAST=7, width=w, height=h, max_images=3)
    try:
        for s, r in enumerate(refs):
            e.upload(s, r[0])
        e.run(3); e.sync()
        for s, (n, r) in enumerate(zip(names, refs)):
            check_slot(e, s, r[1], r[2], "%s in slot %d" % (n, s))
    finally:
        e.close()

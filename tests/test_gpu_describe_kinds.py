"""orb_describe_kernel by kind: orientation (intensity centroid -> cv::fastAtan2 -> sincosf), the steered BRIEF gather and the output assembly, on images that
hold the exact edge cases uniform noise practically never produces.  Every kind is counted on the ORACLE's keypoints, levels and primitives by the unmarked test
(a kind that no case holds fails it); the parity tests carry the gpu marker and compare final keypoints (the angle as a bit pattern) and descriptors as bytes.

Hand-built cases: flat 128 with isolated 255 pixels (`stamp` with a flat ring: a FAST corner whose patch is symmetric, m10 == m01 == 0) and, next to some, one
"marker" pixel 6 grey levels up -- below the second FAST threshold, so no corner of its own -- which sets the two moments exactly: marker at (u, v) gives
m10 = 6 u, m01 = 6 v.  Features are 32 px apart or more.  Dots on the first and last legal column and row (EDGE_THRESHOLD 19: x = 19, w - 20, y = 19, h - 20) of a
level whose pitch equals its width (256 px).  Noise cases (noise in column bands that reach every border, few enough candidates that all survive) add arbitrary
moments, every x alignment and patch reach 18.  nfeatures is large enough that the quadtree keeps every candidate (asserted), so the level counts are the
candidate counts: counts of 1, 2 and 3, every count mod 4, and a 3-level case whose middle level is empty.

The kernel's restated parts (numpy): the moments over the umax circle (checked: pyorc.fast_atan2 of them is the oracle keypoint's angle, bit for bit), the
quadrant of pyorc.sincosf's reduction, and the rotated, rounded pattern coordinates from oracle/brief_pattern.h (checked: they reproduce the oracle's descriptor
of every keypoint from ref.blurred)."""
import os
import re
import numpy as np
import pytest

import octree_cases as OC
from test_gpu_fast_sides import stamp, cells_of

INI_TH, MIN_TH = 20, 7
FACTOR_PI = np.float32(np.pi / 180.0)
TWO_OVER_PI = 0.63661977236758134308
W2, H2 = 256, 130                     # the 2-level geometry: level 0 has pitch == width
MARK = 6                              # a marker's contrast: below MIN_TH


def pattern():
    """oracle/brief_pattern.h as int array [256][4] = (x0, y0, x1, y1)."""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "brief_pattern.h")).read()
    body = text[text.index("{") + 1:text.index("}")]
    v = np.array([int(t) for t in re.findall(r"-?\d+", body)], np.int64)
    assert v.size == 1024 and np.abs(v).max() == 13
    return v.reshape(256, 4)


def feature(img, x, y, marker=None):
    stamp(img, x, y, 255, [128] * 16)
    if marker is not None:
        img[y + marker[1], x + marker[0]] = 128 + MARK


def flat():
    return np.full((H2, W2), 128, np.uint8)


# markers (u, v): zero moments, the diagonal tie in all four quadrants, and both majorities in every open quadrant
MARKERS = [None, (5, 0), (-5, 0), (0, 5), (0, -5), (5, 5), (-5, 5), (-5, -5), (5, -5),
           (7, 3), (-7, 3), (-7, -3), (7, -3), (3, 7), (-3, 7), (-3, -7), (3, -7)]


def img_moments():
    img = flat()
    for i, mk in enumerate(MARKERS):                       # 17 features on a 6 x 3 grid, 36 px apart
        feature(img, 30 + 36 * (i % 6), 30 + 36 * (i // 6), mk)
    return img


def img_extremes():
    """Dots on the four extreme legal positions of level 0 (the corners of the detection area) and on each side's middle: 8 features."""
    img = flat()
    for x in (19, 128, W2 - 20):
        for y in (19, 64, H2 - 20):
            if (x, y) != (128, 64):
                feature(img, x, y, (4, -4) if x == 19 else None)
    return img


def img_dots(n):
    img = flat()
    for i in range(n):
        feature(img, 60 + 64 * i, 40 + 20 * i, [(6, 2), None, (-2, 6)][i])
    return img


def img_noise_bands(w, h, seed, bands):
    img = np.full((h, w), 128, np.uint8)
    rng = np.random.default_rng(seed)
    for x0, x1 in bands:
        img[:, x0:x1] = rng.integers(0, 256, (h, x1 - x0), dtype=np.uint8)
    return img


def img_noise3():
    return img_noise_bands(200, 130, 33, [(0, 60), (150, 200)])


# name: (builder, nfeatures, levels).  Same geometry and configuration = one handle: those cases also run three to a launch (TRIPLES)
CASES = {
    "moments": (img_moments, 3000, 2),
    "extremes": (img_extremes, 3000, 2),
    "one": (lambda: img_dots(1), 3000, 2),
    "two": (lambda: img_dots(2), 3000, 2),
    "three": (lambda: img_dots(3), 3000, 2),
    "noise_a": (lambda: img_noise_bands(W2, H2, 31, [(0, 70), (210, W2)]), 3000, 2),
    "noise_b": (lambda: img_noise_bands(W2, H2, 32, [(0, 40), (100, 150), (226, W2)]), 3000, 2),
    "gap3": (OC.sparse_gap, 2000, 3),
    "single3": (OC.sparse_one, 2000, 3),
    "noise3": (img_noise3, 2000, 3),
}
TRIPLES = [("moments", "one", "noise_a"), ("extremes", "two", "noise_b"), ("three", "noise_a", "moments"), ("gap3", "single3", "noise3")]
MOMENT_KINDS = ["both_zero", "m01_zero_pos", "m01_zero_neg", "m10_zero_pos", "m10_zero_neg"] + ["diag_tie_q%d" % q for q in (1, 2, 3, 4)] + \
               ["xmaj_q%d" % q for q in (1, 2, 3, 4)] + ["ymaj_q%d" % q for q in (1, 2, 3, 4)]
KINDS = MOMENT_KINDS + ["sincos_q%d" % q for q in range(5)] + ["x_19", "x_w20", "y_19", "y_h20", "x_extreme_pitch_eq_width"] + ["xalign_%d" % r for r in range(4)] + \
        ["count_mod4_%d" % r for r in range(4)] + ["count_1", "count_2", "count_3", "empty_between", "reach_row_18", "reach_col_18"]


def moments(I, cx, cy, umax):
    m10 = m01 = 0
    for v in range(-15, 16):
        d = int(umax[abs(v)])
        row = I[cy + v, cx - d:cx + d + 1].astype(np.int64)
        m10 += int((np.arange(-d, d + 1) * row).sum())
        m01 += v * int(row.sum())
    return m10, m01


def moment_kind(m10, m01):
    if m10 == 0 and m01 == 0:
        return "both_zero"
    if m01 == 0:
        return "m01_zero_pos" if m10 > 0 else "m01_zero_neg"
    if m10 == 0:
        return "m10_zero_pos" if m01 > 0 else "m10_zero_neg"
    q = (1 if m01 > 0 else 4) if m10 > 0 else (2 if m01 > 0 else 3)                # image quadrants in the order of the angle: 0-90, 90-180, 180-270, 270-360
    return ("diag_tie_q%d" if abs(m10) == abs(m01) else "xmaj_q%d" if abs(m10) > abs(m01) else "ymaj_q%d") % q


def steered(pyorc, pat, angle_deg):
    """(row, col) [256][2] of the rotated pattern: float32, one operation at a time, rounded half to even -- and the quadrant of the sincosf reduction."""
    rad = np.float32(angle_deg) * FACTOR_PI
    s, c = pyorc.sincosf(rad)
    a, b = np.float32(c), np.float32(s)
    X, Y = pat[:, [0, 2]].astype(np.float32), pat[:, [1, 3]].astype(np.float32)
    row = np.rint(X * b + Y * a).astype(np.int64)
    col = np.rint(X * a - Y * b).astype(np.int64)
    return row, col, int(np.rint(np.float64(rad) * TWO_OVER_PI))


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


class Classified:
    def __init__(self, pyorc, name):
        build, self.nfeatures, self.nlevels = CASES[name]
        self.name, self.img = name, build()
        ref = pyorc.Extractor(self.nfeatures, 1.2, self.nlevels, INI_TH, MIN_TH)
        self.kps, self.desc = ref.extract(self.img)
        tb = ref.tables()
        pat = pattern()
        k = self.kinds = dict.fromkeys(KINDS, 0)
        self.counts = [ref.level_count(l) for l in range(self.nlevels)]
        self.moments = [set() for _ in range(self.nlevels)]                  # (m10, m01) of the level's keypoints
        off = 0
        for l in range(self.nlevels):
            I, cd, n = ref.level(l), ref.candidates(l), self.counts[l]
            h, w = I.shape
            assert n == len(cd), "%s level %d: the quadtree dropped candidates (%d of %d kept): nfeatures is too small for this case" % (name, l, n, len(cd))
            k["count_mod4_%d" % (n % 4)] += 1
            if 1 <= n <= 3:
                k["count_%d" % n] += 1
            if n == 0 and 0 < l < self.nlevels - 1 and self.counts[l - 1] > 0 and ref.level_count(l + 1) > 0:
                k["empty_between"] += 1
            if n == 0:
                continue
            B = ref.blurred(l)
            # level coordinates of the final keypoints: every candidate is kept, so each keypoint is the one candidate with its (scaled) position
            cx, cy = cd["x"].astype(np.int64) + 16, cd["y"].astype(np.int64) + 16
            sx, sy = (cx.astype(np.float32), cy.astype(np.float32)) if l == 0 else (cx.astype(np.float32) * tb["scale"][l], cy.astype(np.float32) * tb["scale"][l])
            where = {(float(a), float(b)): i for i, (a, b) in enumerate(zip(sx, sy))}
            assert len(where) == len(cd)
            for j in range(off, off + n):
                kp = self.kps[j]
                assert kp["octave"] == l
                i = where[(float(kp["x"]), float(kp["y"]))]
                x, y = int(cx[i]), int(cy[i])
                assert 19 <= x <= w - 20 and 19 <= y <= h - 20
                m10, m01 = moments(I, x, y, tb["umax"])
                assert bits(pyorc.fast_atan2(m01, m10)) == bits(kp["angle"]) == bits(pyorc.ic_angle(I, x, y)), "%s level %d (%d, %d): the numpy moments disagree with the oracle's angle" % (name, l, x, y)
                k[moment_kind(m10, m01)] += 1
                self.moments[l].add((m10, m01))
                row, col, q = steered(pyorc, pat, kp["angle"])
                assert 0 <= q <= 4 and np.abs(row).max() <= 18 and np.abs(col).max() <= 18
                t = B[y + row, x + col]
                d = np.packbits((t[:, 0] < t[:, 1]).reshape(32, 8), axis=1, bitorder="little").reshape(32)
                assert np.array_equal(d, self.desc[j]), "%s level %d (%d, %d): the numpy steering disagrees with the oracle's descriptor" % (name, l, x, y)
                k["sincos_q%d" % q] += 1
                k["reach_row_18"] += int(np.abs(row).max() == 18); k["reach_col_18"] += int(np.abs(col).max() == 18)
                k["x_19"] += int(x == 19); k["x_w20"] += int(x == w - 20); k["y_19"] += int(y == 19); k["y_h20"] += int(y == h - 20)
                k["x_extreme_pitch_eq_width"] += int(w % 64 == 0 and x in (19, w - 20))
                k["xalign_%d" % ((x - 18) % 4)] += 1
            off += n
        assert off == len(self.kps)


_cache = {}


def classified(pyorc, name):
    if name not in _cache:
        _cache[name] = Classified(pyorc, name)
    return _cache[name]


def test_describe_kinds_present(pyorc):
    """CPU only: the restatements equal the oracle on every keypoint of every case (asserted while classifying); every kind occurs."""
    cells, _, _ = cells_of(W2, H2)
    assert cells[0][0] + 3 == 19 and cells[-1][0] + cells[-1][2] - 4 == W2 - 20 and cells[0][1] + 3 == 19 and cells[-1][1] + cells[-1][3] - 4 == H2 - 20    # the FAST grid's first and last pixels
    total = dict.fromkeys(KINDS, 0)
    print()
    for name in CASES:
        c = classified(pyorc, name)
        print("%-9s counts %-14s %s" % (name, c.counts, " ".join("%s=%d" % (kd, c.kinds[kd]) for kd in KINDS if c.kinds[kd])))
        for kd in KINDS:
            total[kd] += c.kinds[kd]
    print("describe kinds over all cases:", total)
    for kd in KINDS:
        assert total[kd] > 0, "no keypoint or level of any case is of kind '%s'" % kd
    # the hand-built moments are what the markers say (level 0 of `moments`)
    c = classified(pyorc, "moments")
    assert c.counts[0] == len(MARKERS) and c.moments[0] == {(MARK * m[0], MARK * m[1]) if m else (0, 0) for m in MARKERS}
    for name, n in (("one", 1), ("two", 2), ("three", 3)):
        assert classified(pyorc, name).counts[0] == n, name
    assert classified(pyorc, "gap3").counts[1] == 0 and classified(pyorc, "single3").counts[1] == 1
    for t in TRIPLES:
        assert len({(classified(pyorc, n).img.shape, CASES[n][1:]) for n in t}) == 1 and len({tuple(classified(pyorc, n).counts) for n in t}) == 3, t
    assert {n for t in TRIPLES for n in t} == set(CASES)


def compare(c, k, d, what):
    assert len(k) == len(c.kps), "%s: %d keypoints, the oracle has %d" % (what, len(k), len(c.kps))
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        assert np.array_equal(k[f], c.kps[f]), "%s: keypoint field %s differs, first at %d" % (what, f, int(np.nonzero(k[f] != c.kps[f])[0][0]))
    bad = np.nonzero(bits(k["angle"]) != bits(c.kps["angle"]))[0]
    assert len(bad) == 0, "%s: %d angles differ, first at keypoint %d (level %d, x %g, y %g): got %r, want %r" % (
        what, len(bad), bad[0], k["octave"][bad[0]], k["x"][bad[0]], k["y"][bad[0]], float(k["angle"][bad[0]]), float(c.kps["angle"][bad[0]]))
    assert k.tobytes() == c.kps.tobytes(), "%s: keypoints differ" % what
    bad = np.nonzero((d != c.desc).any(1))[0]
    assert len(bad) == 0, "%s: %d descriptors differ, first at keypoint %d (level %d, x %g, y %g, angle %r)" % (
        what, len(bad), bad[0], k["octave"][bad[0]], k["x"][bad[0]], k["y"][bad[0]], float(k["angle"][bad[0]]))


def _cfg(c, **kw):
    return dict(nfeatures=c.nfeatures, scaleFactor=1.2, nlevels=c.nlevels, iniThFAST=INI_TH, minThFAST=MIN_TH, width=c.img.shape[1], height=c.img.shape[0], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_keypoints_and_descriptors_bit_exact(corb, pyorc, name):
    c = classified(pyorc, name)
    e = corb.ORBextractor(**_cfg(c))
    try:
        k, d = e(c.img)
        compare(c, k, d, name)
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("names", TRIPLES, ids=["+".join(t) for t in TRIPLES])
def test_three_cases_in_one_run(corb, pyorc, names):
    """Three images with different per-level counts in one launch: the group-to-level look-up and the output offsets are per image."""
    cs = [classified(pyorc, n) for n in names]
    e = corb.ORBextractor(**_cfg(cs[0], max_images=3))
    try:
        for s, c in enumerate(cs):
            e.upload(s, c.img)
        e.run(3); e.sync()
        for s, c in enumerate(cs):
            k, d = e.fetch(s)
            compare(c, k, d, "%s in slot %d of (%s)" % (c.name, s, ", ".join(names)))
    finally:
        e.close()

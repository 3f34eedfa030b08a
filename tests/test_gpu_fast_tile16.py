"""orb_fast_kernel's 16-bit pixel-pair tile (pytest -m gpu): pyramid levels, FAST candidates (x, y, response per level), final keypoints and
descriptors byte for byte against the CPU oracle, on small noise images whose geometry aims at what the tile can get wrong.

The kernel keeps a cell in LDS as one 16-bit slot per pixel (pixel in the low byte, its score in the high byte), so that an aligned dword is a
pixel pair; ring values at an odd dx are a byte permute of two adjacent dwords, the window of the last 4-pixel group of a row reaches past the cell into padding slots, and the tile write
spreads re-aligned global dwords to slots for every alignment (iniX - 1) & 3.  Geometries (scale 1.2, 2 levels):

  154 x 74   level 0: four cells of wCell 31 at iniX - 1 = 15, 46, 77, 108 = 3, 2, 1, 0 (mod 4): every write alignment in one image; interiors
             31, 31, 31 and 23 columns (last groups of 3 pixels), level 1 (128 px) wCell 32                              orb_fast_kernel<40>
  156 x 74   the same level 0 with a last interior of 25 columns (1 pixel); level 1 (130 px) has wCell 33, interiors 33 and 26
             (1 and 2 pixels), which takes the handle to the next pitch                                                   orb_fast_kernel<48>
  112 x 74   cells of 40 and 31 interior columns                                                                          orb_fast_kernel<48>
  90 x 90    one cell 58 wide, interior 52 x 52                                                                           orb_fast_kernel<80>

Noise of {0, 64, 128, 192, 255} and {0, 255} lists most pixel pairs and puts values of 0 and 255 next to the masked halves of partial groups.  On
the 154- and 156-px images cell 0 is {0, 255} noise throughout (more listed pairs than one batch of the pair list takes: the tile is read again after
scores were written into it, and the NMS runs over groups instead of over the list) and cell 2 stays within 18 grey levels (no corner at 20: the second threshold, a second pass over the same tile).  Every kind
is counted on the ORACLE's own candidates, and a kind without a case fails the test."""
import numpy as np
import pytest

from test_gpu_fast_sides import INI_TH, MIN_TH, LIST_CAP, SWEEP, cells_of, score_maps

pytestmark = pytest.mark.gpu

GEOMETRIES = [(154, 74, 40), (156, 74, 48), (112, 74, 48), (90, 90, 80)]          # width, height, tile pitch
EDGE_KINDS = ("col0", "col1", "col2", "lastcols", "row_first", "row_last")


def build_image(w, h, seed):
    rng = np.random.default_rng(seed)
    five, two = np.array([0, 64, 128, 192, 255], np.uint8), np.array([0, 255], np.uint8)
    img = rng.choice(five, (h, w))
    img[h // 2:] = rng.choice(two, (h - h // 2, w))
    cells, wcell, _ = cells_of(w, h)
    if len(cells) == 4:
        x_of = lambda j: 16 + 3 + j * wcell                     # first interior column of cell j
        img[:, :x_of(1)] = rng.choice(two, (h, x_of(1)))        # cell 0 and its left ring: saturated noise in every row
        img[:, x_of(2) - 3:x_of(3) + 3] = rng.choice(np.array([119, 128, 137], np.uint8), (h, x_of(3) + 6 - x_of(2)))   # cell 2 with both rings: contrast 18
    return img


def classify(pyorc, img, nlevels=2):
    """Counts on the oracle's levels and candidates; returns (kinds, last-group kinds, extractor, keypoints, descriptors, candidates per level)."""
    ref = pyorc.Extractor(500, 1.2, nlevels, INI_TH, MIN_TH)
    rk, rd = ref.extract(img)
    kinds = dict.fromkeys(EDGE_KINDS + ("second_pass", "wrap"), 0)
    last = {1: 0, 2: 0, 3: 0}                                   # candidates in the last three interior columns of a cell whose last group holds r pixels
    cands, align = [], set()
    for l in range(nlevels):
        I = ref.level(l)
        cd = ref.candidates(l)
        cands.append(cd)
        sb, sd, m, n, _, _ = score_maps(I)
        cells, _, _ = cells_of(I.shape[1], I.shape[0])
        cx, cy = cd["x"].astype(np.int64) + 16, cd["y"].astype(np.int64) + 16
        assert np.array_equal(np.maximum(sb, sd)[cy, cx], cd["response"].astype(np.int64)), "the numpy score map disagrees with the oracle"
        for ix, iy, cw, ch in cells:
            if cw < 7 or ch < 7:
                continue
            if l == 0:
                align.add((ix - 1) & 3)
            x0, y0, iw, ih = ix + 3, iy + 3, cw - 6, ch - 6
            inc = (cx >= x0) & (cx < x0 + iw) & (cy >= y0) & (cy < y0 + ih)
            if not inc.any():
                continue
            px, py = cx[inc] - x0, cy[inc] - y0
            for c in (0, 1, 2):
                kinds["col%d" % c] += int((px == c).sum())
            kinds["lastcols"] += int((px >= iw - 3).sum())
            if iw % 4:
                last[iw % 4] += int((px >= iw - 3).sum())
            kinds["row_first"] += int((py == 0).sum()); kinds["row_last"] += int((py == ih - 1).sum())
            if cd["response"][inc].max() < INI_TH:
                kinds["second_pass"] += int(inc.sum())
            R = (slice(y0, y0 + ih), slice(x0, x0 + iw))
            p20 = (m[R] > INI_TH) | (n[R] > INI_TH)             # pairs phase 1 lists at the first threshold
            pe = np.pad(p20, ((0, 0), (0, iw & 1)))
            per_row = (pe[:, 0::2] | pe[:, 1::2]).sum(1)
            rstep = 64 // ((iw + 3) // 4)
            filled = np.cumsum([per_row[a:a + rstep].sum() for a in range(0, ih, rstep)])
            if (filled[:-1] + SWEEP > LIST_CAP).any():          # no room for another sweep while rows remain: a second batch
                kinds["wrap"] += 1
    return kinds, last, align, ref, rk, rd, cands


def check(e, img, ref, rk, rd, cands, what, nlevels=2):
    k, d = e(img)
    for l in range(nlevels):
        assert np.array_equal(e.pyramid_level(0, l), ref.level(l)), "%s: pyramid level %d" % (what, l)
        g, r = e.candidates(0, l), cands[l]
        assert len(g) == len(r) and all(np.array_equal(g[f], r[f]) for f in ("x", "y", "response")), "%s: FAST level %d" % (what, l)
    assert len(k) == len(rk) and k.tobytes() == rk.tobytes(), "%s: keypoints differ" % what
    assert np.array_equal(d, rd), "%s: descriptors differ" % what


_last = {}


@pytest.mark.parametrize("w,h,tp", GEOMETRIES)
def test_tile_geometry(corb, pyorc, w, h, tp):
    img = build_image(w, h, 1)
    kinds, last, align, ref, rk, rd, cands = classify(pyorc, img)
    wcells = [cells_of(ref.level(l).shape[1], ref.level(l).shape[0])[1] for l in range(2)]
    need = 4 * ((max(wcells) + 3) // 4) + 8
    assert (40 if need <= 40 else 48 if need <= 48 else 80) == tp, "the geometry no longer selects orb_fast_kernel<%d>" % tp
    print(w, h, kinds, last, sorted(align))
    if w in (154, 156):
        l0 = cells_of(w, h)
        assert l0[1] == 31 and len(l0[0]) == 4 and align == {0, 1, 2, 3}, "level 0 no longer holds every write alignment"
        assert kinds["second_pass"] > 0 and kinds["wrap"] > 0, kinds
    if tp == 80:
        (ix, iy, cw, ch), = cells_of(w, h)[0]
        assert (cw, cw - 6) == (58, 52)
    for kd in EDGE_KINDS:
        assert kinds[kd] > 0, "the oracle reports no candidate of kind '%s' on the %d x %d image" % (kd, w, h)
    _last[(w, h)] = last
    # stale LDS: a saturated image of the same size first (its tiles, scores and lists stay behind in LDS), then the test image twice, on one extractor
    white = np.full((h, w), 255, np.uint8)
    wref = pyorc.Extractor(500, 1.2, 2, INI_TH, MIN_TH)
    wk, wd = wref.extract(white)
    wc = [wref.candidates(l) for l in range(2)]
    e = corb.ORBextractor(nfeatures=500, scaleFactor=1.2, nlevels=2, iniThFAST=INI_TH, minThFAST=MIN_TH, width=w, height=h)
    try:
        check(e, white, wref, wk, wd, wc, "all-255 image")
        check(e, img, ref, rk, rd, cands, "first run")
        check(e, img, ref, rk, rd, cands, "second run")
    finally:
        e.close()


def test_partial_last_groups(pyorc):
    """A candidate in the last three interior columns of cells whose last 4-pixel group holds 1, 2 and 3 pixels, over the geometries above (their GPU parity is asserted there)."""
    tot = {1: 0, 2: 0, 3: 0}
    for w, h, _ in GEOMETRIES:
        k = _last.get((w, h)) or classify(pyorc, build_image(w, h, 1))[1]
        for r in tot:
            tot[r] += k[r]
    assert all(tot[r] > 0 for r in tot), tot

"""FAST arc score by sides and the per-cell geometry table (pytest -m gpu): candidates (x, y, response per level) and final keypoints byte for
byte against the CPU oracle on hand-built images that hold what a one-sided score and a cell table can get wrong.

orb_fast_kernel scores a listed pixel with ONE sliding chain, on the side its compass test passes (the dark side on complemented bytes), and the
whole wave runs the second chain only when a pixel passes on both sides.  The images below hold: pixels that pass on both sides (corners and
non-corners), pixel pairs and 4-pixel groups whose pixels take opposite sides, centres and ring values of 0 and 255, a cell that needs the
second threshold (with both-sided pixels at that threshold), cells whose last 4-pixel group holds 1, 2 and 3 pixels, a cell at the right image
border 1 px wide and one too narrow to exist, and a cell that lists more pixel pairs than one sweep of the 512-entry list takes.  Every kind is
counted on the ORACLE's own pyramid levels and candidates (numpy, below), and a kind that is absent fails the test.

Geometries (scale 1.2, 2 levels; a level needs >= 62 px per axis): 152 x 74 has cells 30 and 32 px wide (tile pitch 40: orb_fast_kernel<40>),
112 x 74 has cells 40 and 31 px wide (tile pitch 48: orb_fast_kernel<48>); 783 x 74 ends in a cell of cw = 7 (interior 1 px), 813 x 74 in one of
cw = 6 (no cell)."""
import math
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INI_TH, MIN_TH = 20, 7
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]   # (dx, dy), cv::FAST order
LIST_CAP, SWEEP = 512, 128          # pair list of the kernel: a new batch starts when a whole sweep (128 pairs) no longer fits


def cells_of(w, h):
    """The reference's FAST grid of a level (ORBextractor.cc:773-805): (iniX, iniY, cw, ch) per cell incl. the 3-px ring, row-major; cw or ch < 7: no cell."""
    min_b, max_bx, max_by = 16, w - 16, h - 16
    width, height = float(max_bx - min_b), float(max_by - min_b)
    ncols, nrows = int(width / 30), int(height / 30)
    wcell, hcell = math.ceil(width / ncols), math.ceil(height / nrows)
    out = []
    for i in range(nrows):
        for j in range(ncols):
            ix, iy = min_b + j * wcell, min_b + i * hcell
            out.append((ix, iy, min(ix + wcell + 6, max_bx) - ix, min(iy + hcell + 6, max_by) - iy))
    return out, wcell, hcell


def score_maps(img):
    """Per pixel (3-px border left 0): bright and dark 9-of-16 arc scores (cornerScore = max of the two) and the compass margins m - c, c - n."""
    I = img.astype(np.int32)
    h, w = I.shape
    c = I[3:h - 3, 3:w - 3]
    ring = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in CIRCLE])              # 16, h-6, w-6
    arcs = np.stack([np.stack([ring[(s + k) % 16] for k in range(9)]) for s in range(16)])      # 16 arcs x 9
    sb = arcs.min(1).max(0) - c - 1
    sd = c - arcs.max(1).min(0) - 1
    m = np.minimum(np.maximum(ring[0], ring[8]), np.maximum(ring[4], ring[12])) - c
    n = c - np.maximum(np.minimum(ring[0], ring[8]), np.minimum(ring[4], ring[12]))
    pad = lambda a: np.pad(a, 3, constant_values=-1000)
    return pad(sb), pad(sd), pad(m), pad(n), np.pad(ring.min(0), 3), np.pad(ring.max(0), 3)


def stamp(img, x, y, centre, ring):
    img[y, x] = centre
    for (dx, dy), v in zip(CIRCLE, ring):
        img[y + dy, x + dx] = v


def build_image(w, h, seed):
    """Column bands (the level-0 cells are a single row): saturated binary noise, 5-level noise, noise within 18 grey levels (no corner at 20), flat + stamps."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 128, np.uint8)
    cells, wcell, _ = cells_of(w, h)
    ncols = len(cells)
    x_of = lambda j: 16 + 3 + j * wcell                    # first interior column of cell j
    # noise band (cell 0; with two cells: cell 1): rows split between {0, 255} noise (saturated centres and rings, most pairs listed) and 5-level noise
    # (both-sided pixels, opposite sides).  Low band (last cell but one; with two cells: cell 0): contrast <= 18 everywhere the cell and its ring can
    # see, so the cell has no corner at 20 and takes the second threshold
    if ncols >= 3:
        na, nb, la, lb = 0, x_of(1), x_of(ncols - 2) - 3, x_of(ncols - 1) + 3
        img[:, x_of(1):x_of(2)] = rng.choice(np.array([0, 64, 128, 192, 255], np.uint8), (h, x_of(2) - x_of(1)))
    else:
        na, nb, la, lb = x_of(1) + 3, w, 0, x_of(1) + 3
    img[:, na:nb] = rng.choice(np.array([0, 255], np.uint8), (h, nb - na))
    img[h // 2:, na:nb] = rng.choice(np.array([0, 64, 128, 192, 255], np.uint8), (h - h // 2, nb - na))
    img[:, la:lb] = rng.choice(np.array([119, 128, 137], np.uint8), (h, lb - la))
    if ncols >= 3:
        # last cell: flat 128 with hand-built both-sided pixels: bright arc of 9 (corner on the bright side) / dark arc of 9 / 8 + 8 (corner on neither side)
        x = x_of(ncols - 1) + 8
        stamp(img, x, 26, 128, [255 if (k + 1) % 16 < 9 else 60 for k in range(16)])            # ring 15, 0 .. 7 bright, 8 .. 14 dark
        stamp(img, x + 10, 26, 128, [0 if (k + 1) % 16 < 9 else 200 for k in range(16)])
        stamp(img, x, 40, 128, [255 if k < 8 else 0 for k in range(16)])
        stamp(img, x + 10, 40, 255, [0 if k < 10 else 255 for k in range(16)])                  # centre 255
        stamp(img, x, 52, 0, [255 if k < 11 else 0 for k in range(16)])                         # centre 0
    return img


def classify(pyorc, img, nlevels=2):
    """Counts of every kind on the oracle's levels and candidates; returns (kinds, oracle extractor results)."""
    ref = pyorc.Extractor(500, 1.2, nlevels, INI_TH, MIN_TH)
    rk, rd = ref.extract(img)
    kinds = dict(both_corner=0, both_none=0, opp_pair=0, opp_group=0, centre0=0, centre255=0, ring0=0, ring255=0, second_pass=0, second_both=0, wrap=0,
                 last1=0, last2=0, last3=0, narrow=0)
    cands = []
    for l in range(nlevels):
        I = ref.level(l)
        cd = ref.candidates(l)
        cands.append(cd)
        sb, sd, m, n, rmin, rmax = score_maps(I)
        cells, _, _ = cells_of(I.shape[1], I.shape[0])
        cx, cy = cd["x"].astype(np.int64) + 16, cd["y"].astype(np.int64) + 16           # candidates carry level coordinates - 16
        assert np.array_equal(np.maximum(sb, sd)[cy, cx], cd["response"].astype(np.int64)), "the numpy score map disagrees with the oracle: the kinds below would be miscounted"
        for ix, iy, cw, ch in cells:
            if cw < 7 or ch < 7:
                continue
            x0, y0, iw, ih = ix + 3, iy + 3, cw - 6, ch - 6
            inc = (cx >= x0) & (cx < x0 + iw) & (cy >= y0) & (cy < y0 + ih)
            if not inc.any():
                continue
            resp = cd["response"][inc]
            t = INI_TH if resp.max() >= INI_TH else MIN_TH
            R = (slice(y0, y0 + ih), slice(x0, x0 + iw))
            B, D, bs, ds = sb[R], sd[R], m[R] > t, n[R] > t
            both = bs & ds
            cmask = np.zeros((ih, iw), bool); cmask[cy[inc] - y0, cx[inc] - x0] = True
            kinds["both_corner"] += int((both & cmask).sum())
            kinds["both_none"] += int((both & (np.maximum(B, D) < t)).sum())
            if t == MIN_TH:
                kinds["second_pass"] += int(inc.sum()); kinds["second_both"] += int(both.sum())
            cb, cdk = B >= t, D >= t                                                     # corner by its bright / dark arcs
            ev = iw & ~1
            kinds["opp_pair"] += int(((cb[:, 0:ev:2] & cdk[:, 1:ev:2]) | (cdk[:, 0:ev:2] & cb[:, 1:ev:2])).sum())
            g4 = iw & ~3
            p0b, p0d = cb[:, 0:g4:4] | cb[:, 1:g4:4], cdk[:, 0:g4:4] | cdk[:, 1:g4:4]
            p1b, p1d = cb[:, 2:g4:4] | cb[:, 3:g4:4], cdk[:, 2:g4:4] | cdk[:, 3:g4:4]
            kinds["opp_group"] += int(((p0b & ~p0d & p1d & ~p1b) | (p0d & ~p0b & p1b & ~p1d)).sum())
            cen = I[cy[inc], cx[inc]]
            kinds["centre0"] += int((cen == 0).sum()); kinds["centre255"] += int((cen == 255).sum())
            kinds["ring0"] += int((rmin[cy[inc], cx[inc]] == 0).sum()); kinds["ring255"] += int((rmax[cy[inc], cx[inc]] == 255).sum())
            # pairs phase 1 lists at the cell's first threshold: a pair with a pixel whose compass test passes
            p20 = (m[R] > INI_TH) | (n[R] > INI_TH)
            pe = np.pad(p20, ((0, 0), (0, iw & 1)))
            per_row = (pe[:, 0::2] | pe[:, 1::2]).sum(1)
            rstep = 64 // ((iw + 3) // 4)                                                # rows per sweep of the wave's patch
            filled = np.cumsum([per_row[a:a + rstep].sum() for a in range(0, ih, rstep)])
            if (filled[:-1] + SWEEP > LIST_CAP).any():                                   # no room for another sweep while rows remain: a second batch
                kinds["wrap"] += 1
            if iw % 4 and ((cx[inc] - x0) >= (iw & ~3)).any():
                kinds["last%d" % (iw % 4)] += 1
            if iw == 1:
                kinds["narrow"] += int(inc.sum())
    return kinds, ref, rk, rd, cands


def check_gpu(corb, img, ref, rk, rd, cands, nlevels=2):
    e = corb.ORBextractor(nfeatures=500, scaleFactor=1.2, nlevels=nlevels, iniThFAST=INI_TH, minThFAST=MIN_TH, width=img.shape[1], height=img.shape[0])
    try:
        k, d = e(img)
        for l in range(nlevels):
            assert np.array_equal(e.pyramid_level(0, l), ref.level(l)), "pyramid level %d" % l
            g, r = e.candidates(0, l), cands[l]
            assert len(g) == len(r) and all(np.array_equal(g[f], r[f]) for f in ("x", "y", "response")), "FAST level %d" % l
        assert len(k) == len(rk) and k.tobytes() == rk.tobytes(), "keypoints differ"
        assert np.array_equal(d, rd)
    finally:
        e.close()


PIXEL_KINDS = ("both_corner", "both_none", "opp_pair", "opp_group", "centre0", "centre255", "ring0", "ring255", "second_pass", "second_both", "wrap")
_last = {}


@pytest.mark.parametrize("w,tp", [(152, 40), (112, 48)])
def test_sides_and_saturation(corb, pyorc, w, tp):
    img = build_image(w, 74, 0)
    kinds, ref, rk, rd, cands = classify(pyorc, img)
    wcells = [cells_of(ref.level(l).shape[1], ref.level(l).shape[0])[1] for l in range(2)]
    assert 4 * ((max(wcells) + 3) // 4) + 8 == tp, "the geometry no longer selects orb_fast_kernel<%d>" % tp
    print(w, kinds)
    for kd in PIXEL_KINDS:
        assert kinds[kd] > 0, "the oracle reports no case of kind '%s' on the %d-px image" % (kd, w)
    _last[w] = {r: kinds["last%d" % r] for r in (1, 2, 3)}
    check_gpu(corb, img, ref, rk, rd, cands)


def test_partial_last_groups(pyorc):
    """A candidate in a last 4-pixel group of 1, 2 and 3 valid pixels, over the two geometries above (their GPU parity is asserted there)."""
    tot = {r: 0 for r in (1, 2, 3)}
    for w in (152, 112):
        k = _last.get(w) or {r: classify(pyorc, build_image(w, 74, 0))[0]["last%d" % r] for r in (1, 2, 3)}
        for r in tot:
            tot[r] += k[r]
    assert all(tot[r] > 0 for r in tot), tot


@pytest.mark.parametrize("w,cw_last", [(783, 7), (813, 6)])
def test_image_edge_cells(corb, pyorc, w, cw_last):
    rng = np.random.default_rng(w)
    img = rng.choice(np.array([0, 64, 128, 192, 255], np.uint8), (74, w))
    cells, _, _ = cells_of(w, 74)
    assert cells[-1][2] == cw_last and cells[-2][2] >= 7
    kinds, ref, rk, rd, cands = classify(pyorc, img)
    if cw_last >= 7:
        assert kinds["narrow"] > 0, "the oracle reports no candidate in the 1-px-wide border cell"
    else:
        assert not (cands[0]["x"].astype(np.int64) + 16 >= cells[-1][0] + 3).any()      # nothing right of the last full cell
    check_gpu(corb, img, ref, rk, rd, cands)

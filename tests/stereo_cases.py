"""Seeded stereo pairs shared by the stereo-matcher tests (restatement on the CPU, kernels on the device), the oracle's answer and the restatement's kind
counts for each, computed once per process.

A case is (left, right, configuration): the configuration names a geometry (image size and extractor settings) and the intrinsics (fx, bf) that
Frame::ComputeStereoMatches takes its disparity bounds from (mb = bf / fx, maxD = bf / mb).  SUPPLIES says which case is there for which kind
(tests/stereo_reference.py lists the kinds): test_stereo_reference.py asserts every entry on the oracle's data, so a failure names the input to repair, and
test_gpu_stereo_kinds.py asserts that the cases it runs cover every required kind by this table.

The cases (l, r = synth.stereo_pair(3) at the geometry's size; counts are the oracle's at the time of writing, the tests only ask for > 0):
  plain             (l, r) at the default intrinsics: rows with > 32 candidates, closer candidates of a wrong octave (88) or right of maxU (151), Hamming ties (15),
                    best distances of exactly 74 and 75, rejected distances (255), no acceptable candidate (21), best shift at an end (34), a SAD tie, 67 matches
                    filtered and 78 kept above a median >= 256, an even number of matches
  fx30, fx12        the same pair at fx = 30, bf = 16 and fx = 12, bf = 6 (maxD = fx): closer candidates left of minU (414 / 346), disparity >= maxD (1 / 2); the
                    second leaves exactly one match
  same              (l, l): every best candidate sits at uR == maxU, 290 negative disparities, median 0, so all 312 matches are rejected
  partial           the right eye equals stereo_pair(8)'s left with +-2 grey levels of noise over the left 70 % of the columns: zero disparities whose clamp
                    survives the filter
  noise_roll5, binary_roll4   uniform noise rolled by -5 px, {0, 255} noise rolled by -4 px: median 0 with hundreds of matches, saturated bytes in the SAD
  tile16            a column tile of period 16 px rolled by -3 px: 183 Hamming ties; its left eye has a multiple of 4 keypoints
  alt_rows          the right eye rolled by -6 px and every second row by another 2: best shifts at an end, SAD ties
  half_contrast     the right eye at 0.5 x + 60: an odd number of matches, distances of exactly 74 and 75
  swapped           (r, l): N_left = 4 k + 1
  right_flat_below  the right eye flat below mid-height: 226 left keypoints whose row has no candidate
  flat_left, flat_right, flat_flat   an eye (or both) without keypoints: left keypoints but no match
  two_rects         two rectangles, the lower one missing in the right eye: 11 and 10 keypoints, 6 rows without candidate, N_left = 4 k + 3
  rect7             one rectangle shifted by 7 px: 12 keypoints, matches kept above the median
  lt4               a 3 x 3 dot: two left keypoints
  deep_*, flat2_*   the plain, partial and tile16 pairs at 701 x 231 with 8 levels and at 152 x 74 with 2 levels"""
import numpy as np

import stereo_reference as R

DEFAULT_FX, DEFAULT_BF = 718.856, 386.1448
# geometry -> (width, height, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
GEOMETRIES = {
    "base": (320, 120, 600, 1.2, 4, 20, 7),
    "deep": (701, 231, 1200, 1.2, 8, 20, 7),        # 8 levels, odd width and height (the level-0 pitch differs from the width); the top level is 196 x 64
    "flat2": (152, 74, 500, 1.2, 2, 20, 7),         # 2 levels
}
# configuration -> (geometry, fx, bf): one front-end handle each on the device
CONFIGS = {
    "base": ("base", DEFAULT_FX, DEFAULT_BF),
    "base_fx30": ("base", 30.0, 16.0),
    "base_fx12": ("base", 12.0, 6.0),
    "deep": ("deep", DEFAULT_FX, DEFAULT_BF),
    "flat2": ("flat2", DEFAULT_FX, DEFAULT_BF),
}

# case -> (configuration, kinds the case must show).  Order matters to the per-frame route of the device test: a sparse frame follows a dense one, and "same"
# (every match rejected) follows a frame with matches.
SUPPLIES = {
    "plain": ("base", ("cand17", "cand33", "oct_better", "right_better", "ham_tie", "ham_reject", "none_ok", "edge_inc", "sad_tie", "filt_rej", "med_hi",
                       "filt_kept_above_median", "n_even", "ham_eq_th", "ham_below_th")),
    "same": ("base", ("at_maxU", "disp_neg", "med_zero", "filt_rej")),
    "partial": ("base", ("clamp_kept", "at_maxU")),
    "two_rects": ("base", ("no_cand", "nl_mod4", "nl_rem3")),
    "noise_roll5": ("base", ("med_zero", "filt_rej", "nl_rem3")),
    "lt4": ("base", ("nl_lt4", "nl_mod4", "nl_rem2")),
    "binary_roll4": ("base", ("med_zero",)),
    "tile16": ("base", ("ham_tie",)),
    "alt_rows": ("base", ("edge_inc", "sad_tie")),
    "half_contrast": ("base", ("filt_rej", "n_odd", "ham_eq_th", "ham_below_th")),
    "swapped": ("base", ("right_better", "ham_reject", "nl_rem1")),
    "right_flat_below": ("base", ("no_cand",)),
    "flat_left": ("base", ()),
    "flat_right": ("base", ("no_cand", "no_match_with_keypoints")),
    "rect7": ("base", ("filt_kept_above_median",)),
    "flat_flat": ("base", ()),
    "fx30": ("base_fx30", ("left_better", "disp_big")),
    "fx12": ("base_fx12", ("left_better", "disp_big", "single_match")),
    "deep_plain": ("deep", ("cand33", "oct_better", "filt_rej", "med_hi", "ham_eq_th", "ham_below_th")),
    "deep_partial": ("deep", ("at_maxU",)),
    "deep_tile16": ("deep", ("ham_tie",)),
    "flat2_plain": ("flat2", ("ham_reject",)),
    "flat2_partial": ("flat2", ("at_maxU",)),
    "flat2_tile16": ("flat2", ("ham_tie",)),
}
CASES = list(SUPPLIES)


def geometry_of(case):
    return GEOMETRIES[CONFIGS[SUPPLIES[case][0]][0]]


def cases_of(config):
    return [c for c in CASES if SUPPLIES[c][0] == config]


def _partial(left, seed, amplitude, share):
    """the right eye equals the left; noise of +-amplitude grey levels over the left `share` of the columns"""
    rng = np.random.default_rng(seed)
    h, w = left.shape
    cut = int(w * share)
    right = left.astype(np.int16)
    right[:, :cut] += rng.integers(-amplitude, amplitude + 1, (h, cut), dtype=np.int16)
    return left, np.clip(right, 0, 255).astype(np.uint8)


def _tile16(w, h, seed):
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, (h, 16), dtype=np.uint8)
    t = np.ascontiguousarray(np.tile(noise, (1, w // 16 + 1))[:, :w])
    return t, np.roll(t, -3, axis=1)


_images = {}


def images(synth, case):
    """(left, right) of a case; built once, callers must not modify them"""
    if case in _images:
        return _images[case]
    w, h = geometry_of(case)[:2]
    flat = synth.flat_image(w, h)
    l, r = synth.stereo_pair(3, w, h)
    rng = np.random.default_rng(1000 + CASES.index(case))
    kind = case.split("_", 1)[1] if case.startswith(("deep_", "flat2_")) else case
    if kind in ("plain", "fx30", "fx12"):
        out = (l, r)
    elif kind == "same":
        out = (l, l)
    elif kind == "partial":
        out = _partial(synth.stereo_pair(8, w, h)[0], 1, 2, 0.7)
    elif kind == "noise_roll5":
        n = np.random.default_rng(1).integers(0, 256, (h, w), dtype=np.uint8); out = (n, np.roll(n, -5, axis=1))
    elif kind == "binary_roll4":
        n = rng.choice(np.array([0, 255], np.uint8), (h, w)); out = (n, np.roll(n, -4, axis=1))
    elif kind == "tile16":
        out = _tile16(w, h, 7)
    elif kind == "alt_rows":
        rr = np.roll(l, -6, axis=1); rr[1::2] = np.roll(rr[1::2], -2, axis=1); out = (l, rr)
    elif kind == "half_contrast":
        out = (l, (0.5 * r.astype(np.float32) + 60).astype(np.uint8))
    elif kind == "swapped":
        out = (r, l)
    elif kind == "right_flat_below":
        rr = r.copy(); rr[h // 2:] = 128; out = (l, rr)
    elif kind == "flat_left":
        out = (flat, r)
    elif kind == "flat_right":
        out = (l, flat)
    elif kind == "flat_flat":
        out = (flat, flat)
    elif kind == "two_rects":
        a = flat.copy(); a[30:50, 60:100] = 255; a[80:100, 200:240] = 30
        b = np.roll(a, -9, axis=1); b[70:110] = 128
        out = (a, b)
    elif kind == "rect7":
        a = flat.copy(); a[40:80, 120:180] = 230
        out = (a, np.roll(a, -7, axis=1))
    elif kind == "lt4":
        a = flat.copy(); a[58:61, 158:161] = 255                                    # a 3 x 3 dot: two keypoints
        out = (a, np.roll(a, -6, axis=1))
    else:
        raise KeyError(case)
    out = tuple(np.ascontiguousarray(x, np.uint8) for x in out)
    assert out[0].shape == out[1].shape == (h, w)
    _images[case] = out
    return out


_oracle = {}


def oracle(pyorc, synth, case):
    """the oracle's extraction of both eyes and its stereo match: dict(kl, dl, kr, dr, u_right, depth, n_matched, levels_l, levels_r, scale, inv_scale)"""
    if case in _oracle:
        return _oracle[case]
    _, fx, bf = CONFIGS[SUPPLIES[case][0]]
    w, h, nf, sf, nl, ini, mn = geometry_of(case)
    left, right = images(synth, case)
    el, er = pyorc.Extractor(nf, sf, nl, ini, mn), pyorc.Extractor(nf, sf, nl, ini, mn)
    kl, dl = el.extract(left); kr, dr = er.extract(right); tb = el.tables()
    ur, dp, nm = pyorc.stereo_match(el, er, kl, dl, kr, dr, bf, fx, tb["scale"], tb["inv_scale"])
    o = dict(kl=kl, dl=dl, kr=kr, dr=dr, u_right=ur, depth=dp, n_matched=nm, levels_l=[el.level(i) for i in range(nl)], levels_r=[er.level(i) for i in range(nl)],
             scale=tb["scale"], inv_scale=tb["inv_scale"])
    _oracle[case] = o
    return o


_restated = {}


def restated(pyorc, synth, case):
    """the numpy restatement on the oracle's keypoints and levels: (u_right, depth, n_matched, kinds, decision)"""
    if case not in _restated:
        o = oracle(pyorc, synth, case)
        _, fx, bf = CONFIGS[SUPPLIES[case][0]]
        _restated[case] = R.match(o["kl"], o["dl"], o["kr"], o["dr"], o["levels_l"], o["levels_r"], o["scale"], o["inv_scale"], bf, fx)
    return _restated[case]


def describe(case):
    return "case '%s' (configuration %s; there for: %s)" % (case, SUPPLIES[case][0], ", ".join(SUPPLIES[case][1]) or "no kind of its own")

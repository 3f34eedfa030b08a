"""Frame::ComputeStereoMatches (Frame.cc:470-644) restated in numpy as the CPU oracle states it (oracle/orc_match.c: orc_stereo_match), with a classifier that
counts which of the matcher's decisions an input reaches.  The restatement works in np.float32 steps (one rounding per operation, no fused multiply-add); the one
exception is the zero-disparity clamp's uR = float(uL) - 0.01, computed in double and rounded to float once.  The SAD sums are integers (bytes minus a byte), so
their summation order is free and their conversion to float is exact (<= 121 * 510 < 2^24).

match(...) returns (u_right, depth, n_matched, kinds, decision): kinds is a dict of counts, decision the last decision taken per left keypoint (a name from
DECISIONS).  The counts are only as good as the restatement: tests/test_stereo_reference.py asserts its u_right / depth bit patterns and n_matched equal the
oracle's on every case before it reads a count.

Kinds per left keypoint, in the oracle's order of decisions
  no_cand        the keypoint's row has no right keypoint in the row table
  cand17, cand33 the row lists more than 16 / more than 32 candidates (second half of a 16-lane group's trip / second trip of the device's candidate loop)
  none_ok        candidates exist but none passes both the octave test and uR in [minU, maxU]
  oct_better     a candidate excluded ONLY by the octave test is closer (Hamming) than the accepted best
  right_better   a candidate of an allowed octave with uR > maxU is closer than the accepted best
  left_better    the same with uR < minU
  at_maxU        the accepted best has uR == maxU exactly (the bound is inclusive)
  ham_tie        two or more accepted candidates share the best distance (the lowest iR wins: strict '<' over ascending iR)
  ham_reject     best distance >= (TH_HIGH + TH_LOW) / 2, which includes "every accepted candidate is at TH_HIGH or more"
  ham_eq_th, ham_below_th   best distance exactly (TH_HIGH + TH_LOW) / 2 = 75 (the first value rejected: the test is strict) / exactly 74 (the last accepted)
  sad_tie        two shifts share the minimum SAD (the first shift wins)
  edge_inc       the best shift is -5 or +5: no parabola, no match
  disp_neg       disparity < 0
  disp_big       disparity >= maxD
  clamp_kept     disparity == 0, clamped to 0.01 (uR = uL - 0.01 in double), and the match survives the median filter: depth == f32(bf) / f32(0.01)
  filt_rej       a match the filter rejects: SAD >= 1.5f * 1.4f * median
  filt_kept_above_median   a match the filter keeps although its SAD is above the median
Kinds per frame
  med_zero       the median SAD is 0: the threshold is 0 and every match is rejected
  med_hi         the median SAD is >= 256 (the high digit of the device's two-pass radix selection is not 0)
  single_match   exactly one match reaches the filter
  n_even, n_odd  the number of matches before the filter is even / odd (the median is element n / 2 of the sorted list)
  no_match_with_keypoints  left keypoints exist but no match reaches the filter
  nl_mod4        the number of left keypoints is no multiple of 4: the last wavefront of the device holds a partly filled set of 16-lane groups
  nl_rem1, nl_rem2, nl_rem3   the same by remainder: 1, 2 or 3 of the last wavefront's four groups hold a keypoint
  nl_lt4         1 to 3 left keypoints

Decisions that the front-end cannot reach (UNREACHABLE): the classifier counts them all the same and the CPU test asserts every count is 0.  Should one turn out
non-zero, the input is kept and the kind moves to the required list.
  row_clip       a right keypoint's row range floor(y - r) .. ceil(y + r) leaves [0, rows0 - 1], or a left keypoint's row does.  An extracted keypoint of octave o
                 sits >= 16 px from the border of its level (EDGE_THRESHOLD 19 minus the 3-px FAST ring), so its level-0 y is >= 16 s and <= (h_o - 16) s with
                 s = scale[o] >= 1 and h_o s about h; the radius is r = 2 s, eight times smaller than the margin.
  guard_span     iniu < 0 || endu >= w: the 21-px span of the right patch over all shifts around round(uR0 / s).  The rounded level coordinate of an extracted
                 keypoint is the integer the extractor found it at (x_level * s * (1 / s) rounds back), >= 16 px from each border; the span needs 5 px to the
                 left and 11 to the right.
  guard_defined  the oracle's defined guard behind it (the reference would index outside the image): the patches need 10 px to the left / above and 10 below /
                 to the right, again < 16.
  delta_out      deltaR outside [-1, 1] or NaN.  The chosen shift is the FIRST minimum and not at an end, so d1 > d2 and d3 >= d2: the denominator
                 2 (d1 + d3 - 2 d2) is > 0 and |d1 - d3| <= d1 + d3 - 2 d2, hence |deltaR| <= 0.5.
  row_overflow   the row table holds more entries than the device allots, row_cap = capacity * (2 ceil(2 scale[top]) + 2), capacity = the keypoints an eye
                 can return: floor(y - r) .. ceil(y + r) covers at most 2 ceil(r) + 2 rows and r <= 2 scale[top].  Counted per right keypoint that covers more.
  maxu_neg       maxU = uL < 0: keypoint coordinates are >= 16.
"""
import numpy as np

TH_HIGH, TH_LOW = 100, 50
TH_ORB = (TH_HIGH + TH_LOW) // 2
W = 5            # half patch
L = 5            # shifts -L .. L

KP_KINDS = ("no_cand", "cand17", "cand33", "none_ok", "oct_better", "right_better", "left_better", "at_maxU", "ham_tie", "ham_reject", "ham_eq_th", "ham_below_th", "sad_tie", "edge_inc",
            "disp_neg", "disp_big", "clamp_kept", "filt_rej", "filt_kept_above_median")
FRAME_KINDS = ("med_zero", "med_hi", "single_match", "n_even", "n_odd", "no_match_with_keypoints", "nl_mod4", "nl_rem1", "nl_rem2", "nl_rem3", "nl_lt4")
REQUIRED = KP_KINDS + FRAME_KINDS
UNREACHABLE = ("row_clip", "guard_span", "guard_defined", "delta_out", "row_overflow", "maxu_neg")
DECISIONS = ("row_clip", "no_cand", "maxu_neg", "none_ok", "ham_reject", "guard_span", "guard_defined", "edge_inc", "delta_out", "disp_neg", "disp_big",
             "filt_rej", "clamp_kept", "kept")

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
f32 = np.float32


def roundf(x):
    """C roundf of a float: half away from zero (float + 0.5 is exact in double)"""
    x = float(x)
    return f32(np.floor(x + 0.5) if x >= 0 else -np.floor(-x + 0.5))


def match(kl, dl, kr, dr, levels_l, levels_r, scale, inv_scale, bf, fx):
    """kl, kr: the oracle's keypoints (x, y, octave); dl, dr: n x 32 uint8; levels_*: the oracle's pyramid levels per eye; scale, inv_scale: its tables."""
    N, Nr = len(kl), len(kr)
    scale = np.asarray(scale, f32); inv_scale = np.asarray(inv_scale, f32)
    kinds = {k: 0 for k in REQUIRED + UNREACHABLE}
    decision = ["no_cand"] * N
    u_right = np.full(N, -1.0, f32); depth = np.full(N, -1.0, f32)
    n_rows = levels_l[0].shape[0]
    bf = f32(bf); mb = bf / f32(fx)
    max_d = bf / mb
    # row table (:481-497): the candidates of a row in ascending iR
    rows = [[] for _ in range(n_rows)]
    krx, kry, kro = kr["x"].astype(f32), kr["y"].astype(f32), kr["octave"].astype(np.int64)
    rows_per_keypoint = 2 * int(np.ceil(f32(2.0) * scale[-1])) + 2
    for iR in range(Nr):
        r = f32(2.0) * scale[kro[iR]]
        maxr, minr = int(np.ceil(kry[iR] + r)), int(np.floor(kry[iR] - r))
        if minr < 0 or maxr >= n_rows:
            kinds["row_clip"] += 1
        kinds["row_overflow"] += maxr - minr + 1 > rows_per_keypoint
        for yi in range(max(minr, 0), min(maxr, n_rows - 1) + 1):
            rows[yi].append(iR)
    dl = np.ascontiguousarray(dl, np.uint8).reshape(N, 32); dr = np.ascontiguousarray(dr, np.uint8).reshape(Nr, 32)
    found = []                                       # (SAD, iL)
    clamped = set()
    for iL in range(N):
        level = int(kl["octave"][iL]); vL, uL = f32(kl["y"][iL]), f32(kl["x"][iL])
        row = int(vL)
        if row < 0 or row >= n_rows:
            kinds["row_clip"] += 1; decision[iL] = "row_clip"; continue
        cand = np.asarray(rows[row], np.int64)
        if len(cand) == 0:
            kinds["no_cand"] += 1; decision[iL] = "no_cand"; continue
        min_u, max_u = uL - max_d, uL
        if max_u < 0:
            kinds["maxu_neg"] += 1; decision[iL] = "maxu_neg"; continue
        kinds["cand17"] += len(cand) > 16; kinds["cand33"] += len(cand) > 32
        oct_ok = (kro[cand] >= level - 1) & (kro[cand] <= level + 1)
        uR = krx[cand]
        in_u = (uR >= min_u) & (uR <= max_u)
        dist = _POP[np.bitwise_xor(dr[cand], dl[iL][None, :])].sum(1)
        acc = oct_ok & in_u
        if not acc.any():
            kinds["none_ok"] += 1; decision[iL] = "none_ok"; continue
        best_dist, best_r = TH_HIGH, 0               # int bestDist = TH_HIGH; size_t bestIdxR = 0
        for j in np.nonzero(acc)[0]:
            if dist[j] < best_dist:
                best_dist, best_r = int(dist[j]), int(cand[j])
        kinds["oct_better"] += bool((in_u & ~oct_ok & (dist < best_dist)).any())
        kinds["right_better"] += bool((oct_ok & (uR > max_u) & (dist < best_dist)).any())
        kinds["left_better"] += bool((oct_ok & (uR < min_u) & (dist < best_dist)).any())
        if best_dist < TH_HIGH:
            kinds["at_maxU"] += bool(krx[best_r] == max_u)
            kinds["ham_tie"] += int((acc & (dist == best_dist)).sum()) >= 2
        kinds["ham_eq_th"] += best_dist == TH_ORB; kinds["ham_below_th"] += best_dist == TH_ORB - 1
        if not best_dist < TH_ORB:
            kinds["ham_reject"] += 1; decision[iL] = "ham_reject"; continue
        # sub-pixel refinement by 11 x 11 SAD over the shifts (:556-626)
        uR0 = krx[best_r]
        sf = inv_scale[level]
        su_l, sv_l, su_r0 = roundf(uL * sf), roundf(vL * sf), roundf(uR0 * sf)
        im_l, im_r = levels_l[level], levels_r[level]
        lh, lw = im_l.shape; rw = im_r.shape[1]
        y0, x0 = int(sv_l - f32(W)), int(su_l - f32(W))
        iniu = su_r0 + f32(L) - f32(W); endu = su_r0 + f32(L) + f32(W) + f32(1)
        if iniu < 0 or endu >= rw:
            kinds["guard_span"] += 1; decision[iL] = "guard_span"; continue
        if int(su_r0 - f32(L) - f32(W)) < 0 or x0 < 0 or y0 < 0 or y0 + 10 >= lh or x0 + 10 >= lw:
            kinds["guard_defined"] += 1; decision[iL] = "guard_defined"; continue
        IL = im_l[y0:y0 + 11, x0:x0 + 11].astype(np.int64); IL = IL - IL[W, W]
        best_s, best_inc = 2 ** 31 - 1, 0            # int bestDist = INT_MAX, compared as float
        d = np.zeros(2 * L + 1, f32)
        for inc in range(-L, L + 1):
            xr0 = int(su_r0 + f32(inc) - f32(W))
            IR = im_r[y0:y0 + 11, xr0:xr0 + 11].astype(np.int64); IR = IR - IR[W, W]
            s = f32(np.abs(IL - IR).sum())
            if s < f32(best_s):
                best_s, best_inc = int(s), inc
            d[L + inc] = s
        kinds["sad_tie"] += int((d == d.min()).sum()) >= 2
        if best_inc == -L or best_inc == L:
            kinds["edge_inc"] += 1; decision[iL] = "edge_inc"; continue
        d1, d2, d3 = d[L + best_inc - 1], d[L + best_inc], d[L + best_inc + 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            delta = (d1 - d3) / (f32(2.0) * (d1 + d3 - f32(2.0) * d2))
        if np.isnan(delta) or delta < -1 or delta > 1:
            kinds["delta_out"] += 1; decision[iL] = "delta_out"
            if not np.isnan(delta):                  # (a NaN passes the oracle's two comparisons)
                continue
        best_ur = scale[level] * (su_r0 + f32(best_inc) + delta)
        disp = uL - best_ur
        if disp >= 0 and disp < max_d:
            if disp <= 0:
                disp = f32(0.01); best_ur = f32(float(uL) - 0.01); clamped.add(iL)
            depth[iL] = bf / disp; u_right[iL] = best_ur
            found.append((best_s, iL)); decision[iL] = "kept"
        elif disp < 0:
            kinds["disp_neg"] += 1; decision[iL] = "disp_neg"
        else:
            kinds["disp_big"] += 1; decision[iL] = "disp_big"
    # median filter (:630-643)
    n = len(found)
    n_matched = n
    if N > 0:
        kinds["nl_mod4"] += N % 4 != 0; kinds["nl_lt4"] += N < 4
        if N % 4:
            kinds["nl_rem%d" % (N % 4)] += 1
        kinds["no_match_with_keypoints"] += n == 0
    if n > 0:
        found.sort()
        kinds["single_match"] += n == 1; kinds["n_even"] += n % 2 == 0; kinds["n_odd"] += n % 2 == 1
        median = f32(found[n // 2][0])
        th = f32(1.5) * f32(1.4) * median
        kinds["med_zero"] += bool(median == 0); kinds["med_hi"] += bool(median >= 256)
        for s, iL in reversed(found):
            if f32(s) < th:
                break
            u_right[iL] = -1; depth[iL] = -1; n_matched -= 1
            kinds["filt_rej"] += 1; decision[iL] = "filt_rej"
        for s, iL in found:
            if decision[iL] != "kept":
                continue
            kinds["filt_kept_above_median"] += bool(f32(s) > median)
            if iL in clamped:
                assert depth[iL] == bf / f32(0.01)
                kinds["clamp_kept"] += 1; decision[iL] = "clamp_kept"
    return u_right, depth, n_matched, {k: int(v) for k, v in kinds.items()}, decision

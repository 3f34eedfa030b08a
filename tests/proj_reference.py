"""The projection matchers of the Tracking thread restated as plain sequential Python, with a classifier that counts which of their decisions an input reaches:
  ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)       search_map
  ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)            search_frame
  ORBmatcher::SearchForInitialization                                        search_init
  Frame::PosInGrid / AssignFeaturesToGrid / GetFeaturesInArea                build_grid, features_in_area
  ORBmatcher::ComputeThreeMaxima                                             three_maxima
It restates the decisions of the CPU oracle (oracle/orc_proj.c) and shares no code with it; tests/test_proj_reference.py asserts its outputs equal to the oracle's
on every input before it reads a count.  Arithmetic is in np.float32 steps (one rounding per operation, no fused multiply-add); the 3 x 3 products accumulate in
double and round once (cv::gemm on CV_32F).  roundf is restated (half away from zero; numpy.round rounds half to even).

DEFINED: (int)floorf(NaN) is undefined in C.  A point at the camera centre projects to u = v = NaN, which passes the four bound comparisons; here a NaN window
centre has no candidates (kind nan_window).  The oracle (x86: the conversion gives INT_MIN, so nMaxCellX < 0) and the device (the conversion gives 0, then every
|dx| < r is false) both end without a match for that query: only that common outcome is asserted.

Every function returns (..., kinds, notes): kinds is a dict of counts over ALL_KINDS (per query unless said otherwise), notes a list with one line per query (its
decision), which the device test prints for the queries whose features differ.

Kinds, grid and candidates (all three matchers)
  grid_out        a feature that PosInGrid rounds out of the grid (per feature)
  grid_last_col   a feature in column 63 (the last one that is in)
  clamp_left, clamp_right, clamp_top, clamp_bottom   the window's cell range is clamped at that border
  win_outside     a valid query whose window lies wholly outside the grid
  win_gt64        a window of more than 64 cells (second sweep of the device's lane loop)
  multi_next_empty  a cell with >= 2 features whose neighbour in the device's lane order (same sweep of 64) is empty
  edge_dx, edge_dy  a feature of an allowed octave at |dx| == r (|dy| == r) exactly: excluded
  oct_below, oct_at_min, oct_at_max, oct_above   a feature in the cells at octave min_level - 1 / min_level / max_level / max_level + 1 of a level-checked query
  level0_query    a query with min_level == -1 (a level-0 map point)
  ur_reject, ur_eq, ur_zero, ur_neg   u_right > 0 with |err| > r (rejected) / == r (accepted) / u_right == 0 (no stereo value: not tested) / u_right < 0
  preclaimed_skip a candidate claimed on entry
  cand12, cand13, cand65, cand256, cand_over   the device's candidate list (area + u_right test, claimed ones included) holds exactly 12 / exactly 13 / more than 64 /
                  exactly 256 (2048 for initialisation: cand2048) / more than that (the call reports an overflow)
Greedy resolution (map and frame)
  tie_ix, tie_iy, tie_feat   the best distance is shared; the winner differs from the runner-up by column / by row / only by feature index
  tie_ix_high, tie_iy_high   ... and the winner has a HIGHER feature index than a tied loser (visiting order, not index, decides)
  dist_100, dist_101          bestDist == TH_HIGH accepted / 101 rejected
  ratio_eq, ratio_reject, ratio_level_pass   map: same level and (float)bestDist == nnratio * bestDist2 (accepted) / > (rejected) / the distances would be
                  rejected but the levels differ (accepted)
  single_cand     one candidate in the list
  best_taken      the best candidate by the state on entry was taken by an earlier query of this call
  second_flip     the best is the same, the second best was taken by an earlier query and the ratio outcome differs from the one on entry (map)
  all_taken       the list is not empty but every candidate is claimed
  overwrite       the matched feature already holds an earlier (non-claiming) query of this call: overwritten, both counted
  chain8          dependency depth >= 8 (depth = 1 + the largest depth of an earlier query sharing a candidate that was free on entry)
  deep1024, deep2048   a query of depth >= 2 that matches, with a list longer than 12, at an index in [1024, 2048) / >= 2048
Frame overload
  fwd_oct0, fwd_octpos, backward, neither   the level window of a query by the host's motion rule
  mono_large_z, z_eq_mb   per call: mono with tlc.z > mb / tlc.z == mb exactly (strict: neither)
  invz_neg, out_left, out_right, out_top, out_bottom, nan_window
Rotation (frame and initialisation)
  rot_wrap, rot_half, bin12   rot < 0 wrapped / rot * (1/30) exactly on a half / bin 12
  hist_lt3, max2_tie, max2_tenth, max2_drop, max3_drop   per call: fewer than three non-empty bins / max2 == max1 / (float)max2 == 0.1f * max1 (kept) / max2 dropped /
                  max3 dropped alone
  ori_removed     a match removed by the rotation pass
  ori_overwritten frame: the removed feature belongs to a later query (the event is that of an overwritten earlier query)
Initialisation
  f1_above0, init_empty, md_skip_eq, steal, steal_not_again (the lost partner's bin is outside the maxima and is not subtracted again), steal_entry_decides (the
  lost partners' histogram entries change the three maxima), dist_50, dist_51, init_ratio_eq (rejected), init_ratio_pass (bestDist2 finite, accepted),
  init_single (bestDist2 == INT_MAX), second_eq_best, second_same_lane / second_other_lane (more than 64 candidates; list positions of best and second best are / are
  not congruent mod 64; counted only where every cell of the window holds at most one feature, because then the device's list order is the visiting order --
  inside a cell it is not fixed, the grid is filled with atomics), cand2048

UNREACHABLE lists kinds the classifier counts that no input can reach, with the reason; the CPU test asserts each is 0."""
import numpy as np

TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30
COLS, ROWS = 64, 48
INT_MAX = 2 ** 31 - 1
CAND_CAP, INIT_CAND_CAP, RC = 256, 2048, 12

GRID_KINDS = ("grid_out", "grid_last_col", "clamp_left", "clamp_right", "clamp_top", "clamp_bottom", "win_outside", "win_gt64", "multi_next_empty", "edge_dx", "edge_dy",
              "oct_below", "oct_at_min", "oct_at_max", "oct_above", "level0_query", "ur_reject", "ur_eq", "ur_zero", "ur_neg", "preclaimed_skip",
              "cand12", "cand13", "cand65", "cand256", "cand_over")
GREEDY_KINDS = ("tie_ix", "tie_iy", "tie_feat", "tie_ix_high", "tie_iy_high", "dist_100", "dist_101", "ratio_eq", "ratio_reject", "ratio_level_pass", "single_cand",
                "best_taken", "second_flip", "all_taken", "overwrite", "chain8", "deep1024", "deep2048")
FRAME_KINDS = ("fwd_oct0", "fwd_octpos", "backward", "neither", "mono_large_z", "z_eq_mb", "invz_neg", "out_left", "out_right", "out_top", "out_bottom", "nan_window")
ROT_KINDS = ("rot_wrap", "rot_half", "bin12", "hist_lt3", "max2_tie", "max2_tenth", "max2_drop", "max3_drop", "ori_removed", "ori_overwritten")
INIT_KINDS = ("f1_above0", "init_empty", "md_skip_eq", "steal", "steal_not_again", "steal_entry_decides", "dist_50", "dist_51", "init_ratio_eq", "init_ratio_pass",
              "init_single", "second_eq_best", "second_same_lane", "second_other_lane", "cand2048")
REQUIRED = GRID_KINDS + GREEDY_KINDS + FRAME_KINDS + ROT_KINDS + INIT_KINDS
UNREACHABLE = {
    "bin30": "bin == HISTO_LENGTH: rot is in [0, 360] after the wrap (angles are in [0, 360)), so roundf(rot / 30) <= 12; the reference's `if(bin==HISTO_LENGTH) bin=0`"
             " is dead code with a factor of 1/30",
    "tie_feat_high": "two tied candidates of one cell are visited in ascending feature index, so the lower index always wins inside a cell",
}
ALL_KINDS = REQUIRED + tuple(UNREACHABLE)

f32 = np.float32
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def roundf(x):
    """C roundf of a float: half away from zero (float + 0.5 is exact in double)"""
    x = float(x)
    return f32(np.floor(x + 0.5) if x >= 0 else -np.floor(-x + 0.5))


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def _new_kinds():
    return {k: 0 for k in ALL_KINDS}


def build_grid(F, kinds):
    """Frame::AssignFeaturesToGrid: {(ix, iy): features in ascending index}, and the cell-size inverses"""
    winv = f32(COLS) / (f32(F["max_x"]) - f32(F["min_x"])); hinv = f32(ROWS) / (f32(F["max_y"]) - f32(F["min_y"]))
    cells = {}
    kx, ky = F["keys_un"]["x"].astype(f32), F["keys_un"]["y"].astype(f32)
    for i in range(len(kx)):
        px = int(roundf((kx[i] - f32(F["min_x"])) * winv)); py = int(roundf((ky[i] - f32(F["min_y"])) * hinv))
        if px < 0 or px >= COLS or py < 0 or py >= ROWS:
            kinds["grid_out"] += 1
            continue
        kinds["grid_last_col"] += px == COLS - 1
        cells.setdefault((px, py), []).append(i)
    return dict(cells=cells, winv=winv, hinv=hinv)


def features_in_area(F, G, x, y, r, min_level, max_level, qk):
    """Frame::GetFeaturesInArea: [(feature, ix, iy)] in the reference's visiting order (ix, then iy, then ascending feature index); qk collects the query's kinds"""
    x, y, r = f32(x), f32(y), f32(r)
    if np.isnan(x) or np.isnan(y):
        qk.add("nan_window")
        return []
    mnx, mny = f32(F["min_x"]), f32(F["min_y"])
    a = int(np.floor((x - mnx - r) * G["winv"])); b = int(np.ceil((x - mnx + r) * G["winv"]))
    c = int(np.floor((y - mny - r) * G["hinv"])); d = int(np.ceil((y - mny + r) * G["hinv"]))
    if max(a, 0) >= COLS or min(b, COLS - 1) < 0 or max(c, 0) >= ROWS or min(d, ROWS - 1) < 0:
        qk.add("win_outside")
        return []
    for cond, k in ((a < 0, "clamp_left"), (b > COLS - 1, "clamp_right"), (c < 0, "clamp_top"), (d > ROWS - 1, "clamp_bottom")):
        if cond:
            qk.add(k)
    a, b, c, d = max(a, 0), min(b, COLS - 1), max(c, 0), min(d, ROWS - 1)
    ny = d - c + 1; ncell = (b - a + 1) * ny
    if ncell > 64:
        qk.add("win_gt64")
    check = (min_level > 0) or (max_level >= 0)
    if min_level == -1:
        qk.add("level0_query")
    cells = G["cells"]
    count = lambda lane: len(cells.get((a + lane // ny, c + lane % ny), ()))
    out = []
    kp = F["keys_un"]
    for ix in range(a, b + 1):
        for iy in range(c, d + 1):
            fs = cells.get((ix, iy), ())
            if len(fs) >= 2:
                lane = (ix - a) * ny + (iy - c)
                for nb in (lane - 1, lane + 1):
                    if 0 <= nb < ncell and nb // 64 == lane // 64 and count(nb) == 0:
                        qk.add("multi_next_empty")
            for f in fs:
                o = int(kp["octave"][f])
                if check:
                    if o == min_level - 1 and o >= 0:
                        qk.add("oct_below")
                    if max_level >= 0 and o == max_level + 1:
                        qk.add("oct_above")
                    if o < min_level or (max_level >= 0 and o > max_level):
                        continue
                    if o == min_level:
                        qk.add("oct_at_min")
                    if o == max_level:
                        qk.add("oct_at_max")
                dx = abs(f32(kp["x"][f]) - x); dy = abs(f32(kp["y"][f]) - y)
                if dx == r and dy < r:
                    qk.add("edge_dx")
                if dy == r and dx < r:
                    qk.add("edge_dy")
                if dx < r and dy < r:
                    out.append((f, ix, iy))
    return out


def three_maxima(hist, kinds):
    """ORBmatcher::ComputeThreeMaxima; counts the per-call histogram kinds"""
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(hist):
        if s > max1:
            max3, max2, max1 = max2, max1, s; i3, i2, i1 = i2, i1, i
        elif s > max2:
            max3, max2 = max2, s; i3, i2 = i2, i
        elif s > max3:
            max3 = s; i3 = i
    nz = sum(1 for s in hist if s > 0)
    kinds["hist_lt3"] += 0 < nz < 3
    kinds["max2_tie"] += max1 > 0 and max2 == max1
    kinds["max2_tenth"] += max2 > 0 and f32(max2) == f32(0.1) * f32(max1)
    if f32(max2) < f32(0.1) * f32(max1):
        kinds["max2_drop"] += max2 > 0
        i2 = i3 = -1
    elif f32(max3) < f32(0.1) * f32(max1):
        kinds["max3_drop"] += max3 > 0
        i3 = -1
    return i1, i2, i3


def _rot_bin(a_query, a_feat, qk):
    rot = f32(a_query) - f32(a_feat)
    if rot < 0:
        rot = rot + f32(360.0); qk.add("rot_wrap")
    prod = rot * (f32(1.0) / f32(HISTO_LENGTH))
    if float(prod) - np.floor(float(prod)) == 0.5:
        qk.add("rot_half")
    b = int(roundf(prod))
    if b == HISTO_LENGTH:
        b = 0; qk.add("bin30")
    if b == 12:
        qk.add("bin12")
    return b


def _tie_kinds(elig, best, qk):
    """elig: [(dist, f, ix, iy)] of the candidates that took part; best: the winner's tuple"""
    tied = [e for e in elig if e[0] == best[0] and e[1] != best[1]]
    if not tied:
        return
    run = min(tied, key=lambda e: (e[2], e[3], e[1]))                    # the runner-up in visiting order
    if run[2] != best[2]:
        qk.add("tie_ix"); high = "tie_ix_high"
    elif run[3] != best[3]:
        qk.add("tie_iy"); high = "tie_iy_high"
    else:
        qk.add("tie_feat"); high = "tie_feat_high"
    if any(e[1] < best[1] for e in tied):
        qk.add(high)


def _list_kinds(n, qk, cap):
    for cond, k in ((n == 12, "cand12"), (n == 13, "cand13"), (n > 64, "cand65"), (n == cap, "cand256" if cap == CAND_CAP else "cand2048"), (n > cap, "cand_over")):
        if cond:
            qk.add(k)


def _ur_ok(F, f, ref, r, qk):
    ur = f32(F["u_right"][f])
    if ur > 0:
        er = abs(f32(ref) - ur)
        if er > r:
            qk.add("ur_reject")
            return False
        if er == r:
            qk.add("ur_eq")
    elif ur == 0:
        qk.add("ur_zero")
    else:
        qk.add("ur_neg")
    return True


def _pick2(cands, taken, octave):
    """the reference's best / second-best loop over [(dist, f, ix, iy)] skipping `taken`: (bestDist, bestLevel, bestDist2, bestLevel2, best tuple or None, second feature)"""
    bd, bl, bd2, bl2, best, second = 256, -1, 256, -1, None, -1
    for e in cands:
        if taken[e[1]]:
            continue
        if e[0] < bd:
            bd2, bl2, second = bd, bl, (best[1] if best else -1)
            bd, bl, best = e[0], int(octave[e[1]]), e
        elif e[0] < bd2:
            bd2, bl2, second = e[0], int(octave[e[1]]), e[1]
    return bd, bl, bd2, bl2, best, second


class _Depth:
    """dependency depth of the queries of one call"""
    def __init__(self):
        self.of_feature = {}

    def add(self, feats):
        d = 1 + max([self.of_feature.get(f, 0) for f in feats] or [0])
        for f in feats:
            self.of_feature[f] = max(self.of_feature.get(f, 0), d)
        return d


def _ints(kinds):
    return {k: int(v) for k, v in kinds.items()}


def _flush(kinds, qk):
    for k in qk:
        kinds[k] += 1


def search_map(F, mps, mp_desc, th, nnratio):
    """SearchByProjection(Frame&, MapPoints, th): (match per feature, nmatches, kinds, notes)"""
    kinds = _new_kinds(); G = build_grid(F, kinds)
    n = len(F["keys_un"]); octave = F["keys_un"]["octave"]
    entry = np.asarray(F["claimed"], np.uint8).astype(bool); claimed = entry.copy()
    match = np.full(n, -1, np.int32); nmatches = 0
    scale = np.asarray(F["scale"], f32); nnratio = f32(nnratio); th = f32(th)
    desc = np.asarray(F["desc"], np.uint8).reshape(n, 32); qd = np.asarray(mp_desc, np.uint8).reshape(-1, 32)
    depth = _Depth(); notes = []
    for i in range(len(mps)):
        p = mps[i]
        if not p["valid"]:
            notes.append("invalid"); continue
        qk = set(); lvl = int(p["level"])
        r = f32(2.5) if float(f32(p["view_cos"])) > 0.998 else f32(4.0)
        if float(th) != 1.0:
            r = r * th
        win = r * scale[lvl]
        area = features_in_area(F, G, p["proj_x"], p["proj_y"], win, lvl - 1, lvl, qk)
        lst = []                                                  # the device's list: area + u_right test, claimed candidates included
        for f, ix, iy in area:
            if entry[f]:
                qk.add("preclaimed_skip")
            if _ur_ok(F, f, p["proj_xr"], win, set() if entry[f] else qk):
                lst.append((hamming(qd[i], desc[f]), f, ix, iy))
        if not area:
            notes.append("no candidate"); _flush(kinds, qk); continue
        _list_kinds(len(lst), qk, CAND_CAP)
        if len(lst) == 1:
            qk.add("single_cand")
        d = depth.add([e[1] for e in lst if not entry[e[1]]])
        if d >= 8:
            qk.add("chain8")
        bd, bl, bd2, bl2, best, second = _pick2(lst, claimed, octave)
        hbd, hbl, hbd2, hbl2, hbest, hsecond = _pick2(lst, entry, octave)
        if best is None and any(not entry[e[1]] for e in lst):
            qk.add("all_taken")
        if hbest is not None and claimed[hbest[1]]:
            qk.add("best_taken")
        accept = lambda a, la, b, lb: a <= TH_HIGH and not (la == lb and f32(a) > nnratio * f32(b))
        note = "best %s dist %d level %d, second dist %d level %d" % (best[1] if best else None, bd, bl, bd2, bl2)
        if best is not None:
            _tie_kinds([e for e in lst if not claimed[e[1]]], best, qk)
            if hbest is not None and hbest[1] == best[1] and hsecond != second and accept(bd, bl, bd2, bl2) != accept(hbd, hbl, hbd2, hbl2):
                qk.add("second_flip")
        if bd == TH_HIGH + 1:
            qk.add("dist_101")
        if bd <= TH_HIGH:
            if bl == bl2 and f32(bd) > nnratio * f32(bd2):
                qk.add("ratio_reject"); notes.append(note + ": ratio reject"); _flush(kinds, qk); continue
            if bl == bl2 and f32(bd) == nnratio * f32(bd2):
                qk.add("ratio_eq")
            if bl != bl2 and bd2 < 256 and f32(bd) > nnratio * f32(bd2):
                qk.add("ratio_level_pass")
            if bd == TH_HIGH:
                qk.add("dist_100")
            f = best[1]
            if match[f] >= 0:
                qk.add("overwrite")
            match[f] = i; claimed[f] = bool(p["claims"]); nmatches += 1
            if d >= 2 and len(lst) > RC:
                if 1024 <= i < 2048:
                    qk.add("deep1024")
                if i >= 2048:
                    qk.add("deep2048")
            note += ": matched"
        notes.append(note); _flush(kinds, qk)
    return match, nmatches, _ints(kinds), notes


def _gemm3(A, x, c):
    """(float)(A(3 x 3 of a row-major matrix with 4 columns) * x + c) with double accumulation"""
    out = np.zeros(3, f32)
    for i in range(3):
        s = 0.0
        for k in range(3):
            s += float(A[i][k]) * float(x[k])
        out[i] = f32(s + (float(c[i]) if c is not None else 0.0))
    return out


def motion(Tcw, Tlw, mb, mono):
    """the host rule (ORBmatcher.cc:1480-1491): (forward, backward, tlc.z)"""
    Tcw = np.asarray(Tcw, f32).reshape(4, 4); Tlw = np.asarray(Tlw, f32).reshape(4, 4)
    Rt = [[-Tcw[j][i] for j in range(3)] for i in range(3)]
    twc = _gemm3(Rt, Tcw[:3, 3], None)
    tlc = _gemm3(Tlw, twc, Tlw[:3, 3])
    return bool(tlc[2] > f32(mb) and not mono), bool(-tlc[2] > f32(mb) and not mono), tlc[2]


def search_frame(C, Tcw, Tlw, fx, fy, cx, cy, bf, mb, last, last_desc, th, mono, check_ori):
    """SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono): (match per feature, nmatches, kinds, notes)"""
    kinds = _new_kinds(); G = build_grid(C, kinds)
    n = len(C["keys_un"]); octave = C["keys_un"]["octave"]
    entry = np.asarray(C["claimed"], np.uint8).astype(bool); claimed = entry.copy()
    match = np.full(n, -1, np.int32); nmatches = 0
    scale = np.asarray(C["scale"], f32); th = f32(th)
    desc = np.asarray(C["desc"], np.uint8).reshape(n, 32); qd = np.asarray(last_desc, np.uint8).reshape(-1, 32)
    T = np.asarray(Tcw, f32).reshape(4, 4)
    fwd, bwd, tz = motion(Tcw, Tlw, mb, mono)
    kinds["mono_large_z"] += bool(mono and tz > f32(mb)); kinds["z_eq_mb"] += bool(tz == f32(mb))
    fx, fy, cx, cy, bf = f32(fx), f32(fy), f32(cx), f32(cy), f32(bf)
    events = []; hist = [0] * HISTO_LENGTH
    depth = _Depth(); notes = []
    for i in range(len(last)):
        p = last[i]
        if not p["valid"]:
            notes.append("invalid"); continue
        qk = set()
        x3 = _gemm3(T, p["world"], T[:3, 3])
        with np.errstate(divide="ignore", invalid="ignore"):
            invz = f32(np.float64(1.0) / np.float64(x3[2]))
            if invz < 0:
                kinds["invz_neg"] += 1; notes.append("invzc < 0"); continue
            u = fx * x3[0] * invz + cx; v = fy * x3[1] * invz + cy
        out = None
        for cond, k in ((u < f32(C["min_x"]), "out_left"), (u > f32(C["max_x"]), "out_right")):
            if cond and out is None:
                out = k
        if out is None:
            for cond, k in ((v < f32(C["min_y"]), "out_top"), (v > f32(C["max_y"]), "out_bottom")):
                if cond and out is None:
                    out = k
        if out:
            kinds[out] += 1; notes.append(out); continue
        o = int(p["octave"]); radius = th * scale[o]
        if fwd:
            qk.add("fwd_oct0" if o == 0 else "fwd_octpos"); lv = (o, -1)
        elif bwd:
            qk.add("backward"); lv = (0, o)
        else:
            qk.add("neither"); lv = (o - 1, o + 1)
        area = features_in_area(C, G, u, v, radius, lv[0], lv[1], qk)
        lst = []
        with np.errstate(invalid="ignore"):
            ur_ref = u - bf * invz
        for f, ix, iy in area:
            if entry[f]:
                qk.add("preclaimed_skip")
            if _ur_ok(C, f, ur_ref, radius, set() if entry[f] else qk):
                lst.append((hamming(qd[i], desc[f]), f, ix, iy))
        if not area:
            notes.append("no candidate (u %r, v %r)" % (float(u), float(v))); _flush(kinds, qk); continue
        _list_kinds(len(lst), qk, CAND_CAP)
        if len(lst) == 1:
            qk.add("single_cand")
        d = depth.add([e[1] for e in lst if not entry[e[1]]])
        if d >= 8:
            qk.add("chain8")
        bd, _, _, _, best, _ = _pick2(lst, claimed, octave)
        hbest = _pick2(lst, entry, octave)[4]
        if best is None and any(not entry[e[1]] for e in lst):
            qk.add("all_taken")
        if hbest is not None and claimed[hbest[1]]:
            qk.add("best_taken")
        note = "u %r v %r best %s dist %d" % (float(u), float(v), best[1] if best else None, bd)
        if best is not None:
            _tie_kinds([e for e in lst if not claimed[e[1]]], best, qk)
        if bd == TH_HIGH + 1:
            qk.add("dist_101")
        if bd <= TH_HIGH:
            if bd == TH_HIGH:
                qk.add("dist_100")
            f = best[1]
            if match[f] >= 0:
                qk.add("overwrite")
            match[f] = i; claimed[f] = bool(p["claims"]); nmatches += 1
            if d >= 2 and len(lst) > RC:
                if 1024 <= i < 2048:
                    qk.add("deep1024")
                if i >= 2048:
                    qk.add("deep2048")
            note += ": matched"
            if check_ori:
                b = _rot_bin(p["angle"], C["keys_un"]["angle"][f], qk)
                events.append((f, b, i)); hist[b] += 1
                note += " bin %d" % b
        notes.append(note); _flush(kinds, qk)
    if check_ori:
        i1, i2, i3 = three_maxima(hist, kinds)
        for f, b, i in events:
            if b != i1 and b != i2 and b != i3:
                kinds["ori_removed"] += 1
                kinds["ori_overwritten"] += match[f] >= 0 and match[f] != i
                match[f] = -1; nmatches -= 1
                notes[i] += ", removed by the rotation pass"
    return match, nmatches, _ints(kinds), notes


def search_init(F1, F2, prev_matched, window_size, nnratio, check_ori):
    """SearchForInitialization: (vnMatches12, vbPrevMatched after the call, nmatches, kinds, notes)"""
    kinds = _new_kinds(); G = build_grid(F2, kinds)
    n1, n2 = len(F1["keys_un"]), len(F2["keys_un"])
    pm = np.array(prev_matched, f32, copy=True).reshape(-1, 2)
    d1 = np.asarray(F1["desc"], np.uint8).reshape(n1, 32); d2 = np.asarray(F2["desc"], np.uint8).reshape(n2, 32)
    matched_dist = [INT_MAX] * n2; match21 = [-1] * n2
    match12 = np.full(n1, -1, np.int32); nmatches = 0
    nnratio = f32(nnratio)
    events = []; hist = [0] * HISTO_LENGTH; lost = []
    notes = []
    for i1 in range(n1):
        if F1["keys_un"]["octave"][i1] > 0:
            kinds["f1_above0"] += 1; notes.append("level > 0"); continue
        qk = set()
        area = features_in_area(F2, G, pm[i1, 0], pm[i1, 1], f32(window_size), 0, 0, qk)
        qk.discard("level0_query")
        if not area:
            qk.add("init_empty"); notes.append("no candidate"); _flush(kinds, qk); continue
        _list_kinds(len(area), qk, INIT_CAND_CAP)
        bd, bd2, best, pos, pos2 = INT_MAX, INT_MAX, None, -1, -1
        elig = []
        for j, (f, ix, iy) in enumerate(area):
            dist = hamming(d1[i1], d2[f])
            if matched_dist[f] <= dist:
                if matched_dist[f] == dist:
                    qk.add("md_skip_eq")
                continue
            elig.append((dist, f, ix, iy))
            if dist < bd:
                bd2, pos2 = bd, pos
                bd, best, pos = dist, (dist, f, ix, iy), j
            elif dist < bd2:
                bd2, pos2 = dist, j
        note = "best %s dist %d second %d" % (best[1] if best else None, bd, bd2)
        if best is not None:
            _tie_kinds(elig, best, qk)
            if bd2 == bd:
                qk.add("second_eq_best")
            if len(area) > 64 and bd2 != INT_MAX and len(set((e[1], e[2]) for e in area)) == len(area):       # one feature per cell: the list order is known
                qk.add("second_same_lane" if pos % 64 == pos2 % 64 else "second_other_lane")
        if bd == TH_LOW + 1:
            qk.add("dist_51")
        if bd <= TH_LOW:
            if f32(bd) == f32(bd2) * nnratio:
                qk.add("init_ratio_eq")
            if f32(bd) < f32(bd2) * nnratio:
                qk.add("init_single" if bd2 == INT_MAX else "init_ratio_pass")
                if bd == TH_LOW:
                    qk.add("dist_50")
                f = best[1]
                if match21[f] >= 0:
                    qk.add("steal"); lost.append(match21[f])
                    match12[match21[f]] = -1; nmatches -= 1
                match12[i1] = f; match21[f] = i1; matched_dist[f] = bd; nmatches += 1
                note += ": matched"
                if check_ori:
                    b = _rot_bin(F1["keys_un"]["angle"][i1], F2["keys_un"]["angle"][f], qk)
                    events.append((i1, b)); hist[b] += 1
                    note += " bin %d" % b
        notes.append(note); _flush(kinds, qk)
    if check_ori:
        i1_, i2_, i3_ = three_maxima(hist, kinds)
        for i1, b in events:
            if b != i1_ and b != i2_ and b != i3_:
                if match12[i1] >= 0:
                    match12[i1] = -1; nmatches -= 1; kinds["ori_removed"] += 1
                    notes[i1] += ", removed by the rotation pass"
                elif i1 in lost:
                    kinds["steal_not_again"] += 1
        if lost:                                                  # would the maxima differ without the lost partners' entries?
            h2 = list(hist)
            for i1, b in events:
                if i1 in lost and match12[i1] < 0:
                    h2[b] -= 1
            kinds["steal_entry_decides"] += three_maxima(h2, _new_kinds()) != (i1_, i2_, i3_)
    for i1 in range(n1):
        if match12[i1] >= 0:
            pm[i1, 0] = F2["keys_un"]["x"][match12[i1]]; pm[i1, 1] = F2["keys_un"]["y"][match12[i1]]
    return match12, pm, nmatches, _ints(kinds), notes

"""Small hand-built inputs for the projection matchers (tests/proj_reference.py lists the kinds), the oracle's answer and the restatement's kind counts for each,
computed once per process.  SUPPLIES says which case is there for which kind: test_proj_reference.py asserts every entry on the oracle's data, so a failure names
the input to repair, and test_gpu_proj_kinds.py asserts that the cases it runs cover every required kind by this table.

How the inputs are made exact
  descriptors   a descriptor with k leading bits set; against the all-zero query the Hamming distance is exactly k (two such descriptors are |k1 - k2| apart)
  frame         1241 x 376 from the origin, eight levels of 1.2^l; a cell is 19.39 x 7.83 px.  Coordinates are small integers or quarters, exact in float
  map overload  th = 1, view_cos = 0.9: r = 4 at level 0 (`r *= th` is skipped at th == 1)
  frame overload  fx = fy = 512, cx = 620, cy = 188, bf = 256, mb = 0.5, Tlw = I, Tcw = [I | (0, 0, tz)]: tlc.z = -tz; a world point (X, Y, Z) with Z + tz = 4 projects to
                (128 X + 620, 128 Y + 188) exactly and its stereo coordinate is u - 64
Scenarios of one case sit far enough apart that their windows do not touch.

A case is a dict: kind ("map" / "frame" / "init"), the arguments, and `overflow` where the call must report CORB_ERR_OVERFLOW (the oracle has no cap and answers all the same).

Counts per required kind over all cases, on the oracle's data at the time of writing (the tests only ask for > 0):
  grid_out 5, grid_last_col 5, clamp_left 5, clamp_right 5, clamp_top 6, clamp_bottom 6, win_outside 5, win_gt64 9, multi_next_empty 387, edge_dx 5, edge_dy 8, oct_below 13,
  oct_at_min 218, oct_at_max 239, oct_above 31, level0_query 38, ur_reject 10, ur_eq 10, ur_zero 10, ur_neg 446, preclaimed_skip 7, cand12 24, cand13 26, cand65 143,
  cand256 4, cand_over 3, tie_ix 3, tie_iy 3, tie_feat 6, tie_ix_high 3, tie_iy_high 3, dist_100 4, dist_101 4, ratio_eq 1, ratio_reject 3, ratio_level_pass 110,
  single_cand 119, best_taken 294, second_flip 1, all_taken 11, overwrite 7, chain8 180, deep1024 38, deep2048 22, fwd_oct0 240, fwd_octpos 6, backward 21, neither 30,
  mono_large_z 1, z_eq_mb 1, invz_neg 3, out_left 3, out_right 3, out_top 3, out_bottom 3, nan_window 3, rot_wrap 2, rot_half 2, bin12 1, hist_lt3 8, max2_tie 1,
  max2_tenth 1, max2_drop 2, max3_drop 1, ori_removed 9, ori_overwritten 1, f1_above0 1, init_empty 4, md_skip_eq 1, steal 3, steal_not_again 1, steal_entry_decides 1,
  dist_50 1, dist_51 1, init_ratio_eq 1, init_ratio_pass 5, init_single 22, second_eq_best 4, second_same_lane 1, second_other_lane 1, cand2048 1; unreachable: bin30 0,
  tie_feat_high 0

What a wrong kernel would trip over, by reading proj_kernels.hip (case, kind):
  the spill loops of proj_resolve_kernel starting at PR_RC + 1   map_lists / frame_lists, cand13 (and cand65): the feature at list position 12 is seen by none of the 13 queries
                                          and stays unmatched (from the pick loop), or its query never becomes final (from the feat_min loop); map_deep / frame_chain,
                                          deep1024, for the second register set
  `o1 == o2` dropped from the ratio test  map_ratio query 2, ratio_level_pass: 41 against 80 across levels would be rejected
  the second `feat_min[...] == q` dropped map_ties query 9, second_flip: final in round 1 with the earlier query's feature as second best, 10 against 11 rejected; the
                                          oracle matches it (10 against 40)
  `ur > 0` changed to `ur >= 0`           map_grid query at (300, 50) and frame_forward at (300, 100), ur_zero: |90 - 0| > r would exclude the only candidate
  roundf changed to rintf                 frame_rot query 19 and init_rot query 0, rot_half: bin 0 in place of bin 1 keeps a match the oracle removes
  the winner lane of init_resolve_kernel offering its best   init_lanes query 0, second_same_lane: second best 10 in place of 30, 10 < 9 fails, no match"""
import numpy as np

import proj_reference as R

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
TRACKED_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"), ("level", "<i4"), ("valid", "u1"), ("claims", "u1"), ("pad", "u1", 2)])
LAST_DTYPE = np.dtype([("world", "<f4", 3), ("angle", "<f4"), ("octave", "<i4"), ("valid", "u1"), ("claims", "u1"), ("pad", "u1", 2)])
W, H = 1241.0, 376.0
SCALE = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
FX = FY = 512.0; CX, CY, BF, MB = 620.0, 188.0, 256.0, 0.5


def bits(k):
    """32 bytes with the k leading bits set"""
    b = np.zeros(256, np.uint8); b[:k] = 1
    return np.packbits(b)


class Frame:
    """features of a target frame"""
    def __init__(self):
        self.rows = []

    def feat(self, x, y, k, octave=0, ur=-1.0, claimed=0, angle=0.0):
        self.rows.append((x, y, k, octave, ur, claimed, angle))
        return len(self.rows) - 1

    def view(self):
        n = len(self.rows)
        keys = np.zeros(n, KP_DTYPE); desc = np.zeros((n, 32), np.uint8); ur = np.zeros(n, np.float32); cl = np.zeros(n, np.uint8)
        for i, (x, y, k, o, u, c, a) in enumerate(self.rows):
            keys[i]["x"], keys[i]["y"], keys[i]["octave"], keys[i]["angle"] = x, y, o, a
            desc[i] = bits(k); ur[i] = u; cl[i] = c
        return dict(keys_un=keys, u_right=ur, desc=desc, claimed=cl, min_x=0.0, min_y=0.0, max_x=W, max_y=H, scale=SCALE)


class MapQueries:
    def __init__(self):
        self.rows = []

    def q(self, x, y, level=0, xr=0.0, k=0, valid=1, claims=1, view_cos=0.9):
        self.rows.append((x, y, xr, view_cos, level, valid, claims, k))
        return len(self.rows) - 1

    def pad_to(self, n):
        while len(self.rows) < n:
            self.q(0.0, 0.0, valid=0)

    def view(self):
        m = np.zeros(len(self.rows), TRACKED_DTYPE); d = np.zeros((len(self.rows), 32), np.uint8)
        for i, r in enumerate(self.rows):
            m[i]["proj_x"], m[i]["proj_y"], m[i]["proj_xr"], m[i]["view_cos"], m[i]["level"], m[i]["valid"], m[i]["claims"] = r[:7]
            d[i] = bits(r[7])
        return m, d


def _map(F, Q, th=1.0, nnratio=0.8, overflow=False):
    mps, desc = Q.view()
    return dict(kind="map", frame=F.view(), mps=mps, desc=desc, th=th, nnratio=nnratio, overflow=overflow)


# ---- map overload ----
def map_grid():
    F, Q = Frame(), MapQueries()
    F.feat(1232, 100, 1); F.feat(1230, 100, 5); Q.q(1231, 100)                  # PosInGrid: 1232 is out, 1230 is in column 63; the window is clamped on the right
    F.feat(3, 100, 3); Q.q(2, 100)                                              # clamped on the left
    F.feat(300, 2, 3); Q.q(300, 1)                                              # ... at the top
    F.feat(300, 371, 3); Q.q(300, 374)                                          # ... at the bottom
    Q.q(1300, 100); Q.q(300, 500); Q.q(-50, 100); Q.q(300, -30)                  # wholly outside, on each side
    F.feat(504, 200, 1); F.feat(503.75, 200, 5); Q.q(500, 200)                  # |dx| == r is out, 3.75 is in
    F.feat(600, 204, 1); F.feat(600, 203.75, 5); Q.q(600, 200)                  # |dy| == r
    for o, k in ((1, 1), (2, 9), (3, 8), (4, 2)):                               # octaves min_level - 1 .. max_level + 1 of a level-3 query
        F.feat(700, 200, k, octave=o)
    Q.q(700, 200, level=3)
    F.feat(800, 200, 1, octave=1); F.feat(800, 200, 6, octave=0); Q.q(800, 200)  # level-0 query: octave 1 is above
    # u_right: rejected just above r, accepted at equality, 0 is no stereo value, < 0
    F.feat(100, 50, 1, ur=94.5); F.feat(100, 50, 20, ur=-1.0); Q.q(100, 50, xr=90.0)
    F.feat(200, 50, 1, ur=94.0); Q.q(200, 50, xr=90.0)
    F.feat(300, 50, 1, ur=0.0); Q.q(300, 50, xr=90.0)
    F.feat(400, 50, 1, claimed=1); F.feat(400, 50, 30); Q.q(400, 50)            # claimed on entry
    return _map(F, Q)


def map_wide():
    """th = 8 at level 3: r = 55.3 px, 7 x 16 cells > 64; a cell of several features next to empty cells, lists of more than 64"""
    F, Q = Frame(), MapQueries()
    for j in range(70):
        F.feat(600, 190, 100 - j, octave=2 + j % 2)                             # one cell, the best last
    F.feat(560, 150, 3, octave=3); F.feat(650, 230, 2, octave=2)
    Q.q(600, 190, level=3); Q.q(601, 190, level=3); Q.q(599, 191, level=3)
    return _map(F, Q, th=8.0)


def map_lists():
    """candidate lists of exactly 12, 13, 65 and 256 at one spot each.  The order of a cell's features in the device's list is not fixed (the grid is filled with atomics),
    so which feature sits at list position 12 -- the first one outside the register cache -- is not known: the lists of 12, 13 and 65 are therefore emptied by as many
    claiming queries as they hold features (levels alternate along the distances, so the ratio test never applies), and every feature must end up matched."""
    F, Q = Frame(), MapQueries()
    for x, n in ((100, 12), (200, 13), (300, 65)):
        for j in range(n):
            F.feat(x, 100, n - j, octave=j % 2)
        for j in range(n):
            Q.q(x + (j % 3) - 1, 100, level=1)
    for j in range(256):
        F.feat(400, 100, 90 - j if j >= 254 else 95 + j % 150, octave=j % 2)
    Q.q(400, 100, level=1); Q.q(401, 100, level=1)
    return _map(F, Q)


def map_over():
    F, Q = Frame(), MapQueries()
    for j in range(257):
        F.feat(400, 100, 1 + j % 200)
    Q.q(400, 100)
    return _map(F, Q, overflow=True)


def map_ties():
    F, Q = Frame(), MapQueries()
    # a tie across columns (the column boundary is at x = 126.03) and across rows (y = 97.92): the visiting order wins, not the lower index
    F.feat(128, 100, 3, octave=1); F.feat(124, 100, 3, octave=0); Q.q(126, 100, level=1)
    F.feat(300, 99, 3, octave=1); F.feat(300, 97, 3, octave=0); Q.q(300, 98, level=1)
    F.feat(400, 100, 3, octave=1); F.feat(400, 100, 3, octave=0); Q.q(400, 100, level=1)          # the same cell: the lower index
    F.feat(500, 100, 100); Q.q(500, 100)                                        # TH_HIGH accepted
    F.feat(600, 100, 101); Q.q(600, 100)                                        # 101 rejected
    # the best is taken by an earlier query; then the only candidate left; then all taken
    F.feat(700, 100, 1); F.feat(700, 100, 30, octave=1); Q.q(700, 100, level=1); Q.q(701, 100, level=1); Q.q(699, 100, level=1)
    # the second best is taken by an earlier query, so the ratio test passes: A(799) 11, B(802) 10, C(802) 40
    F.feat(799, 100, 11); F.feat(802, 100, 10); F.feat(802, 100, 40)
    Q.q(797, 100); Q.q(800, 100); Q.q(796, 100)                                 # the first sees A only; the last sees A only, taken
    # a non-claiming query, then one that matches the same feature
    F.feat(900, 100, 7); Q.q(900, 100, claims=0); Q.q(901, 100)
    # a chain of 10 queries over 14 features, levels alternate so that the ratio test never applies; the best ones are last in the list
    for j in range(14):
        F.feat(1000, 100, 5 * (14 - j), octave=j % 2)
    for j in range(10):
        Q.q(1000 + (j % 3) - 1, 100, level=1)
    return _map(F, Q)


def map_ratio():
    """nnratio = 0.5: 40 against 80 at one level is accepted, 41 against 80 is rejected, and accepted when the levels differ"""
    F, Q = Frame(), MapQueries()
    F.feat(100, 100, 40); F.feat(100, 100, 80); Q.q(100, 100)
    F.feat(200, 100, 41); F.feat(200, 100, 80); Q.q(200, 100)
    F.feat(300, 100, 41, octave=1); F.feat(300, 100, 80, octave=0); Q.q(300, 100, level=1)
    return _map(F, Q, nnratio=0.5)


def map_deep():
    """contended queries at indices >= 1024 and >= 2048 (the front is padded with invalid queries), lists of 20, the best ones last"""
    F, Q = Frame(), MapQueries()
    for x in (200, 600):
        for j in range(20):
            F.feat(x, 100, 4 * (20 - j), octave=j % 2)
    Q.pad_to(1030)
    for j in range(20):                                                         # as many claiming queries as features: every feature ends up matched
        Q.q(200 + (j % 3) - 1, 100, level=1)
    Q.pad_to(2060)
    for j in range(12):
        Q.q(600 + (j % 3) - 1, 100, level=1, claims=int(j % 5 != 3))
    return _map(F, Q)


# ---- frame overload ----
class LastPoints:
    def __init__(self, tz):
        self.rows = []; self.tz = tz

    def at(self, u, v, octave=0, k=0, angle=0.0, valid=1, claims=1, zc=4.0):
        """a point that projects to (u, v) at camera depth zc (u - 620 and v - 188 must be multiples of 512 / zc / 2^k)"""
        return self.world((u - CX) * zc / FX, (v - CY) * zc / FY, zc - self.tz, octave, k, angle, valid, claims)

    def world(self, X, Y, Z, octave=0, k=0, angle=0.0, valid=1, claims=1):
        self.rows.append((X, Y, Z, angle, octave, valid, claims, k))
        return len(self.rows) - 1

    def pad_to(self, n):
        while len(self.rows) < n:
            self.world(0, 0, 8, valid=0)

    def view(self):
        m = np.zeros(len(self.rows), LAST_DTYPE); d = np.zeros((len(self.rows), 32), np.uint8)
        for i, r in enumerate(self.rows):
            m[i]["world"] = r[:3]; m[i]["angle"], m[i]["octave"], m[i]["valid"], m[i]["claims"] = r[3:7]
            d[i] = bits(r[7])
        return m, d


def _frame(F, L, th=3.0, mono=0, ori=1, overflow=False):
    last, desc = L.view()
    Tcw = np.eye(4, dtype=np.float32); Tcw[2, 3] = L.tz
    return dict(kind="frame", cur=F.view(), Tcw=Tcw, Tlw=np.eye(4, dtype=np.float32), fx=FX, fy=FY, cx=CX, cy=CY, bf=BF, mb=MB, last=last, desc=desc, th=th, mono=mono,
                ori=ori, overflow=overflow)


def _levels(F, L):
    """octaves around the query's: a query of octave 0 and one of octave 3, each with features at octaves 0 .. 5 whose distance falls with the octave's distance"""
    for u, o in ((300, 0), (500, 3), (700, 1)):
        for fo in range(6):
            F.feat(u, 188, 10 + 7 * abs(fo - o) + fo, octave=fo)
        L.at(u, 188, octave=o); L.at(u, 188, octave=o, k=3); L.at(u + 1, 188, octave=o, k=1)


def _edges(F, L):
    """projections outside each side, behind the camera, at the camera centre; the window edge; u_right"""
    L.at(-20, 188); L.at(1260, 188); L.at(620, -68); L.at(620, 444); L.at(620, 188, zc=-4.0)
    L.world(0, 0, -L.tz)
    F.feat(103, 100, 1); F.feat(102.75, 100, 5); L.at(100, 100)                  # r = th = 3 at octave 0
    F.feat(200, 103, 1); F.feat(200, 102.75, 5); L.at(200, 100)
    F.feat(300, 100, 1, ur=239.5); F.feat(300, 100, 9, ur=239.0); F.feat(300, 100, 12, ur=0.0); L.at(300, 100); L.at(300, 100, k=2); L.at(300, 100, k=1)      # ur_ref = 236
    F.feat(400, 100, 1, claimed=1); F.feat(400, 100, 100); F.feat(400, 100, 101); L.at(400, 100); L.at(400, 100)
    F.feat(2, 100, 4); L.at(1, 100); F.feat(1230, 100, 4); F.feat(1232, 100, 1); L.at(1231, 100)
    F.feat(500, 2, 4); L.at(500, 1); F.feat(500, 371, 4); L.at(500, 374)


def frame_forward():
    F, L = Frame(), LastPoints(-1.0)
    _levels(F, L); _edges(F, L)
    return _frame(F, L)


def frame_backward():
    F, L = Frame(), LastPoints(1.0)
    _levels(F, L); _edges(F, L)
    return _frame(F, L)


def frame_neither():
    """tlc.z == mb exactly: the comparison is strict"""
    F, L = Frame(), LastPoints(-0.5)
    _levels(F, L); _edges(F, L)
    return _frame(F, L)


def frame_mono():
    F, L = Frame(), LastPoints(-8.0)
    _levels(F, L)
    return _frame(F, L, mono=1)


def _pairs(F, L, counts, extra=()):
    """one query and one feature per histogram entry: counts = [(rot, n)], 16 px apart along rows of 60 (u = 108 + 16 j: a multiple of 1/32 at depth 4)"""
    j = 0
    for rot, n in list(counts) + [(r, 1) for r in extra]:
        for _ in range(n):
            u, v = 108 + 16 * (j % 60), 60 + 32 * (j // 60); j += 1
            qa, fa = (rot, 0.0) if rot >= 0 else (10.0, 10.0 - rot)
            F.feat(u, v, 2, angle=fa); L.at(u, v, angle=qa)
    return j


def frame_rot():
    """bin 0 ten times, bin 2 five, bin 3 four; rot = 15 is exactly bin 0.5 -> bin 1 (one entry: removed; rintf would keep it in bin 0); rot = -10 wraps to 350 = bin 12 (removed)"""
    F, L = Frame(), LastPoints(-1.0)
    _pairs(F, L, [(0.0, 10), (60.0, 5), (90.0, 4)], extra=(15.0, -10.0))
    return _frame(F, L)


def frame_hist_tenth():
    """10 and 1: max2 is exactly a tenth and kept; two non-empty bins"""
    F, L = Frame(), LastPoints(-1.0)
    _pairs(F, L, [(30.0, 10), (120.0, 1)])
    return _frame(F, L)


def frame_hist_eleventh():
    """11 and 1: max2 dropped, its match removed"""
    F, L = Frame(), LastPoints(-1.0)
    _pairs(F, L, [(30.0, 11), (120.0, 1)])
    return _frame(F, L)


def frame_hist_ties():
    """3, 3, 2, 2, 1: max2 ties max1 (the earlier bin stays first), a tie for the third place (the earlier bin keeps it)"""
    F, L = Frame(), LastPoints(-1.0)
    _pairs(F, L, [(150.0, 3), (60.0, 3), (240.0, 2), (90.0, 2), (300.0, 1)])
    return _frame(F, L)


def frame_hist_max3():
    """20, 5, 1: max3 dropped alone; and a feature removed through the entry of an overwritten query: a non-claiming query in a bad bin, then a claiming one in a good bin"""
    F, L = Frame(), LastPoints(-1.0)
    j = _pairs(F, L, [(30.0, 20), (120.0, 5), (210.0, 1)])
    u, v = 108 + 16 * j, 60
    F.feat(u, v, 2, angle=0.0); L.at(u, v, angle=270.0, claims=0); L.at(u, v, angle=30.0)
    return _frame(F, L)


def frame_chain():
    """greedy kinds of the frame overload: ties across columns and rows, a taken best, all taken, an overwrite, a chain of depth >= 8 and contended queries at indices
    >= 1024 and >= 2048 with lists of 20 (no orientation test)"""
    F, L = Frame(), LastPoints(-1.0)
    F.feat(128, 100, 3); F.feat(124, 100, 3); L.at(126, 100)
    F.feat(300, 99, 3); F.feat(300, 97, 3); L.at(300, 98)
    F.feat(400, 100, 3); F.feat(400, 100, 3); L.at(400, 100); L.at(400, 100); L.at(400, 100)
    F.feat(500, 100, 7); L.at(500, 100, claims=0); L.at(500, 100)
    for x in (600, 800, 1000):
        for j in range(20):
            F.feat(x, 100, 4 * (20 - j), octave=j % 2)
    for j in range(10):
        L.at(600 + (j % 3) - 1, 100)
    L.pad_to(1030)
    for j in range(20):
        L.at(800 + (j % 3) - 1, 100)
    L.pad_to(2060)
    for j in range(12):
        L.at(1000 + (j % 3) - 1, 100, claims=int(j % 5 != 3))
    return _frame(F, L, ori=0)


def frame_lists():
    """lists of 12, 13, 65 and 256 through the frame overload (th = 3); the first three are emptied by as many claiming queries (see map_lists)"""
    F, L = Frame(), LastPoints(-1.0)
    for x, n in ((100, 12), (200, 13), (300, 65)):
        for j in range(n):
            F.feat(x, 100, n - j)
        for j in range(n):
            L.at(x + (j % 3) - 1, 100)
    for j in range(256):
        F.feat(400, 100, 90 - j if j >= 254 else 95 + j % 150)
    L.at(400, 100); L.at(401, 100)
    return _frame(F, L, ori=0)


def frame_over():
    F, L = Frame(), LastPoints(-1.0)
    for j in range(257):
        F.feat(400, 100, 1 + j % 200)
    L.at(400, 100)
    return _frame(F, L, overflow=True)


# ---- initialisation ----
class InitQueries:
    def __init__(self):
        self.rows = []

    def q(self, x, y, k=0, octave=0, angle=0.0):
        self.rows.append((x, y, k, octave, angle))
        return len(self.rows) - 1

    def view(self):
        n = len(self.rows)
        keys = np.zeros(n, KP_DTYPE); desc = np.zeros((n, 32), np.uint8); pm = np.zeros((n, 2), np.float32)
        for i, (x, y, k, o, a) in enumerate(self.rows):
            keys[i]["x"], keys[i]["y"], keys[i]["octave"], keys[i]["angle"] = x, y, o, a
            desc[i] = bits(k); pm[i] = (x, y)
        return dict(keys_un=keys, desc=desc, min_x=0.0, min_y=0.0, max_x=W, max_y=H, scale=SCALE), pm


def _init(F2, Q, win=10, ratio=0.9, ori=1, overflow=False):
    f1, pm = Q.view()
    f2 = F2.view(); del f2["claimed"]; del f2["u_right"]
    return dict(kind="init", f1=f1, f2=f2, pm=pm, win=win, ratio=ratio, ori=ori, overflow=overflow)


def init_basic():
    """nnratio = 0.5, window 10, scenarios 40 px apart"""
    F, Q = Frame(), InitQueries()
    F.feat(100, 100, 50); Q.q(100, 100)                                         # TH_LOW accepted, one candidate: bestDist2 == INT_MAX
    F.feat(140, 100, 51); Q.q(140, 100)                                         # 51 rejected
    F.feat(180, 100, 40); F.feat(181, 100, 80); Q.q(180, 100)                   # 40 < 80 * 0.5 is false: rejected
    F.feat(220, 100, 39); F.feat(221, 100, 80); Q.q(220, 100)                   # accepted
    F.feat(260, 100, 20); F.feat(261, 100, 20); Q.q(260, 100)                   # the second best equals the best
    F.feat(300, 100, 5); Q.q(300, 100, octave=1)                                # F1 above level 0
    F.feat(340, 100, 5, octave=1); F.feat(341, 100, 30); Q.q(340, 100)          # F2 above level 0: excluded, the other is taken
    Q.q(380, 100); Q.q(1300, 100)                                               # an empty list; a window outside the grid
    F.feat(420, 100, 20); F.feat(421, 100, 45); Q.q(420, 100); Q.q(420, 101)    # vMatchedDistance <= dist at equality: the second query falls to the other feature
    F.feat(460, 100, 30); Q.q(460, 100); Q.q(460, 101, k=20)                    # a steal: 30, then 10
    F.feat(510, 100, 3); Q.q(500, 100); F.feat(540, 110, 3); Q.q(540, 100)      # |dx| == window, |dy| == window: excluded
    F.feat(2, 200, 4); Q.q(1, 200); F.feat(1230, 200, 4); F.feat(1232, 200, 1); Q.q(1231, 200); F.feat(600, 2, 4); Q.q(600, 1); F.feat(600, 371, 4); Q.q(600, 374)
    return _init(F, Q, ratio=0.5, ori=0)


def _one_per_cell(F, centre_x, dists):
    """len(dists) level-0 features, one per grid cell, in the visiting order of a window around (centre_x, 180): columns px(centre_x) - 1 .. + 1, rows 12 .. 35.  With one
    feature per cell the device's list order is the visiting order, so list positions (and the lanes of init_resolve_kernel, position mod 64) are known."""
    col = int(round(centre_x * 64 / W))
    cells = [(ix, iy) for ix in (col - 1, col, col + 1) for iy in range(12, 36)]
    for (ix, iy), k in zip(cells, dists):
        F.feat(ix * (W / 64), iy * (H / 48) + 0.5, k)


def init_lanes():
    """70 candidates, one per cell: best and second best 64 list positions apart (one lane of the device), and in different lanes; ties across cells"""
    F, Q = Frame(), InitQueries()
    _one_per_cell(F, 300, [10 if j == 3 else 30 if j == 67 else 100 + j for j in range(70)])
    Q.q(300, 180)
    _one_per_cell(F, 900, [10 if j == 3 else 30 if j == 10 else 100 + j for j in range(70)])
    Q.q(900, 180)
    F.feat(600, 20.5, 3); F.feat(600, 18.5, 3); Q.q(600, 19.5)                  # ties for the best: rows 3 and 2 (rejected by the ratio test all the same)
    F.feat(620, 360, 3); F.feat(600, 360, 3); Q.q(610, 360)                     # ... and columns
    return _init(F, Q, win=100, ratio=0.9, ori=0)


def init_rot():
    """rotation pass of the initialiser: 11 in bin 1 of which one is a lost partner, 1 in bin 4: with the lost partner's entry max2 = 1 < 0.1f * 11 is dropped and the
    bin-4 match removed; without the entry 1 of 10 would be kept.  A second lost partner sits in bin 8 (outside the maxima) and is not subtracted again.  rot = 15
    (bin 1, exactly on the half) and a wrapped rot (-330 + 360 = 30, bin 1) are among the ten."""
    F, Q = Frame(), InitQueries()
    for j in range(7):
        F.feat(100 + 40 * j, 100, 5, angle=0.0); Q.q(100 + 40 * j, 100, angle=30.0 if j else 15.0)
    F.feat(500, 100, 5, angle=340.0); Q.q(500, 100, angle=10.0)                 # rot = -330, wrapped to 30
    F.feat(540, 100, 30, angle=0.0); Q.q(540, 100, angle=30.0); Q.q(540, 101, k=25, angle=30.0)    # the first is a lost partner in bin 1 (10 entries + its own)
    F.feat(620, 100, 5, angle=0.0); Q.q(620, 100, angle=120.0)                  # bin 4: removed
    F.feat(700, 100, 30, angle=0.0); Q.q(700, 100, angle=240.0); Q.q(700, 101, k=25, angle=30.0)   # a lost partner in bin 8
    return _init(F, Q, ratio=0.9, ori=1)


def init_2048():
    """exactly 2048 level-0 candidates in one window (and a level-1 feature that does not count)"""
    F, Q = Frame(), InitQueries()
    for j in range(2048):
        F.feat(600 + (j % 8), 180 + (j // 8) % 8, 12 if j == 1999 else 60 + j % 150)
    F.feat(600, 180, 1, octave=1)
    Q.q(604, 184)
    return _init(F, Q, win=100, ratio=0.9, ori=1)


def init_over():
    F, Q = Frame(), InitQueries()
    for j in range(2049):
        F.feat(600 + (j % 8), 180 + (j // 8) % 8, 60 + j % 150)
    Q.q(604, 184)
    return _init(F, Q, win=100, overflow=True)


BUILDERS = dict(map_grid=map_grid, map_wide=map_wide, map_lists=map_lists, map_ties=map_ties, map_ratio=map_ratio, map_deep=map_deep, map_over=map_over,
                frame_forward=frame_forward, frame_backward=frame_backward, frame_neither=frame_neither, frame_mono=frame_mono, frame_rot=frame_rot,
                frame_hist_tenth=frame_hist_tenth, frame_hist_eleventh=frame_hist_eleventh, frame_hist_ties=frame_hist_ties, frame_hist_max3=frame_hist_max3,
                frame_chain=frame_chain, frame_lists=frame_lists, frame_over=frame_over,
                init_basic=init_basic, init_lanes=init_lanes, init_rot=init_rot, init_2048=init_2048, init_over=init_over)

# case -> the kinds it is there for
SUPPLIES = {
    "map_grid": ("grid_out", "grid_last_col", "clamp_left", "clamp_right", "clamp_top", "clamp_bottom", "win_outside", "edge_dx", "edge_dy", "oct_below", "oct_at_min",
                 "oct_at_max", "oct_above", "level0_query", "ur_reject", "ur_eq", "ur_zero", "ur_neg", "preclaimed_skip", "single_cand"),
    "map_wide": ("win_gt64", "multi_next_empty", "cand65", "best_taken"),
    "map_lists": ("cand12", "cand13", "cand65", "cand256", "best_taken"),
    "map_ties": ("tie_ix", "tie_iy", "tie_feat", "tie_ix_high", "tie_iy_high", "dist_100", "dist_101", "single_cand", "best_taken", "second_flip", "all_taken", "overwrite",
                 "chain8"),
    "map_ratio": ("ratio_eq", "ratio_reject", "ratio_level_pass"),
    "map_deep": ("deep1024", "deep2048", "chain8", "overwrite"),
    "map_over": ("cand_over",),
    "frame_forward": ("fwd_oct0", "fwd_octpos", "invz_neg", "out_left", "out_right", "out_top", "out_bottom", "nan_window", "edge_dx", "edge_dy", "ur_reject", "ur_eq",
                      "ur_zero", "preclaimed_skip", "dist_100", "dist_101", "clamp_left", "clamp_right", "clamp_top", "clamp_bottom", "grid_out", "oct_below", "oct_at_min"),
    "frame_backward": ("backward", "oct_at_max", "oct_above", "nan_window"),
    "frame_neither": ("neither", "z_eq_mb", "oct_below", "oct_at_min", "oct_at_max", "oct_above"),
    "frame_mono": ("neither", "mono_large_z"),
    "frame_rot": ("rot_wrap", "rot_half", "bin12", "ori_removed"),
    "frame_hist_tenth": ("hist_lt3", "max2_tenth"),
    "frame_hist_eleventh": ("hist_lt3", "max2_drop", "ori_removed"),
    "frame_hist_ties": ("max2_tie", "ori_removed"),
    "frame_hist_max3": ("max3_drop", "ori_removed", "ori_overwritten", "overwrite"),
    "frame_chain": ("tie_ix", "tie_iy", "tie_feat", "tie_ix_high", "tie_iy_high", "best_taken", "all_taken", "overwrite", "chain8", "deep1024", "deep2048"),
    "frame_lists": ("cand12", "cand13", "cand65", "cand256"),
    "frame_over": ("cand_over",),
    "init_basic": ("dist_50", "dist_51", "init_ratio_eq", "init_ratio_pass", "init_single", "second_eq_best", "f1_above0", "oct_above", "init_empty", "win_outside",
                   "md_skip_eq", "steal", "edge_dx", "edge_dy", "clamp_left", "clamp_right", "clamp_top", "clamp_bottom", "grid_out"),
    "init_lanes": ("cand65", "second_same_lane", "second_other_lane", "tie_ix", "tie_iy", "tie_ix_high", "tie_iy_high", "second_eq_best"),
    "init_rot": ("steal", "steal_not_again", "steal_entry_decides", "max2_drop", "ori_removed", "rot_half", "rot_wrap"),
    "init_2048": ("cand2048", "win_gt64", "oct_above"),
    "init_over": ("cand_over",),
}
CASES = list(SUPPLIES)
assert sorted(CASES) == sorted(BUILDERS)

_built, _oracle, _restated = {}, {}, {}


def build(case):
    """the case's arguments; built once, callers must not modify them"""
    if case not in _built:
        _built[case] = BUILDERS[case]()
    return _built[case]


def oracle_call(pyorc, c):
    """pyorc on the arguments of a case: (match, count) or (match12, prev_matched, count)"""
    if c["kind"] == "map":
        return pyorc.search_by_projection_map(c["frame"], c["mps"], c["desc"], c["th"], c["nnratio"])
    if c["kind"] == "frame":
        return pyorc.search_by_projection_frame(c["cur"], c["Tcw"], c["Tlw"], c["fx"], c["fy"], c["cx"], c["cy"], c["bf"], c["mb"], c["last"], c["desc"], c["th"],
                                                c["mono"], c["ori"])
    return pyorc.search_for_initialization(c["f1"], c["f2"], c["pm"], c["win"], c["ratio"], bool(c["ori"]))


def restate_call(c):
    """the restatement on the arguments of a case: the same tuple, then kinds and notes"""
    if c["kind"] == "map":
        return R.search_map(c["frame"], c["mps"], c["desc"], c["th"], c["nnratio"])
    if c["kind"] == "frame":
        return R.search_frame(c["cur"], c["Tcw"], c["Tlw"], c["fx"], c["fy"], c["cx"], c["cy"], c["bf"], c["mb"], c["last"], c["desc"], c["th"], c["mono"], c["ori"])
    return R.search_init(c["f1"], c["f2"], c["pm"], c["win"], c["ratio"], c["ori"])


def device_call(corb, c):
    """the library on the arguments of a case: the same tuple as oracle_call"""
    if c["kind"] == "map":
        return corb.ORBmatcher(c["nnratio"], True).SearchByProjection(c["frame"], c["mps"], c["desc"], c["th"])
    if c["kind"] == "frame":
        return corb.ORBmatcher(0.9, bool(c["ori"])).SearchByProjection_Frame(c["cur"], c["Tcw"], c["Tlw"], c["fx"], c["fy"], c["cx"], c["cy"], c["bf"], c["mb"], c["last"],
                                                                             c["desc"], c["th"], c["mono"])
    return corb.ORBmatcher(c["ratio"], bool(c["ori"])).SearchForInitialization(c["f1"], c["f2"], c["pm"], c["win"])


def as_bytes(result):
    return tuple(np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else int(x) for x in result)


def oracle(pyorc, case):
    if case not in _oracle:
        _oracle[case] = oracle_call(pyorc, build(case))
    return _oracle[case]


def restated(case):
    if case not in _restated:
        _restated[case] = restate_call(build(case))
    return _restated[case]


def describe(case):
    return "case '%s' (%s; there for: %s)" % (case, build(case)["kind"], ", ".join(SUPPLIES[case]))

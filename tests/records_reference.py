"""What a device-resident record means to the reference, in plain numpy: the flat views the oracle's matchers and optimisers take, and the record contents the
reference's code leaves behind, both derived from per-feature arrays (keys, u_right, descriptors, MapPoint ids, flag bytes), map-point records with their
observation lists, and the id -> slot relation as a Python dict.  Written from the reference's source (C/src = corbslam_client/src), one pointer-level test per
line reference; it shares no code with the kernels that gather the same views on the device.

A feature of a frame record holds a MapPoint pointer when its id is not NO_MAP_POINT and its DISCARDED bit is clear: "Discard outliers" sets
mvpMapPoints[i] = NULL and keeps the id only as the point's mnLastFrameSeen (Tracking.cc:919-940).  A pointer the map cannot resolve (an id that is not in the
store) gives no position and no descriptor; where the reference only tests the pointer for NULL (sAlreadyFound, `if(CurrentFrame.mvpMapPoints[i2]) continue;`)
such an id still counts."""
import numpy as np

NO_MAP_POINT = 0xFFFFFFFFFFFFFFFF
NONE = np.uint64(NO_MAP_POINT)
HAS_MP, OUTLIER, DISCARDED = 1, 2, 4                  # flag bits of a frame record's feature (mvbOutlier; discarded as an outlier)
MP_BAD = 1                                            # MapPoint::isBad()
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
LAST_DTYPE = np.dtype([("world", "<f4", 3), ("angle", "<f4"), ("octave", "<i4"), ("valid", "u1"), ("claims", "u1"), ("pad", "u1", 2)])
MP_DTYPE = np.dtype([("world", "<f4", 3), ("normal", "<f4", 3), ("min_distance", "<f4"), ("max_distance", "<f4"), ("angle", "<f4"), ("valid", "u1"), ("pad", "u1", 3)])
MP_RECORD_DTYPE = np.dtype([("id", "<u8"), ("ref_kf_id", "<u8"), ("descriptor", "u1", 32), ("client_id", "<i4"), ("n_obs", "<i4"), ("flags", "<u4"), ("world_pos", "<f4", 3),
                            ("normal", "<f4", 3), ("min_distance", "<f4"), ("max_distance", "<f4"), ("pos_gba", "<f4", 3), ("ba_global_for_kf", "<u8")], align=True)


def slot_dict(rec):
    """the id -> slot relation of records stored from slot 0 on"""
    return {int(i): s for s, i in enumerate(rec["id"])}


def slots_of(ids, slot_of):
    """slot of every id, -1 for NULL and for ids the map does not know"""
    return np.array([-1 if int(i) == NO_MAP_POINT else slot_of.get(int(i), -1) for i in np.asarray(ids, np.uint64)], np.int64)


def held_ids(mp_id, flags):
    """mvpMapPoints as ids: NULL where the feature's point was discarded"""
    return np.where((np.asarray(flags) & DISCARDED) != 0, NONE, np.asarray(mp_id, np.uint64))


def _known(mp_id, flags, slot_of):
    s = slots_of(held_ids(mp_id, flags), slot_of)
    return s, s >= 0


def _pick(rec, field, s, ok):
    """rec[field][s] where ok, zero elsewhere"""
    v = rec[field][np.maximum(s, 0)]
    return np.where(ok.reshape((-1,) + (1,) * (v.ndim - 1)), v, 0).astype(v.dtype)


def _mp_view(rec, s, ok, angle=None):
    v = np.zeros(len(s), MP_DTYPE)
    v["world"] = _pick(rec, "world_pos", s, ok); v["normal"] = _pick(rec, "normal", s, ok)
    v["min_distance"] = _pick(rec, "min_distance", s, ok); v["max_distance"] = _pick(rec, "max_distance", s, ok)
    if angle is not None:
        v["angle"] = np.where(ok, angle, 0)
    v["valid"] = ok
    return v, _pick(rec, "descriptor", s, ok)


def _claimed(mp_id, flags, rec, slot_of):
    """`if(CurrentFrame.mvpMapPoints[i2]) if(...->Observations()>0) continue;` (ORBmatcher.cc:1545-1547, :98-100): isBad() is not asked"""
    s, ok = _known(mp_id, flags, slot_of)
    return (ok & (rec["n_obs"][np.maximum(s, 0)] > 0)).astype(np.uint8)


# ---- tracking thread ----
def last_frame_view(last_keys, last_mp_id, last_flags, cur_mp_id, cur_flags, rec, slot_of):
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono): `MapPoint* pMP = LastFrame.mvpMapPoints[i]; if(pMP) if(!LastFrame.mvbOutlier[i])`
    (ORBmatcher.cc:1496-1500) -- a discarded, outlier, bad or unknown point is no MapPoint.  Returns (LAST_DTYPE rows, query descriptors, claimed of the
    current frame (:1545-1547))."""
    s, ok = _known(last_mp_id, last_flags, slot_of)
    ok = ok & ((rec["flags"][np.maximum(s, 0)] & MP_BAD) == 0) & ((np.asarray(last_flags) & OUTLIER) == 0)
    v = np.zeros(len(s), LAST_DTYPE)
    v["world"] = _pick(rec, "world_pos", s, ok); v["angle"] = last_keys["angle"]; v["octave"] = last_keys["octave"]
    v["valid"] = ok; v["claims"] = ok & (rec["n_obs"][np.maximum(s, 0)] > 0)
    return v, _pick(rec, "descriptor", s, ok), _claimed(cur_mp_id, cur_flags, rec, slot_of)


def matched_writes(mp_id, flags, match, source_ids):
    """`CurrentFrame.mvpMapPoints[bestIdx2] = pMP` (ORBmatcher.cc:1582, :1692, :122): the matched feature holds the point, which is neither an outlier nor discarded"""
    ids = np.array(mp_id, np.uint64, copy=True); fl = np.array(flags, np.uint8, copy=True)
    m = np.asarray(match) >= 0
    ids[m] = np.asarray(source_ids, np.uint64)[np.asarray(match)[m]]
    fl[m] &= np.uint8(0xFF ^ (OUTLIER | DISCARDED))
    return ids, fl


def pose_edges(keys, u_right, mp_id, flags, rec, slot_of, inv_level_sigma2):
    """Optimizer::PoseOptimization (Optimizer.cc:300-366): for i = 0 .. N-1, `if(pMP)` adds one edge -- monocular where mvuRight[i] < 0 (:310), stereo
    otherwise -- with the point's position, the observation (x, y[, u_right]) and invSigma2 of the keypoint's octave.  Bad points have left the frame before
    the call (Tracking.cc:1176-1179).  Returns dict(feat, points, obs, w, mono, klass): klass 0 for fewer than 3 edges (`return 0`, :369-370), 1 for fewer
    than 10 (one round, :470-471), else 4."""
    s, ok = _known(mp_id, flags, slot_of)
    ok = ok & ((rec["flags"][np.maximum(s, 0)] & MP_BAD) == 0)
    feat = np.nonzero(ok)[0]
    ur = np.asarray(u_right, np.float32)[feat]
    obs = np.stack([keys["x"][feat], keys["y"][feat], ur], 1).astype(np.float32).reshape(-1, 3)
    E = len(feat)
    return dict(feat=feat, points=rec["world_pos"][s[feat]].reshape(-1, 3), obs=obs, w=np.asarray(inv_level_sigma2, np.float32)[keys["octave"][feat]],
                mono=ur < 0, klass=0 if E < 3 else 1 if E < 10 else 4)


def pose_writes(flags, feat, rejected, discard):
    """mvbOutlier after PoseOptimization: false for every feature that carries an edge (:318, :345), true for the rejected ones (:422-440); with "Discard outliers"
    (Tracking.cc:919-940) a rejected feature loses its point and its outlier mark instead.  mvbOutlier is only ever read next to a non-NULL pointer, so for
    features without an edge the record keeps it cleared."""
    fl = np.array(flags, np.uint8, copy=True) & np.uint8(0xFF ^ OUTLIER)
    fl[np.asarray(feat)[np.asarray(rejected, bool)]] |= np.uint8(DISCARDED if discard else OUTLIER)
    return fl


def seen_in_frame(cur_mp_id, cur_flags, rec, slot_of):
    """the ids whose mnLastFrameSeen is this frame after the first loop of SearchLocalPoints: held points that are not bad, and points discarded as outliers in
    this frame (Tracking.cc:933, :1183); ids the map does not know name no MapPoint"""
    cur_mp_id = np.asarray(cur_mp_id, np.uint64)
    s = slots_of(cur_mp_id, slot_of)
    bad = (s >= 0) & ((rec["flags"][np.maximum(s, 0)] & MP_BAD) != 0)
    return {int(i) for i in cur_mp_id[(s >= 0) & (((np.asarray(cur_flags, np.uint8) & DISCARDED) != 0) | ~bad)]}


def local_points_view(cur_mp_id, cur_flags, local_ids, rec, slot_of):
    """The first loop of Tracking::SearchLocalPoints (Tracking.cc:1171-1187): a bad point leaves the frame (*vit = NULL), every other held point is seen in this
    frame (mnLastFrameSeen) -- and so is a point discarded as an outlier earlier in this frame (:933).  Returns (mvpMapPoints after the loop as ids, candidate
    mask over local_ids for isInFrustum (`mnLastFrameSeen == mCurrentFrame.mnId` and `isBad()` skip, :1194-1197), claimed per feature)."""
    cur_mp_id = np.asarray(cur_mp_id, np.uint64); cur_flags = np.asarray(cur_flags, np.uint8)
    disc = (cur_flags & DISCARDED) != 0
    s = slots_of(cur_mp_id, slot_of)                                  # (the id of a discarded feature is still the point's mnLastFrameSeen)
    bad = (s >= 0) & ((rec["flags"][np.maximum(s, 0)] & MP_BAD) != 0)
    after = np.where(bad & ~disc, NONE, cur_mp_id)
    seen = seen_in_frame(cur_mp_id, cur_flags, rec, slot_of)
    ls = slots_of(local_ids, slot_of)
    cand = (ls >= 0) & ((rec["flags"][np.maximum(ls, 0)] & MP_BAD) == 0) & np.array([int(i) not in seen for i in np.asarray(local_ids, np.uint64)], bool).reshape(len(ls))
    claimed = ((s >= 0) & ~disc & ~bad & (rec["n_obs"][np.maximum(s, 0)] > 0)).astype(np.uint8)
    return after, cand, claimed


# ---- keyframe matchers ----
def reloc_view(kf_keys, kf_mp_id, frame_mp_id, frame_flags, rec, slot_of):
    """SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist): `if(pMP) if(!pMP->isBad() && !sAlreadyFound.count(pMP))` (ORBmatcher.cc:1634-1639) with
    sAlreadyFound = the pointers the frame holds (Tracking.cc:1440-1500), known to the map or not; `if(CurrentFrame.mvpMapPoints[i2]) continue;` (:1680).
    Returns (MP_DTYPE view of pKF's points with pKF->mvKeysUn[i].angle (:1699), descriptors, claimed of the frame)."""
    h = held_ids(frame_mp_id, frame_flags)
    found = {int(i) for i in h if int(i) != NO_MAP_POINT}
    s = slots_of(kf_mp_id, slot_of)
    ok = (s >= 0) & ((rec["flags"][np.maximum(s, 0)] & MP_BAD) == 0) & np.array([int(i) not in found for i in np.asarray(kf_mp_id, np.uint64)], bool).reshape(len(s))
    v, d = _mp_view(rec, s, ok, kf_keys["angle"])
    return v, d, (h != NONE).astype(np.uint8)


def scw_view(matched_ids, mp_slots, rec):
    """SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th): spAlreadyFound = set(vpMatched) minus NULL (ORBmatcher.cc:441-442); `if(pMP->isBad() ||
    spAlreadyFound.count(pMP)) continue;` (:452); `if(vpMatched[idx]) continue;` (:510).  Returns (view of vpPoints in call order, descriptors, claimed)."""
    matched_ids = np.asarray(matched_ids, np.uint64)
    found = {int(i) for i in matched_ids if int(i) != NO_MAP_POINT}
    s = np.asarray(mp_slots, np.int64)
    ok = ((rec["flags"][s] & MP_BAD) == 0) & np.array([int(i) not in found for i in rec["id"][s]], bool).reshape(len(s))
    v, d = _mp_view(rec, s, ok)
    return v, d, (matched_ids != NONE).astype(np.uint8)


def index_in_keyframe(obs, kf_id):
    """MapPoint::GetIndexInKeyFrame: mObservations[pKF] or -1; obs = [(keyframe id, feature index)]"""
    for k, i in obs:
        if int(k) == int(kf_id):
            return int(i)
    return -1


def sim3_views(ids1, ids2, matched12_ids, rec, slot_of, obs_lists, kf2_id):
    """SearchBySim3: vbAlreadyMatched1[i] = vpMatches12[i] != NULL, vbAlreadyMatched2[idx2] for idx2 = pMP->GetIndexInKeyFrame(pKF2) with 0 <= idx2 < N2
    (ORBmatcher.cc:1270-1283); `if(!pMP || vbAlreadyMatched1[i1]) continue; if(pMP->isBad()) continue;` (:1291-1296, :1371-1376).  obs_lists[slot] = the
    observation list of the map point in that slot.  Returns ((view1, desc1), (view2, desc2))."""
    n1, n2 = len(ids1), len(ids2)
    al1 = np.zeros(n1, bool); al2 = np.zeros(n2, bool)
    if matched12_ids is not None:
        m = np.asarray(matched12_ids, np.uint64)
        al1 = m != NONE
        for s in slots_of(m, slot_of):
            if s >= 0:
                j = index_in_keyframe(obs_lists[s], kf2_id)
                if 0 <= j < n2:
                    al2[j] = True
    out = []
    for ids, al in ((ids1, al1), (ids2, al2)):
        s = slots_of(ids, slot_of)
        ok = (s >= 0) & ~al & ((rec["flags"][np.maximum(s, 0)] & MP_BAD) == 0)
        out.append(_mp_view(rec, s, ok))
    return out[0], out[1]


def fuse_view(mp_slots, rec, obs_lists, kf_id):
    """Fuse(pKF, vpMapPoints, th): `if(pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;` (ORBmatcher.cc:990-993)"""
    s = np.asarray(mp_slots, np.int64)
    ok = ((rec["flags"][s] & MP_BAD) == 0) & np.array([index_in_keyframe(obs_lists[int(k)], kf_id) < 0 for k in s], bool).reshape(len(s))
    return _mp_view(rec, s, ok)


def fuse_writes(best_idx, held, point_ids, obs_lists, kf_id):
    """The map update of Fuse, sequentially (ORBmatcher.cc:1083-1104): a fused point whose feature holds no MapPoint enters it (pMP->AddObservation(pKF, bestIdx);
    pKF->AddMapPoint(pMP, bestIdx)) -- action 1, its list stays ascending in the keyframe id; one whose feature holds a MapPoint by then ends in Replace -- action 2.
    Returns (mvpMapPoints of pKF after, action per point, observation lists after)."""
    mp = np.array(held, np.uint64, copy=True); n = len(best_idx)
    act = np.zeros(n, np.uint8); lists = [list(l) for l in obs_lists]
    for i in range(n):
        f = int(best_idx[i])
        if f < 0:
            continue
        if mp[f] != NONE:
            act[i] = 2
        else:
            act[i] = 1; mp[f] = np.uint64(point_ids[i]); lists[i] = sorted(lists[i] + [(kf_id, f)])
    return mp, act, lists


# ---- id generators ----
_M64 = (1 << 64) - 1


def id_hash(k):
    """the 64-bit finaliser the id tables of device_util.h hash with (restated; low 32 bits)"""
    k &= _M64
    k ^= k >> 33; k = (k * 0xff51afd7ed558ccd) & _M64; k ^= k >> 33; k = (k * 0xc4ceb9fe1a85ec53) & _M64; k ^= k >> 33
    return k & 0xFFFFFFFF


def id_table_cells(n):
    """cells of a table for n ids: a power of two, at least 64, at most half full"""
    c = 64
    while c < 2 * max(n, 1):
        c <<= 1
    return c


def colliding_ids(n, table_cells, rng, n_collide=16):
    """n distinct ids (uint64, none of them NO_MAP_POINT) of which the first n_collide hash to the last four cells of a table of table_cells cells, so that linear
    probing from there runs past the last cell and wraps to cell 0; id 0 and id 2**64 - 2 are among the rest.  An input generator only: nothing is asserted against
    this hash on the GPU.  If the kernels' hash changes, the tests that use these ids stay valid -- the ids are still distinct ids -- and only this case loses its
    point (tests/test_random_cases.py then says so: it checks the chain under the restated hash)."""
    assert n >= n_collide + 2
    hit, seen = [], {0, _M64 - 1, _M64}
    while len(hit) < n_collide:
        for k in rng.integers(0, 1 << 63, 4096, dtype=np.uint64):
            k = int(k) * 2 + 1
            if k not in seen and (id_hash(k) & (table_cells - 1)) >= table_cells - 4:
                hit.append(k); seen.add(k)
    rest = [0, _M64 - 1]
    while len(rest) < n - n_collide:
        k = int(rng.integers(1, 1 << 62, dtype=np.uint64))
        if k not in seen:
            rest.append(k); seen.add(k)
    return np.array(hit[:n_collide] + rest, np.uint64)


def probe_chain(ids, table_cells):
    """linear probing of the ids in order into an empty table: (longest displacement from the home cell, number of ids that wrapped past the last cell)"""
    cells = [None] * table_cells
    longest = wrapped = 0
    for k in ids:
        h = home = id_hash(int(k)) & (table_cells - 1); d = 0
        while cells[h] is not None:
            h = (h + 1) & (table_cells - 1); d += 1
        cells[h] = int(k); longest = max(longest, d); wrapped += h < home
    return longest, wrapped


def row_medians(desc):
    """vDists[0.5*(N-1)] of every sorted row of the N x N Hamming matrix (MapPoint.cc:371-395); the reference keeps the first row with the least median"""
    b = np.unpackbits(np.asarray(desc, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    D = (b[:, None, :] != b[None, :, :]).sum(2)
    return np.sort(D, axis=1)[:, int(0.5 * (len(b) - 1))]

"""Keyframe insertion of the reference, restated as plain serial loops on dict records: the definition the calls of include/corb_keyframe_insert.h are compared with
byte for byte.  Paths are under corbslam_client/src of the reference.

  scene["kfs"][slot]   a keyframe / frame record or None: id, Tcw (4x4 float32), nlevels, kf_flags, kp (KP_DTYPE), desc (n x 32), u_right, depth, flags (uint8 per
                       feature: bit 0 has-a-map-point, bit 1 outlier), mp_id (uint64, NO_MAP_POINT = none)
  scene["mps"][slot]   a map-point record or None (a record of zeros): id, ref_kf_id, descriptor, client_id, flags, world_pos, normal, min_distance, max_distance,
                       obs = [(keyframe id, feature index)] ascending in the id, n_visible, n_found, replaced_by, scratch (dict of the non-zero CorbMapPointScratch fields)
  scene["index"]       MapPoint id -> slot, what corb_mp_store_build_index built (build_index below)
  scene["cam"]         fx, fy, cx, cy, scale (mvScaleFactors)
  scene["F"], ["O"]    features per keyframe record, observations per map-point record

Readings: float expressions with the C++ types of the source, one IEEE operation at a time; cv::Mat products = cv::gemm (double accumulation, one
rounding); cv::norm = a double sum; Mat / double = a product with the reciprocal.  UnprojectStereo is tests/newpoints_reference.py's; UpdateNormalAndDepth follows
csrc/normal_depth.h (camera centre in float).  Every function leaves `scene` alone and returns (outputs, scene afterwards): with apply == 0, or on a capacity error, the
second is the scene it was given."""
import copy

import numpy as np

import newpoints_reference as NP

f32, f64 = np.float32, np.float64
NO_MAP_POINT = NP.NO_MAP_POINT
KP_DTYPE = NP.KP_DTYPE
MP_BAD, KF_BAD = 1, 1
HAS_MP, OUTLIER = 1, 2


# ---------------------------------------------------------------- the visit rule (Tracking.cc:1103-1156, :832-883, :524-540)
def visit_order(depth, th_depth, mode):
    """feature indices in the order the loop visits them"""
    depth = np.asarray(depth, f32)
    if mode == 0:                                                   # StereoInitialization: for(int i=0; i<N; i++) { float z = mvDepth[i]; if(z>0)
        return [i for i in range(len(depth)) if depth[i] > 0]
    v = []
    for i in range(len(depth)):
        z = depth[i]
        if z > 0:                                                   # (NaN fails)
            v.append((float(z), i))
    v.sort()                                                        # sort(vDepthIdx.begin(), vDepthIdx.end()): pair<float,int>, equal depths in index order
    out = []; n_points = 0
    for z, i in v:
        out.append(i)
        n_points += 1                                               # (both branches of bCreateNew increment)
        if f32(z) > f32(th_depth) and n_points > 100:
            break
    return out


def n_visited_closed_form(m, n_near, mode):
    """csrc/kfinsert_math.h kfi_n_visited: m candidates of which n_near are not beyond th_depth"""
    if mode == 0:
        return m
    J = max(100, n_near)
    return J + 1 if J < m else m


# ---------------------------------------------------------------- arithmetic
def centre_float(T):
    """KeyFrame::SetPose's Ow in float (csrc/kfinsert_math.h bas_camera_center, which csrc/normal_depth.h uses)"""
    T = np.asarray(T, f32).reshape(4, 4)
    return np.array([-(T[0, a] * T[0, 3] + T[1, a] * T[1, 3] + T[2, a] * T[2, 3]) for a in range(3)], f32)


def _level(octave, nlevels):
    nl = min(max(int(nlevels), 1), 16)
    return min(max(int(octave), 0), nl - 1), nl


def unproject(Tcw, cam, kp, z):
    """Frame::UnprojectStereo (Frame.cc:670-684)"""
    return NP._unproject(NP._Cam(dict(Tcw=Tcw, fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"])), kp, z)


def single_observation(Tcw, X, octave, nlevels, scale):
    """UpdateNormalAndDepth (MapPoint.cc:424-471) of a point with the one observation in the keyframe of pose Tcw: (normal, min_distance, max_distance)"""
    Ow = centre_float(Tcw); X = np.asarray(X, f32)
    v = [f32(X[a] - Ow[a]) for a in range(3)]
    s = f64(v[0]) * f64(v[0]) + f64(v[1]) * f64(v[1]) + f64(v[2]) * f64(v[2])
    with np.errstate(all="ignore"):
        inv = f64(1) / np.sqrt(s)
        nrm = [f32(f32(0) + f32(f64(v[a]) * inv)) for a in range(3)]
        dist = f32(np.sqrt(s))
        level, nl = _level(octave, nlevels)
        normal = np.array([f32(f64(nrm[a]) * (f64(1) / f64(1))) for a in range(3)], f32)
        mx = f32(dist * f32(scale[level])); mn = f32(mx / f32(scale[nl - 1]))
    return normal, mn, mx


def temporal_point(Tcw, X, octave, nlevels, scale):
    """MapPoint(x3D, cacher, pFrame, idxF) (MapPoint.cc:61-95): Ow = the frame's mOw (gemm), normal = (Pos - Ow) / norm, the distances from the feature's octave"""
    Ow = NP.camera_centre(Tcw); X = np.asarray(X, f32)
    v = [f32(X[a] - Ow[a]) for a in range(3)]
    with np.errstate(all="ignore"):
        nrm = np.sqrt(f64(v[0]) * f64(v[0]) + f64(v[1]) * f64(v[1]) + f64(v[2]) * f64(v[2])); inv = f64(1) / nrm
        normal = np.array([f32(f64(v[a]) * inv) for a in range(3)], f32)
        dist = f32(nrm)
        level, nl = _level(octave, nlevels)
        mx = f32(dist * f32(scale[level])); mn = f32(mx / f32(scale[nl - 1]))
    return normal, mn, mx


def found_ratio_culls(n_found, n_visible):
    """GetFoundRatio() < 0.25f: static_cast<float>(mnFound) / mnVisible"""
    with np.errstate(all="ignore"):
        return bool(f32(np.int32(n_found)) / f32(np.int32(n_visible)) < f32(0.25))


def cull_decision(bad, n_found, n_visible, cur_kf_id, first_kf_id, n_obs_weighted, th_obs):
    """the else-if chain of LocalMapping.cc:175-186"""
    age = int(np.int64(cur_kf_id).astype(np.int32)) - int(np.int64(first_kf_id).astype(np.int32))      # (int)nCurrentKFid - (int)pMP->mnFirstKFid
    if bad:
        return 1
    if found_ratio_culls(n_found, n_visible):
        return 2
    if age >= 2 and n_obs_weighted <= th_obs:
        return 3
    if age >= 3:
        return 4
    return 0


# ---------------------------------------------------------------- records
def blank_point():
    return dict(id=0, ref_kf_id=0, descriptor=np.zeros(32, np.uint8), client_id=0, flags=0, world_pos=np.zeros(3, f32), normal=np.zeros(3, f32), min_distance=f32(0),
                max_distance=f32(0), obs=[], n_visible=0, n_found=0, replaced_by=0, scratch={})


def build_index(scene, first, n):
    scene["index"] = {}
    for s in range(first, first + n):
        mp = scene["mps"][s]
        pid = 0 if mp is None else int(mp["id"])
        assert pid not in scene["index"], "two of the slots hold the same id"
        scene["index"][pid] = s


def resolve(scene, pid):
    """slot of the record the id resolves to, or None"""
    pid = int(pid)
    return None if pid == NO_MAP_POINT else scene["index"].get(pid)


def at_hand(scene, kf_first, kf_n):
    """keyframe id -> slot among the named slots (a slot without features is no keyframe; of two slots with one id the lower)"""
    out = {}
    for s in range(kf_first, kf_first + kf_n):
        k = scene["kfs"][s]
        if k is not None and len(k["kp"]) > 0 and int(k["id"]) not in out:
            out[int(k["id"])] = s
    return out


def _mp(scene, slot):
    if scene["mps"][slot] is None:
        scene["mps"][slot] = blank_point()
    return scene["mps"][slot]


def observations(scene, mp, hand):
    """MapPoint::Observations(): the weighted nObs (MapPoint.cc:155-158) from the list -- 2 when the keyframe is at hand and stereo at that feature, else 1"""
    w = 0
    for kid, idx in mp["obs"]:
        s = hand.get(int(kid))
        w += 2 if s is not None and idx < len(scene["kfs"][s]["kp"]) and scene["kfs"][s]["u_right"][idx] >= 0 else 1
    return w


# ---------------------------------------------------------------- call 1
def create_stereo_points(scene, slot, th_depth, mode, apply, first_mp_slot=0, first_mp_id=0, client_id=0, frame_id=0, mirror=None):
    """Tracking::CreateNewKeyFrame (:1103-1156, mode 1), StereoInitialization (:524-540, mode 0), UpdateLastFrame (:830-883, mode 2).  mirror = (slot) of a second
    record whose ids take the same writes.  Returns dict(order, kind, x3d, n_visited, n_created, capacity_error), scene afterwards."""
    S = copy.deepcopy(scene); kf = S["kfs"][slot]; cam = S["cam"]
    order = visit_order(kf["depth"], th_depth, mode)
    kinds, x3d, new = [], [], []
    for i in order:
        pid = int(kf["mp_id"][i])
        if mode == 0 or pid == NO_MAP_POINT:
            kind = 1                                                # if(!pMP) bCreateNew = true;
        else:
            s = resolve(scene, pid)
            if s is None:
                kind = 3                                            # a temporal point the store never saw: held
            else:
                kind = 2 if len(_mp(scene, s)["obs"]) < 1 else 0   # else if(pMP->Observations()<1)
        kinds.append(kind)
        if kind not in (1, 2):
            continue
        X = unproject(kf["Tcw"], cam, kf["kp"][i], kf["depth"][i])
        k = len(x3d); x3d.append(X)
        p = blank_point()
        p["id"] = first_mp_id + k; p["client_id"] = client_id; p["world_pos"] = X; p["descriptor"] = kf["desc"][i].copy()
        p["n_visible"] = 1; p["n_found"] = 1
        octave = int(kf["kp"][i]["octave"]); nlevels = len(cam["scale"])
        if mode == 2:
            p["normal"], p["min_distance"], p["max_distance"] = temporal_point(kf["Tcw"], X, octave, nlevels, cam["scale"])
            p["scratch"] = dict(first_kf_id=-1, first_frame=frame_id, track_in_view=1)
        else:
            p["ref_kf_id"] = int(kf["id"]); p["obs"] = [(int(kf["id"]), i)]
            p["normal"], p["min_distance"], p["max_distance"] = single_observation(kf["Tcw"], X, octave, nlevels, cam["scale"])
            p["scratch"] = dict(first_kf_id=int(kf["id"]), first_frame=frame_id, n_obs_weight=2 if kf["u_right"][i] >= 0 else 1)
        new.append((i, p))
    out = dict(order=np.array(order, np.int32), kind=np.array(kinds, np.uint8), x3d=np.array(x3d, f32).reshape(-1, 3), n_visited=len(order), n_created=len(new), capacity_error=False)
    if not apply:
        return out, scene
    if len(new) > len(S["mps"]) - first_mp_slot:
        out["capacity_error"] = True
        return out, scene
    for k, (i, p) in enumerate(new):
        S["mps"][first_mp_slot + k] = p
        for r in [kf] + ([S["kfs"][mirror]] if mirror is not None else []):
            r["mp_id"][i] = p["id"]; r["flags"][i] |= HAS_MP
    return out, S


# ---------------------------------------------------------------- call 2
def need_keyframe_counts(scene, cur_slot, th_depth, ref_slot, min_obs, kf_first, kf_n, frames=None):
    """(nTrackedClose, nNonTrackedClose) of Tracking.cc:1026-1035 on the frame record, nRefMatches = KeyFrame::TrackedMapPoints(min_obs) on the reference keyframe"""
    cur = (frames if frames is not None else scene["kfs"])[cur_slot]
    tracked = non = 0
    for i in range(len(cur["kp"])):
        z = f32(cur["depth"][i])
        if z > 0 and z < f32(th_depth):
            if resolve(scene, cur["mp_id"][i]) is not None and not (cur["flags"][i] & OUTLIER):
                tracked += 1
            else:
                non += 1
    ref_matches = 0
    if ref_slot >= 0:
        hand = at_hand(scene, kf_first, kf_n); ref = scene["kfs"][ref_slot]
        for i in range(len(ref["kp"])):
            s = resolve(scene, ref["mp_id"][i])
            if s is None or (_mp(scene, s)["flags"] & MP_BAD):
                continue
            if min_obs > 0:
                if observations(scene, _mp(scene, s), hand) >= min_obs:
                    ref_matches += 1
            else:
                ref_matches += 1
    return tracked, non, ref_matches


# ---------------------------------------------------------------- call 3
def update_normal_and_depth(scene, mp, hand, scale_factor):
    """csrc/normal_depth.h corb_update_normal_depth over the keyframes at hand"""
    pr = hand.get(int(mp["ref_kf_id"]))
    if pr is None:
        return
    pos = np.asarray(mp["world_pos"], f32)
    ref_f = -1; n = 0; acc = [f32(0), f32(0), f32(0)]
    for kid, idx in mp["obs"]:
        if int(kid) == int(mp["ref_kf_id"]):
            ref_f = idx
        s = hand.get(int(kid))
        if s is None:
            continue
        Ow = centre_float(scene["kfs"][s]["Tcw"])
        v = [f32(pos[a] - Ow[a]) for a in range(3)]
        inv = f64(1) / np.sqrt(f64(v[0]) * f64(v[0]) + f64(v[1]) * f64(v[1]) + f64(v[2]) * f64(v[2]))
        acc = [f32(acc[a] + f32(f64(v[a]) * inv)) for a in range(3)]; n += 1
    ref = scene["kfs"][pr]
    if ref_f < 0 or ref_f >= len(ref["kp"]) or n == 0:
        return
    Or = centre_float(ref["Tcw"])
    c = [f32(pos[a] - Or[a]) for a in range(3)]
    dist = f32(np.sqrt(f64(c[0]) * f64(c[0]) + f64(c[1]) * f64(c[1]) + f64(c[2]) * f64(c[2])))
    level, nl = _level(ref["kp"][ref_f]["octave"], ref["nlevels"])
    sc = f32(1); sc_level = f32(1)
    for l in range(1, nl):
        sc = f32(sc * f32(scale_factor))
        if l == level:
            sc_level = sc
    mp["max_distance"] = f32(dist * sc_level); mp["min_distance"] = f32(mp["max_distance"] / sc)
    rn = f64(1) / f64(n)
    mp["normal"] = np.array([f32(f64(acc[a]) * rn) for a in range(3)], f32)


def compute_distinctive_descriptors(scene, mp, hand):
    """MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:337-402) over the observations in non-bad keyframes at hand: the first row of least median"""
    if mp["flags"] & MP_BAD:
        return
    D = []
    for kid, idx in mp["obs"]:
        s = hand.get(int(kid))
        if s is None or (scene["kfs"][s]["kf_flags"] & KF_BAD) or idx >= scene["F"]:
            continue
        D.append(scene["kfs"][s]["desc"][idx])
    if not D:
        return
    bits = np.unpackbits(np.array(D, np.uint8), axis=1).astype(np.int32)
    N = len(D); best, best_median = 0, 1 << 30
    for i in range(N):
        dists = sorted(int((bits[i] != bits[j]).sum()) for j in range(N))
        median = dists[int(0.5 * (N - 1))]
        if median < best_median:
            best_median, best = median, i
    mp["descriptor"] = np.array(D[best], np.uint8).copy()


def process_new_keyframe(scene, slot, kf_first, kf_n, scale_factor, apply):
    """LocalMapping::ProcessNewKeyFrame's loop (LocalMapping.cc:136-151).  Returns dict(kind, recent_slots, n_added, capacity_error), scene afterwards."""
    S = copy.deepcopy(scene); kf = S["kfs"][slot]; kid = int(kf["id"]); hand = at_hand(S, kf_first, kf_n)
    kinds, recent = [], []; full = False
    for i in range(len(kf["kp"])):
        pid = int(kf["mp_id"][i])
        if pid == NO_MAP_POINT:
            kinds.append(0); continue
        s = resolve(S, pid)
        if s is None:
            kinds.append(2); continue                               # MapPoint *pMP = vpMapPointMatches[i]; if (pMP)
        mp = _mp(S, s)
        if mp["flags"] & MP_BAD:
            kinds.append(1); continue                               # if (!pMP->isBad())
        if not any(int(k) == kid for k, _ in mp["obs"]):            # if (!pMP->IsInKeyFrame(mpCurrentKeyFrame))
            kinds.append(3)
            if len(mp["obs"]) >= S["O"]:
                full = True
                mp["obs"] = mp["obs"] + [(kid, i)]                  # (the answer is a capacity error; the later features still meet a point that is in the keyframe)
                continue
            mp["obs"] = sorted(mp["obs"] + [(kid, i)])              # pMP->AddObservation(mpCurrentKeyFrame, i)
            update_normal_and_depth(S, mp, hand, scale_factor)      # pMP->UpdateNormalAndDepth()
            compute_distinctive_descriptors(S, mp, hand)            # pMP->ComputeDistinctiveDescriptors()
        else:
            kinds.append(4); recent.append(s)                       # mlpRecentAddedMapPoints.push_back(pMP)
    out = dict(kind=np.array(kinds, np.uint8), recent_slots=np.array(recent, np.int32), n_added=kinds.count(3), capacity_error=full)
    return out, (S if apply and not full else scene)


# ---------------------------------------------------------------- call 4
def set_bad_flag(scene, mp, hand):
    """MapPoint::SetBadFlag (MapPoint.cc:255-269) as corb_local_ba_store does it on records"""
    for kid, idx in mp["obs"]:
        s = hand.get(int(kid))
        if s is None or idx >= len(scene["kfs"][s]["kp"]):
            continue
        scene["kfs"][s]["mp_id"][idx] = NO_MAP_POINT; scene["kfs"][s]["flags"][idx] &= ~np.uint8(HAS_MP)      # pKF->EraseMapPointMatch(mit->second)
    mp["flags"] |= MP_BAD; mp["obs"] = []


def map_point_culling(scene, recent_slots, cur_kf_id, th_obs, kf_first, kf_n, apply):
    """LocalMapping::MapPointCulling (LocalMapping.cc:161-188).  Returns dict(decision, kept_slots, n_culled), scene afterwards."""
    S = copy.deepcopy(scene); hand = at_hand(S, kf_first, kf_n)
    decision, kept = [], []
    for s in recent_slots:
        mp = _mp(S, int(s))
        d = cull_decision(bool(mp["flags"] & MP_BAD), mp["n_found"], mp["n_visible"], cur_kf_id, mp["scratch"].get("first_kf_id", 0), observations(S, mp, hand), th_obs)
        if d in (2, 3):
            set_bad_flag(S, mp, hand)
        if d == 0:
            kept.append(int(s))
        decision.append(d)
    out = dict(decision=np.array(decision, np.uint8), kept_slots=np.array(kept, np.int32), n_culled=sum(1 for d in decision if d in (2, 3)))
    return out, (S if apply else scene)

"""The server -> clients publish of the reference, restated as plain serial Python on dict records: the definition the calls of include/corb_map_publish.h are compared
with byte for byte.  S/ = corbslam_server/src, C/ = corbslam_client/src of the reference.

  keyframe record    dict: id, client_id, kf_flags (KF_BAD | KF_FIXED), nlevels, fx, fy, cx, cy, bf, Tcw, TcwGBA (4x4 float32), kp (KP_DTYPE), desc (n x 32), u_right,
                     depth, mp_id -- the fields tests/kfinsert_reference.py's records have, plus the ones a pushed keyframe carries
  map-point record   dict: id, ref_kf_id, descriptor, client_id, flags (MP_BAD | MP_FIXED), world_pos, normal, min_distance, max_distance, obs = [(keyframe id,
                     feature index)], n_visible, n_found, replaced_by
  a store            a list of records by slot; None = an empty slot
  message            dict A (keyframe records), B (map-point records), C [(id, KFPose 4x4)], D [(id, position)], E [(client id, T, Tinv)]: what the server's four
                     publishers hand out (S/PubToClient.cpp:24-163) with transMs beside them
  client             dict client_id, kfs, mps (stores), kf_first, kf_n (the slots getKeyFrameById searches), kf_free_first, kf_room, mp_first, mp_n (the slots the
                     map's id index covers), mp_free_first, mp_room

Readings: cv::Mat products are cv::gemm (exact float products summed in double, left to right, one rounding); Rcw * p + tcw is one gemm with
the addend: the double row sum plus (double)t, rounded once; Mat::inv of a float 4x4 is the cofactor inverse of the full 4x4 in double, times 1 / det, rounded once.
The subscriber loops are transcribed, not vectorised; `apply` leaves `client` alone and returns (outputs, client afterwards): with apply = False, or when the free
slots do not hold what the loops accept, the second is the client it was given."""
import copy

import numpy as np

f32, f64 = np.float32, np.float64
KF_BAD, KF_FIXED, MP_BAD, MP_FIXED = 1, 2, 1, 2


class PackError(Exception):
    """corb_pub_pack answers CORB_ERR_ARG"""


# ---------------------------------------------------------------- arithmetic
def det3(a, b, c, d, e, f, g, h, i):
    return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)


def cofactor(A, r, c):
    rr = [k for k in range(4) if k != r]; cc = [k for k in range(4) if k != c]
    m = det3(A[rr[0]][cc[0]], A[rr[0]][cc[1]], A[rr[0]][cc[2]], A[rr[1]][cc[0]], A[rr[1]][cc[1]], A[rr[1]][cc[2]], A[rr[2]][cc[0]], A[rr[2]][cc[1]], A[rr[2]][cc[2]])
    return -m if (r + c) & 1 else m


def inverse4(T):
    """Ttrans.inv() (Cache.cc:479): csrc/publish_math.h pub_inverse4, the same expressions in float64.  None: the determinant is zero or not finite"""
    A = [[f64(f32(T[r][c])) for c in range(4)] for r in range(4)]
    with np.errstate(all="ignore"):
        C = [[cofactor(A, r, c) for c in range(4)] for r in range(4)]
        det = ((A[0][0] * C[0][0] + A[0][1] * C[0][1]) + A[0][2] * C[0][2]) + A[0][3] * C[0][3]
        if not (det != 0) or not np.isfinite(det):
            return None
        inv = f64(1) / det
        return np.array([[f32(C[c][r] * inv) for c in range(4)] for r in range(4)], f32)


def mul44(a, M):
    """Tcw * Ttrans.inv(): cv::gemm of two float 4x4"""
    a = np.asarray(a, f32).reshape(4, 4); M = np.asarray(M, f32).reshape(4, 4)
    o = np.zeros((4, 4), f32)
    with np.errstate(all="ignore"):
        for r in range(4):
            for c in range(4):
                s = f64(a[r, 0]) * f64(M[0, c])
                s = s + f64(a[r, 1]) * f64(M[1, c])
                s = s + f64(a[r, 2]) * f64(M[2, c])
                s = s + f64(a[r, 3]) * f64(M[3, c])
                o[r, c] = f32(s)
    return o


def point(T, p):
    """Rcw * tPose + tcw with Rcw, tcw of Ttrans (Cache.cc:528-531)"""
    T = np.asarray(T, f32).reshape(4, 4); p = np.asarray(p, f32)
    o = np.zeros(3, f32)
    with np.errstate(all="ignore"):
        for r in range(3):
            s = f64(T[r, 0]) * f64(p[0])
            s = s + f64(T[r, 1]) * f64(p[1])
            s = s + f64(T[r, 2]) * f64(p[2])
            s = s + f64(T[r, 3])
            o[r] = f32(s)
    return o


# ---------------------------------------------------------------- the server: PubToClient's four sets and transMs
def pack(kfs, new_kf_slots, upd_kf_slots, mps, new_mp_slots, upd_mp_slots, trans):
    """trans = [(client id, T)] in table order.  Entries keep the order of the slot lists."""
    for s in list(new_kf_slots) + list(upd_kf_slots):
        if s < 0 or s >= len(kfs) or kfs[s] is None:
            raise PackError("keyframe slot %d" % s)
    for s in list(new_mp_slots) + list(upd_mp_slots):
        if s < 0 or s >= len(mps):
            raise PackError("map-point slot %d" % s)
    seen = set(); E = []
    for cid, T in trans:
        if cid in seen:
            raise PackError("client %d named twice" % cid)
        seen.add(cid)
        T = np.array(T, f32).reshape(4, 4); Tinv = inverse4(T)
        if Tinv is None:
            raise PackError("client %d: singular transform" % cid)
        E.append((int(cid), T, Tinv))
    return dict(A=[copy.deepcopy(kfs[s]) for s in new_kf_slots], B=[copy.deepcopy(mps[s]) for s in new_mp_slots],
                C=[(int(kfs[s]["id"]), np.array(kfs[s]["Tcw"], f32).reshape(4, 4)) for s in upd_kf_slots],
                D=[(int(mps[s]["id"]), np.array(mps[s]["world_pos"], f32)) for s in upd_mp_slots], E=E)


# ---------------------------------------------------------------- the client: Cache's lookups and its four subscriber callbacks
def get_keyframe_by_id(cl, kid):
    """Cache::getKeyFrameById over the slots the call names and the ones this call filled: a slot without features is no keyframe, the lower slot wins"""
    for s in range(cl["kf_first"], cl["kf_first"] + cl["kf_n"]):
        k = cl["kfs"][s]
        if k is not None and len(k["kp"]) > 0 and int(k["id"]) == int(kid):
            return s
    for s in cl["_kf_new"]:                                        # (accepted by this call: held whatever it carries)
        if int(cl["kfs"][s]["id"]) == int(kid):
            return s
    return -1


def get_map_point_by_id(cl, pid):
    """Cache::getMapPointById through the map's id index and the slots this call filled"""
    s = cl["_index"].get(int(pid), -1)
    if s >= 0:
        return s
    for s in cl["_mp_new"]:
        if int(cl["mps"][s]["id"]) == int(pid):
            return s
    return -1


def transform_of(msg, client_id):
    """transMs.find(pClientId) (Cache.cc:456)"""
    for cid, T, Tinv in msg["E"]:
        if cid == client_id:
            return T, Tinv
    return None


def sub_new_keyframes(msg, cl, kind):
    """Cache::subNewInsertKeyFramesFromServer (Cache.cc:446-492)"""
    tr = transform_of(msg, cl["client_id"])
    if tr is None:
        return
    Ttrans, Tinv = tr
    for mit in range(len(msg["A"])):
        tKF = copy.deepcopy(msg["A"][mit])
        if tKF["client_id"] != cl["client_id"]:
            if get_keyframe_by_id(cl, tKF["id"]) >= 0:
                kind[mit] = 2
                continue
            tKF["Tcw"] = mul44(tKF["Tcw"], Tinv)                   # Tcw = Tcw * Ttrans.inv(); tKF->SetPose( Tcw );
            tKF["kf_flags"] = int(tKF["kf_flags"]) | KF_FIXED      # tKF->setFixed();
            slot = cl["kf_free_first"] + len(cl["_kf_new"])        # this->AddKeyFrameFromServer(tKF)
            while len(cl["kfs"]) <= slot:
                cl["kfs"].append(None)                             # (beyond the room: the call will answer CORB_ERR_CAPACITY and keep nothing)
            cl["kfs"][slot] = tKF; cl["_kf_new"].append(slot)
            kind[mit] = 3
        else:
            kind[mit] = 1


def sub_new_map_points(msg, cl, kind):
    """Cache::subNewInsertMapPointFromServer (Cache.cc:494-543); mNormalVector, mfMinDistance and mfMaxDistance stay as sent"""
    tr = transform_of(msg, cl["client_id"])
    if tr is None:
        return
    Ttrans, Tinv = tr
    for mit in range(len(msg["B"])):
        tMP = copy.deepcopy(msg["B"][mit])
        if tMP["client_id"] != cl["client_id"]:
            if get_map_point_by_id(cl, tMP["id"]) >= 0:
                kind[mit] = 2
                continue
            tMP["world_pos"] = point(Ttrans, tMP["world_pos"])     # tPose = Rcw * tPose + tcw
            tMP["flags"] = int(tMP["flags"]) | MP_FIXED            # tMP->setFixed();
            slot = cl["mp_free_first"] + len(cl["_mp_new"])        # this->AddMapPointFromServer(tMP)
            while len(cl["mps"]) <= slot:
                cl["mps"].append(None)
            cl["mps"][slot] = tMP; cl["_mp_new"].append(slot)
            kind[mit] = 3
        else:
            kind[mit] = 1


def sub_updated_keyframe_poses(msg, cl, kind):
    """Cache::subUpdatedKeyFramesPose (Cache.cc:545-587)"""
    tr = transform_of(msg, cl["client_id"])
    if tr is None:
        return
    Ttrans, Tinv = tr
    for mit in range(len(msg["C"])):
        KFPId, KFPose = msg["C"][mit]
        s = get_keyframe_by_id(cl, KFPId)
        if s < 0:
            continue
        tKF = cl["kfs"][s]
        if int(tKF["kf_flags"]) & KF_FIXED:                        # if (tKF && tKF->getFixed())
            tKF["Tcw"] = mul44(KFPose, Tinv)
            kind[mit] = 2
        else:
            kind[mit] = 1


def sub_updated_map_point_poses(msg, cl, kind):
    """Cache::subUpdatedMapPointsPose (Cache.cc:589-634)"""
    tr = transform_of(msg, cl["client_id"])
    if tr is None:
        return
    Ttrans, Tinv = tr
    for mit in range(len(msg["D"])):
        MPPId, MPPose = msg["D"][mit]
        s = get_map_point_by_id(cl, MPPId)
        if s < 0:
            continue
        tMP = cl["mps"][s]
        if int(tMP["flags"]) & MP_FIXED:
            tMP["world_pos"] = point(Ttrans, MPPose)
            kind[mit] = 2
        else:
            kind[mit] = 1


def build_index(cl):
    """corb_mp_store_build_index over [mp_first, mp_first + mp_n)"""
    return {int(cl["mps"][s]["id"]): s for s in range(cl["mp_first"], cl["mp_first"] + cl["mp_n"])}


def apply(msg, client, apply=True):
    """corb_pub_apply: the four callbacks in the publication order of MapFusion.cpp:352-358.  Returns (outputs, client afterwards)."""
    cl = copy.deepcopy(client)
    cl["_kf_new"] = []; cl["_mp_new"] = []; cl["_index"] = build_index(cl)
    kinds = [np.zeros(len(msg[k]), np.uint8) for k in "ABCD"]
    sub_new_keyframes(msg, cl, kinds[0])
    sub_new_map_points(msg, cl, kinds[1])
    sub_updated_keyframe_poses(msg, cl, kinds[2])
    sub_updated_map_point_poses(msg, cl, kinds[3])
    n_kf, n_mp = len(cl["_kf_new"]), len(cl["_mp_new"])
    full = n_kf > client["kf_room"] or n_mp > client["mp_room"]
    out = dict(kind_kf_new=kinds[0], kind_mp_new=kinds[1], kind_kf_upd=kinds[2], kind_mp_upd=kinds[3],
               kf_new_slots=np.array(cl["_kf_new"][: client["kf_room"]], np.int32), mp_new_slots=np.array(cl["_mp_new"][: client["mp_room"]], np.int32),
               n_kf_inserted=n_kf, n_mp_inserted=n_mp, n_kf_updated=int((kinds[2] == 2).sum()), n_mp_updated=int((kinds[3] == 2).sum()),
               no_transform=int(transform_of(msg, client["client_id"]) is None), capacity_error=bool(full))
    if not apply or full:
        return out, copy.deepcopy(client)
    for k in ("_kf_new", "_mp_new", "_index"):
        del cl[k]
    cl["mp_n"] = client["mp_n"] + n_mp if n_mp else client["mp_n"]          # the rebuilt index covers the new slots
    return out, cl


# ---------------------------------------------------------------- the closed forms the kernels evaluate
def kinds_new_closed_form(ids, client_ids, client_id, held, found):
    """A / B without the loop: own -> 1; held -> 2; of the others with one id the lowest position -> 3, the rest -> 2"""
    kind = np.zeros(len(ids), np.uint8)
    if not found:
        return kind
    first = {}
    for i in range(len(ids)):
        if client_ids[i] != client_id and int(ids[i]) not in held:
            first.setdefault(int(ids[i]), i)
    for i in range(len(ids)):
        kind[i] = 1 if client_ids[i] == client_id else (3 if first.get(int(ids[i])) == i else 2)
    return kind


def upd_closed_form(ids, values, fixed_of, found):
    """C / D without the loop.  fixed_of: id -> whether the held entity is fixed (absent: not held; the entities phases A / B accepted are held and fixed).
    Returns (kind, {id: the value that stays}): of several kind-2 entries with one id the highest position's"""
    kind = np.zeros(len(ids), np.uint8); last = {}
    if not found:
        return kind, {}
    for i in range(len(ids)):
        if int(ids[i]) in fixed_of:
            kind[i] = 2 if fixed_of[int(ids[i])] else 1
            if kind[i] == 2:
                last[int(ids[i])] = i
    return kind, {k: values[i] for k, i in last.items()}

"""Records of tests/publish_reference.py <-> bytes and device stores.  The byte layouts are restated from the record descriptions in include/corb_accel.h (keyframe
record: 256-byte header = {n, n_nodes, CorbKeyFrameMeta}, then kp | desc | u_right | depth | angle | flags | fv_node | fv_off | fv_idx | mp_id, every section 64-byte
aligned; map-point record: CorbMapPointRecord, the counters, obs_kf | obs_idx, CorbMapPointScratch), as corb_kf_store_put_batch and corb_mp_store_put_host +
corb_mp_store_set_counters leave them in a zero-initialised store -- so that "every byte of every record" can be checked against the definition.  Shared by
tests/test_gpu_publish*.py and tools/publish_rate.py; `corb` is the loaded package."""
import numpy as np

import publish_reference as R

NO_MAP_POINT = 0xFFFFFFFFFFFFFFFF


def _al(v, a=64):
    return (v + a - 1) // a * a


def kf_layout(F):
    o = 256; L = {}
    for name, size in (("kp", 28 * F), ("desc", 32 * F), ("ur", 4 * F), ("depth", 4 * F), ("angle", 4 * F), ("flags", F), ("fv_node", 4 * F), ("fv_off", 4 * (F + 1)), ("fv_idx", 4 * F), ("mp_id", 8 * F)):
        L[name] = o; o = _al(o + size)
    L["bytes"] = o
    return L


def mp_layout(O):
    L = dict(obs_kf=128, obs_idx=128 + 8 * O); L["scratch"] = _al(L["obs_idx"] + 4 * O); L["bytes"] = _al(L["scratch"] + 104)
    return L


def kf_meta(corb, k):
    m = np.zeros((), corb.KF_META_DTYPE)
    m["id"] = k["id"]; m["client_id"] = k["client_id"]; m["flags"] = k["kf_flags"]; m["nlevels"] = k["nlevels"]
    for f in ("fx", "fy", "cx", "cy", "bf", "ba_global_for_kf", "inv_level_sigma2"):
        m[f] = k[f]
    m["Tcw"] = np.asarray(k["Tcw"], np.float32).reshape(16); m["TcwGBA"] = np.asarray(k["TcwGBA"], np.float32).reshape(16)
    return m


def kf_raw(corb, k, F):
    """the bytes of a keyframe record"""
    L = kf_layout(F); b = np.zeros(L["bytes"], np.uint8); n = len(k["kp"])
    b[0:4] = np.array([n], np.int32).view(np.uint8); b[8:248] = np.frombuffer(kf_meta(corb, k).tobytes(), np.uint8)

    def put(name, arr, fill=None, width=None):
        full = np.zeros(F, arr.dtype) if arr.ndim == 1 else np.zeros((F,) + arr.shape[1:], arr.dtype)
        if fill is not None:
            full[...] = fill
        full[:n] = arr
        raw = np.frombuffer(full.tobytes(), np.uint8); b[L[name]: L[name] + len(raw)] = raw
    put("kp", np.ascontiguousarray(k["kp"], corb.KP_DTYPE)); put("desc", np.ascontiguousarray(k["desc"], np.uint8).reshape(n, 32))
    put("ur", np.asarray(k["u_right"], np.float32), -1.0); put("depth", np.asarray(k["depth"], np.float32), -1.0)
    put("angle", np.ascontiguousarray(k["kp"]["angle"], np.float32)); put("mp_id", np.asarray(k["mp_id"], np.uint64), NO_MAP_POINT)
    return b.tobytes()


def mp_header(corb, p):
    r = np.zeros((), corb.MP_RECORD_DTYPE)
    for f in ("id", "ref_kf_id", "descriptor", "client_id", "flags", "world_pos", "normal", "min_distance", "max_distance", "pos_gba", "ba_global_for_kf"):
        r[f] = p[f]
    r["n_obs"] = len(p["obs"])
    return r


def mp_raw(corb, p, O):
    L = mp_layout(O); b = np.zeros(L["bytes"], np.uint8)
    b[0:112] = np.frombuffer(mp_header(corb, p).tobytes(), np.uint8)
    c = np.zeros((), corb.MP_COUNTERS_DTYPE); c["n_visible"] = p["n_visible"]; c["n_found"] = p["n_found"]; c["replaced_by"] = p["replaced_by"]
    b[112:128] = np.frombuffer(c.tobytes(), np.uint8)
    okf = np.zeros(O, np.uint64); oi = np.zeros(O, np.uint32)
    for q, (k, i) in enumerate(p["obs"]):
        okf[q] = k; oi[q] = i
    b[L["obs_kf"]: L["obs_kf"] + 8 * O] = np.frombuffer(okf.tobytes(), np.uint8); b[L["obs_idx"]: L["obs_idx"] + 4 * O] = np.frombuffer(oi.tobytes(), np.uint8)
    return b.tobytes()


def message_raw(corb, msg, F, O):
    """the bytes of a message and its counts (include/corb_map_publish.h: five sections, each at a multiple of 16)"""
    A = b"".join(kf_raw(corb, k, F) for k in msg["A"]); B = b"".join(mp_raw(corb, p, O) for p in msg["B"])
    C = np.zeros(len(msg["C"]), corb.KF_POSE_PACKET_DTYPE); D = np.zeros(len(msg["D"]), corb.MP_POSE_PACKET_DTYPE); E = np.zeros(len(msg["E"]), corb.PUBLISH_TRANSFORM_DTYPE)
    for i, (kid, T) in enumerate(msg["C"]):
        C[i]["id"] = kid; C[i]["Tcw"] = np.asarray(T, np.float32).reshape(16)
    for i, (pid, x) in enumerate(msg["D"]):
        D[i]["id"] = pid; D[i]["pos"] = x
    for i, (cid, T, Tinv) in enumerate(msg["E"]):
        E[i]["client_id"] = cid; E[i]["T"] = T.reshape(16); E[i]["Tinv"] = Tinv.reshape(16)
    out = b""
    for sec in (A, B, C.tobytes(), D.tobytes(), E.tobytes()):
        out += sec + b"\0" * (_al(len(sec), 16) - len(sec))
    return out, [len(msg[k]) for k in "ABCDE"]


def to_stores(corb, kfs, mps, F, O, extra_kf=0, extra_mp=0):
    """every record of the two lists (no empty slot among them) filed from slot 0 on; extra_*: further, empty slots"""
    KF = corb.KeyFrameStore(max(len(kfs) + extra_kf, 1), F); MP = corb.MapPointStore(max(len(mps) + extra_mp, 1), O)
    if kfs:
        meta = np.array([kf_meta(corb, k) for k in kfs], corb.KF_META_DTYPE)
        off = np.concatenate([[0], np.cumsum([len(k["kp"]) for k in kfs])]).astype(np.int32)
        cat = lambda f, dt: np.concatenate([np.asarray(k[f], dt).reshape((len(k["kp"]),) + np.asarray(k[f]).shape[1:]) for k in kfs])
        KF.put_batch(0, meta, off, cat("kp", corb.KP_DTYPE), cat("desc", np.uint8), cat("u_right", np.float32), cat("depth", np.float32), cat("mp_id", np.uint64))
    if mps:
        rec = np.array([mp_header(corb, p) for p in mps], corb.MP_RECORD_DTYPE)
        lens = [len(p["obs"]) for p in mps]
        okf = np.array([k for p in mps for k, _ in p["obs"]], np.uint64); oi = np.array([i for p in mps for _, i in p["obs"]], np.uint32)
        MP.put(0, rec, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), okf, oi)
        MP.set_counters(0, [p["n_visible"] for p in mps], [p["n_found"] for p in mps], [p["replaced_by"] for p in mps])
    return KF, MP


def client_stores(corb, cl, F, O):
    KF, MP = to_stores(corb, cl["kfs"], cl["mps"], F, O)
    MP.build_index(cl["mp_first"], cl["mp_n"])
    return KF, MP


def raw_of(corb, reader, KF, n_kf, MP, n_mp):
    """the bytes of slots [0, n_kf) and [0, n_mp) as they stand on the device, read through a pack of whole records on `reader` (a MapPublisher of its own)"""
    reader.pack(KF, new_kf_slots=np.arange(n_kf), mp=MP, new_mp_slots=np.arange(n_mp))
    return reader.message_bytes().tobytes()


def raw_expected(corb, kfs, mps, F, O):
    return b"".join(kf_raw(corb, k, F) for k in kfs) + b"".join(mp_raw(corb, p, O) for p in mps)


def same_outputs(got, want):
    for k, v in want.items():
        g = got[k]
        if isinstance(v, np.ndarray):
            if not np.array_equal(np.asarray(g), v):
                return k
        elif int(g) != int(v):
            return k
    return None

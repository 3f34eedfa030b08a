"""Scenes of tests/kfinsert_reference.py <-> device stores: a scene filed into a KeyFrameStore / MapPointStore through the public calls, the arrays the definition's
records make, and what the stores hold read back as bytes.  Shared by tests/test_gpu_kfinsert.py and tools/kfinsert_rate.py; `corb` is the loaded package."""
import numpy as np


def to_stores(corb, sc):
    kfs = sc["kfs"]
    KF = corb.KeyFrameStore(len(kfs), sc["F"]); MP = corb.MapPointStore(len(sc["mps"]), sc["O"])
    for slot, k in enumerate(kfs):
        m = np.zeros((), corb.KF_META_DTYPE)
        m["id"] = k["id"]; m["client_id"] = 1; m["flags"] = k["kf_flags"]; m["nlevels"] = k["nlevels"]; m["Tcw"] = np.asarray(k["Tcw"], np.float32).reshape(16)
        for f in ("fx", "fy", "cx", "cy", "bf"):
            m[f] = sc["cam"][f]
        KF.put_frame(slot, k["kp"], k["desc"], k["u_right"], k["depth"], m)
        if "fv" in k:
            KF.set_bow(slot, k["fv"])
        if len(k["kp"]):
            KF.set_flags(slot, k["flags"]); KF.set_map_points(slot, k["mp_id"])
    rec, okf, oi, cnt, scr = mp_arrays(corb, sc)
    n = max([s + 1 for s, p in enumerate(sc["mps"]) if p is not None], default=0)
    if n:
        lens = rec["n_obs"][:n]
        MP.put(0, rec[:n], np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.concatenate([okf[s, : lens[s]] for s in range(n)]), np.concatenate([oi[s, : lens[s]] for s in range(n)]))
        MP.set_counters(0, cnt["n_visible"][:n], cnt["n_found"][:n], cnt["replaced_by"][:n]); MP.set_scratch(0, scr[:n])
    slots = sorted(sc["index"].values())
    assert slots == list(range(slots[0], slots[-1] + 1)) if slots else True
    MP.build_index(slots[0] if slots else 0, len(slots))            # (an index over no record resolves no id)
    return KF, MP


def mp_arrays(corb, sc):
    cap, O = len(sc["mps"]), sc["O"]
    rec = np.zeros(cap, corb.MP_RECORD_DTYPE); okf = np.zeros((cap, O), np.uint64); oi = np.zeros((cap, O), np.uint32)
    cnt = np.zeros(cap, corb.MP_COUNTERS_DTYPE); scr = np.zeros(cap, corb.MP_SCRATCH_DTYPE)
    for s, p in enumerate(sc["mps"]):
        if p is None:
            continue
        for f in ("id", "ref_kf_id", "descriptor", "client_id", "flags", "world_pos", "normal", "min_distance", "max_distance"):
            rec[s][f] = p[f]
        rec[s]["n_obs"] = len(p["obs"])
        for q, (k, i) in enumerate(p["obs"]):
            okf[s, q] = k; oi[s, q] = i
        for f in ("n_visible", "n_found", "replaced_by"):
            cnt[s][f] = p[f]
        for f, v in p["scratch"].items():
            scr[s][f] = v
    return rec, okf, oi, cnt, scr


def expected_state(corb, sc):
    rec, okf, oi, cnt, scr = mp_arrays(corb, sc)
    kf = [(np.asarray(k["flags"], np.uint8).tobytes(), np.asarray(k["mp_id"], np.uint64).tobytes()) for k in sc["kfs"]]
    return kf, rec.tobytes(), okf.tobytes(), oi.tobytes(), cnt.tobytes(), scr.tobytes()


def state(KF, MP):
    """what the records hold: (flags, ids) per keyframe slot and the map-point arrays; the rest of the keyframe records (features, meta) separately"""
    cap = MP.capacity
    rec, okf, oi = MP.get(0, cap)
    kf = []; rest = []
    for s in range(KF.capacity):
        g = KF.get(s)
        kf.append((g["flags"].tobytes(), KF.get_map_points(s).tobytes()))
        rest.append((g["kp"].tobytes(), g["desc"].tobytes(), g["u_right"].tobytes(), g["depth"].tobytes(), KF.get_meta(s).tobytes()))
    return (kf, rec.tobytes(), okf.tobytes(), oi.tobytes(), MP.get_counters(0, cap).tobytes(), MP.get_scratch(0, cap).tobytes()), rest

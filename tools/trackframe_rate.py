"""The initial pose of a tracked frame on records, one GPU: the one call (corb_track_with_motion_model, corb_track_reference_keyframe) beside the route it replaces,
on the one-client map of tools/tracklocal_rate.py.

The map: one client's synth.ba_problem_fast map -- about 2000 features per keyframe, 300 keyframes.  The last frame is a copy of a keyframe's record (it holds that
keyframe's points, and that keyframe is the reference keyframe), the current frame a copy of the next keyframe's features.  Every map point has a random descriptor
and a feature carries its point's, so both matchers have real work; the vocabulary is a random full tree (k = 4, L = 5: four nodes at levelsup 4).

Routes, alternating call by call in the same process on the same data; every call ends in a synchronise, so the host clock around it is the call's time (no kernel
times are taken here).  Before every call, untimed, both frames' records (ids, flags, pose) are put back.
  motion_model / one_call   : KeyFrameStore.TrackWithMotionModel(check_replaced, Tlr given), the retry not taken
  motion_model / two_calls  : TrackSearchLastFrame + TrackPoseOptimization(discard) with the poses already on the host -- the bar: the one call's median may exceed
                              this median by no more than this route's own 10th - 90th spread, or the gating of the wide search has failed
  motion_model / equivalent : the same plus the host upkeep that makes it equivalent: the counters of the last frame's points (CheckReplacedInLastFrame), the
                              reference keyframe's pose, both SetPose, the fill, and the n_obs of the held points for nmatchesMap
  reference_keyframe / one_call   : KeyFrameStore.TrackReferenceKeyFrame (the FeatureVectors are in the records)
  reference_keyframe / equivalent : SearchByBoW on slots, the keyframe's ids fetched, gathered and uploaded, flags and pose set, TrackPoseOptimization(discard), n_obs
Before timing, one_call and equivalent must leave equal frame records, matches and counts.  Prints one JSON line (and writes it to --out), times in ms as
median [p10, p90] over --calls calls after --warmup.
usage: python tools/trackframe_rate.py [--kf 300] [--ppk 360] [--calls 200] [--warmup 20] [--out profiles/trackframe_rate.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import corbload  # noqa: E402

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
FRAME_ID = 900000008


def stats(ts, calls):
    ts = np.sort(np.array(ts)) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(ts[int(0.1 * len(ts))]), 4), p90_ms=round(float(ts[int(0.9 * len(ts))]), 4), calls=calls)


def gemm4(A, B):
    """cv::gemm on CV_32F: a double sum over k ascending, rounded once"""
    C = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            s = np.float64(0.0)
            for k in range(4):
                s = s + np.float64(A[i, k]) * np.float64(B[k, j])
            C[i, j] = np.float32(s)
    return C


def random_vocabulary(corb, rng, k=4, L=5):
    parent, leaf = [], []
    level = [0]
    for d in range(1, L + 1):
        nxt = []
        for p in level:
            for _ in range(k):
                parent.append(p); leaf.append(1 if d == L else 0); nxt.append(len(parent))
        level = nxt
    n = len(parent)
    return corb.Vocabulary(k, L, parent, leaf, rng.integers(0, 256, (n, 32), dtype=np.uint8), np.where(np.array(leaf) > 0, rng.uniform(0.5, 3.0, n), 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=300)
    ap.add_argument("--ppk", type=int, default=360, help="new points per keyframe; a point is seen by ~5.5 keyframes")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trackframe_rate.json"))
    a = ap.parse_args()
    corb = corbload.load_pkg()
    from corb_slam_amd import synth
    prob = synth.ba_problem_fast(n_clients=1, kf_per_client=a.kf, pts_per_kf=a.ppk, seed=1000, obs_range=(3, 8), window=6)
    arr = synth.map_arrays(prob, a.kf, a.ppk)
    K, n_mp = len(arr["meta"]), len(arr["mp_records"])
    off = arr["feat_off"]; feats = np.diff(off)
    out = dict(config="one client, %d keyframes, %d map points, features per keyframe median %d / max %d" % (K, n_mp, int(np.median(feats)), int(feats.max())),
               timing="host to host, every call ends in a synchronise; routes alternate call by call; kernel times not measured")
    if corb.device_count() < 1:
        raise SystemExit("no MI355X visible")
    rng = np.random.default_rng(7)
    rec = arr["mp_records"]
    rec["descriptor"] = rng.integers(0, 256, (n_mp, 32), dtype=np.uint8)
    order = np.argsort(rec["id"]); sorted_ids = rec["id"][order]
    pos = np.searchsorted(sorted_ids, arr["mp_id"]); pos[pos >= n_mp] = 0
    slot = np.where(sorted_ids[pos] == arr["mp_id"], order[pos], -1)
    desc = rng.integers(0, 256, (len(arr["kp"]), 32), dtype=np.uint8)
    desc[slot >= 0] = rec["descriptor"][slot[slot >= 0]]
    ref = int(np.linspace(0, K - 2, 16).astype(int)[8]); nxt = ref + 1
    KF = corb.KeyFrameStore(K, arr["max_features"]); MP = corb.MapPointStore(n_mp, arr["max_obs"]); FR = corb.KeyFrameStore(2, arr["max_features"])
    KF.put_batch(0, arr["meta"], off, arr["kp"], desc, arr["ur"], None, arr["mp_id"])
    MP.put(0, rec, arr["obs_off"], arr["obs_kf"], arr["obs_idx"]); MP.build_index(0, n_mp)
    sl_l = slice(off[ref], off[ref + 1]); sl_c = slice(off[nxt], off[nxt + 1]); n_l = int(feats[ref]); n_c = int(feats[nxt])
    meta_l = arr["meta"][ref: ref + 1].copy(); meta_l["id"] = FRAME_ID - 1
    meta_c = arr["meta"][nxt: nxt + 1].copy(); meta_c["id"] = FRAME_ID
    FR.put_batch(0, np.concatenate([meta_l, meta_c]), np.array([0, n_l, n_l + n_c], np.int32), np.concatenate([arr["kp"][sl_l], arr["kp"][sl_c]]),
                 np.concatenate([desc[sl_l], desc[sl_c]]), np.concatenate([arr["ur"][sl_l], arr["ur"][sl_c]]), None,
                 np.concatenate([arr["mp_id"][sl_l], np.full(n_c, NONE, np.uint64)]))
    voc = random_vocabulary(corb, rng)
    KF.compute_bow([ref], voc, 4); FR.compute_bow([1], voc, 4)
    ids_l = np.array(arr["mp_id"][sl_l], np.uint64)
    KF.set_flags(ref, (slot[sl_l] >= 0).astype(np.uint8))
    m0 = arr["meta"][ref]
    cam = corb.TrackCamera.make(float(m0["fx"]), float(m0["fy"]), float(m0["cx"]), float(m0["cy"]), float(m0["bf"]), float(m0["bf"]) / float(m0["fx"]),
                                0.0, 2.0 * float(m0["cx"]), 0.0, 2.0 * float(m0["cy"]), (1.2 ** np.arange(8)).astype(np.float32))
    T_ref = arr["meta"]["Tcw"][ref].reshape(4, 4).astype(np.float32); T_cur = arr["meta"]["Tcw"][nxt].reshape(4, 4).astype(np.float32)
    Tlr = np.eye(4, dtype=np.float32)
    vel = (T_cur.astype(np.float64) @ np.linalg.inv(T_ref.astype(np.float64))).astype(np.float32)
    none_c = np.full(n_c, NONE, np.uint64); flags_l = np.zeros(n_l, np.uint8); flags_c = np.zeros(n_c, np.uint8)
    held_slots = slot[sl_l][slot[sl_l] >= 0]; lo, hi = int(held_slots.min()), int(held_slots.max())
    n_obs_all = rec["n_obs"]

    def reset():
        FR.set_map_points(0, ids_l); FR.set_flags(0, flags_l); FR.set_meta_raw(0, meta_l[0])
        FR.set_map_points(1, none_c); FR.set_flags(1, flags_c); FR.set_meta_raw(1, meta_c[0])

    def state(r_counts):
        return [FR.get_map_points(s).tobytes() for s in (0, 1)] + [FR.get(s)["flags"].tobytes() for s in (0, 1)] + [FR.get_meta(s).tobytes() for s in (0, 1)] + [repr(r_counts)]

    def slots_of(ids):
        p = np.searchsorted(sorted_ids, ids); p[p >= n_mp] = 0
        return np.where(sorted_ids[p] == ids, order[p], -1)

    def map_count(n_matches, outl):
        """the "Discard outliers" loop's counts on the host: the held points' n_obs come from the store"""
        held = FR.get_map_points(1); fl = FR.get(1)["flags"]
        s = slots_of(held); live = (s >= 0) & ((fl & 4) == 0)
        recs = MP.get(lo, hi - lo + 1)[0]                                                # the fetch a client without the records' n_obs has to make
        inside = live & (s >= lo) & (s <= hi)
        n_map = int((recs["n_obs"][s[inside] - lo] > 0).sum()) + int((n_obs_all[s[live & ~inside]] > 0).sum())
        return n_matches - int(outl.sum()), n_map

    # ---- TrackWithMotionModel ----
    def mm_one():
        r = FR.TrackWithMotionModel(1, 0, KF, ref, MP, cam, vel, FRAME_ID, Tlr=Tlr, sensor=1, check_replaced=True)
        return r["match"], (r["n_matches"], r["n_matches_kept"], r["n_matches_map"], bool(r["ok"]), bool(r["searched_wide"]))

    Tlw0 = gemm4(Tlr, T_ref); Tpred0 = gemm4(vel, Tlw0)

    def mm_two():
        m, n = FR.TrackSearchLastFrame(1, 0, MP, Tpred0, Tlw0, cam, 7.0, mono=False)
        FR.TrackPoseOptimization(1, MP, cam, Tpred0, discard_outliers=True)
        return m, n

    def mm_equivalent():
        c = MP.get_counters(lo, hi - lo + 1)                                             # CheckReplacedInLastFrame: the counters of the last frame's points
        rep = c["replaced_by"][held_slots - lo]
        if rep.any():
            ids = ids_l.copy(); ids[np.nonzero(slot[sl_l] >= 0)[0][rep != 0]] = rep[rep != 0] - np.uint64(1); FR.set_map_points(0, ids)
        Tlw = gemm4(Tlr, np.array(KF.get_meta(ref)["Tcw"], np.float32).reshape(4, 4))    # the reference keyframe's pose as it stands
        FR.set_meta(0, Tcw=Tlw)
        Tpred = gemm4(vel, Tlw)
        FR.set_meta(1, Tcw=Tpred)
        FR.set_map_points(1, none_c); FR.set_flags(1, flags_c)
        m, n = FR.TrackSearchLastFrame(1, 0, MP, Tpred, Tlw, cam, 7.0, mono=False)
        assert n >= 20
        T, outl, inl = FR.TrackPoseOptimization(1, MP, cam, Tpred, discard_outliers=True)
        kept, n_map = map_count(n, outl)
        return m, (n, kept, n_map, n_map >= 10, False)

    # ---- TrackReferenceKeyFrame ----
    def rk_one():
        r = FR.TrackReferenceKeyFrame(1, 0, KF, ref, MP, cam, FRAME_ID, voc=None, sensor=1)
        return r["match"], (r["n_matches"], r["n_matches_kept"], r["n_matches_map"], bool(r["ok"]), False)

    def rk_equivalent():
        m, n = KF.SearchByBoW(ref, FR, 1, nnratio=0.7, checkOri=True, variant=0)
        assert n >= 15
        kf_ids = KF.get_map_points(ref)
        ids = np.where(m >= 0, kf_ids[np.maximum(m, 0)], NONE)
        FR.set_map_points(1, ids); FR.set_flags(1, flags_c)
        Tlw = np.array(FR.get_meta(0)["Tcw"], np.float32).reshape(4, 4)
        FR.set_meta(1, Tcw=Tlw)
        T, outl, inl = FR.TrackPoseOptimization(1, MP, cam, Tlw, discard_outliers=True)
        kept, n_map = map_count(n, outl)
        return m, (n, kept, n_map, n_map >= 10, False)

    def timed(routes):
        ts = {k: [] for k in routes}
        for i in range(a.warmup + a.calls):
            for name, fn in routes.items():
                reset()
                t0 = time.perf_counter(); fn(); t = time.perf_counter() - t0
                if i >= a.warmup:
                    ts[name].append(t)
        return {k: stats(v, a.calls) for k, v in ts.items()}

    for section, one, equivalent, bare in (("motion_model", mm_one, mm_equivalent, mm_two), ("reference_keyframe", rk_one, rk_equivalent, None)):
        reset(); m_new, c_new = one(); s_new = state(c_new)
        reset(); m_old, c_old = equivalent(); s_old = state(c_old)
        assert np.array_equal(m_new, m_old) and s_new == s_old, "%s: the two routes leave different bytes: %r / %r" % (section, c_new, c_old)
        routes = dict(one_call=one, equivalent=equivalent)
        if bare:
            routes["two_calls"] = bare
        res = timed(routes)
        res["routes_leave_equal_bytes"] = True
        res["counts"] = dict(features=n_c, last_features=n_l, matches=c_new[0], kept=c_new[1], in_map=c_new[2], ok=c_new[3], searched_wide=c_new[4])
        if bare:
            spread = res["two_calls"]["p90_ms"] - res["two_calls"]["p10_ms"]
            res["one_call_within_two_calls_spread"] = res["one_call"]["median_ms"] <= res["two_calls"]["median_ms"] + spread
        out[section] = res
    voc.close(); KF.close(); MP.close(); FR.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

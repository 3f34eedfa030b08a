"""GPU parity of the calls on device-resident records on seeded random scenes: the tracking-thread calls (TrackSearchLastFrame, TrackPoseOptimization,
TrackSearchLocalPoints), the keyframe matchers on records (TrackSearchReloc, SearchByProjectionScw, SearchBySim3, Fuse), MapPoint::Replace and
ComputeDistinctiveDescriptors.  Every case builds records with random holes (features without a point, bad and unobserved points, ids the store does not know,
outlier and discarded flags and both), calls the record route, and compares it with the oracle on the flat views tests/records_reference.py derives from the
same arrays, and the records read back with the writes the reference would leave.  Everything but a pose is bit for bit; poses carry the bars of
tests/test_gpu_random_ba.py plus bit equality with the host-pointer batch call on the in-order edge list.  Sizes sit at the wave (64), the 1024-feature chunk of
the edge gather and the 2048-feature boundary; tests/test_random_cases.py checks on the CPU that the lists reach them and that the oracle alone answers non-trivially."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import newpoints_reference as NP  # noqa: E402
import records_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-4                                           # tests/test_gpu_random_ba.py
NONE = R.NONE
UNKNOWN0 = 1 << 60                                    # ids from here on are in no store
W, H = 1241.0, 376.0
SCALE = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
LOGS = float(np.float32(np.log(np.float32(1.2))))
INV_S2 = np.array([1.0 / (1.2 ** k) ** 2 for k in range(8)]).astype(np.float32)      # synth.pose_opt_problem's inv_sigma2 per octave
GOOD, NO_POINT, BAD_POINT, UNKNOWN, OUTLIER, DISCARDED, BOTH = range(7)              # what a feature of a generated frame holds


def _id(prefix, c, keys):
    return "%s-%03d-" % (prefix, c["i"]) + "-".join("%s_%s" % (k, c[k]) for k in keys)


def _ids(n, rng, collide_cells=0):
    """map-point ids that are not slots; collide_cells: ids whose table of that many cells has a probe chain across its end"""
    if collide_cells:
        return R.colliding_ids(n, collide_cells, rng)
    return np.uint64(1000) + np.uint64(3) * np.arange(n, dtype=np.uint64)


def _records(n, ids, world, desc, rng, unobserved=0.1):
    rec = np.zeros(n, R.MP_RECORD_DTYPE)
    rec["id"] = ids; rec["world_pos"] = world; rec["descriptor"] = desc; rec["client_id"] = 1; rec["ref_kf_id"] = 1
    rec["n_obs"] = rng.random(n) >= unobserved
    return rec


def _hold(kinds, point_of, rec, rng):
    """per-feature ids and flag bytes of a frame whose feature i holds point slot point_of[i] in the way kinds[i] says; marks the bad points in rec"""
    n = len(kinds)
    ids = np.where(kinds == NO_POINT, NONE, rec["id"][point_of]).astype(np.uint64)
    unk = kinds == UNKNOWN
    ids[unk] = np.uint64(UNKNOWN0) + rng.permutation(4 * n)[: int(unk.sum())].astype(np.uint64)
    rec["flags"][point_of[kinds == BAD_POINT]] |= R.MP_BAD
    fl = np.zeros(n, np.uint8)
    fl[(kinds == OUTLIER) | (kinds == BOTH)] |= R.OUTLIER; fl[(kinds == DISCARDED) | (kinds == BOTH)] |= R.DISCARDED
    return ids, fl


def _obs_lists(rec, kf_id=1):
    return [[(kf_id, i)] if rec["n_obs"][i] else [] for i in range(len(rec))]


# ================================================================ A. the tracking thread ================================================================
_r = np.random.default_rng(4700)
TRACK_POSE_CASES = [dict(i=i, seed=47000 + i, n=n, edges=e, F=n + df, discard=bool(i & 1), collide=False) for i, (n, e, df) in
                    enumerate([(70, 0, 0), (64, 2, 1), (65, 3, 37), (70, 9, 0), (63, 10, 1), (70, 11, 37)])]
TRACK_POSE_CASES += [dict(i=6 + j, seed=47006 + j, n=n, edges=int(n * _r.uniform(0.4, 0.7)), F=n + (0, 1, 37)[j % 3], discard=bool(j & 1), collide=False)
                     for j, n in enumerate([63, 64, 65, 1023, 1024, 1025, 2049, 3000])]
TRACK_POSE_CASES += [dict(i=14, seed=47014, n=1500, edges=800, F=1537, discard=False, collide=True)]
TRACK_LAST_CASES = [dict(i=i, seed=47100 + i, n_cur=a, n_last=b, th=float(_r.choice([7.0, 15.0])), nnratio=float(_r.choice([0.7, 0.9])), mono=bool(_r.integers(0, 2)),
                         ori=bool(_r.integers(0, 2)), collide=False) for i, (a, b) in enumerate([(40, 63), (63, 40), (64, 700), (65, 64), (700, 2100), (2100, 65), (2900, 2100)])]
TRACK_LAST_CASES += [dict(i=7, seed=47107, n_cur=700, n_last=2100, th=7.0, nnratio=0.9, mono=False, ori=True, collide=True),
                     dict(i=8, seed=47108, n_cur=63, n_last=2900, th=15.0, nnratio=0.7, mono=True, ori=False, collide=False)]
TRACK_LOCAL_CASES = [dict(i=i, seed=47200 + i, n_cur=a, n_local=b, th=float(_r.choice([1.0, 3.0])), nnratio=float(_r.choice([0.6, 0.8])), only_bad=False, collide=False)
                     for i, (a, b) in enumerate([(40, 63), (63, 65), (64, 40), (65, 700), (700, 2100), (2100, 64), (2900, 2100)])]
TRACK_LOCAL_CASES += [dict(i=7, seed=47207, n_cur=2100, n_local=700, th=1.0, nnratio=0.8, only_bad=True, collide=False),
                      dict(i=8, seed=47208, n_cur=700, n_local=65, th=1.0, nnratio=0.8, only_bad=False, collide=True),
                      dict(i=9, seed=47211, n_cur=65, n_local=2900, th=3.0, nnratio=0.6, only_bad=False, collide=False)]
# ================================================================ B. keyframe matchers on records ================================================================
REC_RELOC_CASES = [dict(i=i, seed=47300 + i, n=n, cur_smaller=bool(i & 1), span=float(_r.choice([1.0, 0.3])), th=float(_r.choice([10.0, 3.0])), dist=int(_r.choice([100, 64])),
                        ori=bool(_r.integers(0, 2))) for i, n in enumerate([50, 64, 600, 2100])]
REC_SCW_CASES = [dict(i=i, seed=47400 + i, n=n, span=sp, th=float(_r.choice([10.0, 4.0])), scale=float(np.float32(_r.choice([1.0, 1.03]))))
                 for i, (n, sp) in enumerate([(40, 1.0), (63, 0.3), (65, 1.0), (600, 0.3), (2100, 1.0)])]
REC_SIM3_CASES = [dict(i=i, seed=47500 + i, n=n, span=sp, max_obs=int(_r.choice([3, 5, 8]))) for i, (n, sp) in enumerate([(40, 1.0), (63, 1.0), (65, 0.3), (600, 1.0), (2100, 0.3)])]
# later: half of the points have an observer after KF2 (with max_obs = 2 their lists are full: the "no room" path); without it every list has room
REC_FUSE_CASES = [dict(i=i, seed=47600 + i, n=n, span=sp, apply=ap, max_obs=O, later=True, th=float(_r.choice([3.0, 4.0])))
                  for i, (n, sp, ap, O) in enumerate([(40, 1.0, True, 8), (63, 0.3, False, 2), (65, 1.0, True, 2), (600, 0.3, True, 8), (2100, 1.0, True, 8), (600, 1.0, False, 8)])]
REC_FUSE_CASES += [dict(i=6, seed=47606, n=600, span=1.0, apply=True, max_obs=2, later=False, th=4.0)]
# ================================================================ C. Replace and distinctive descriptors ================================================================
REPLACE_CASES = [dict(i=i, seed=47700 + i, merged=L) for i, L in enumerate([1, 2, 63, 64, 65, 80])]
DISTINCTIVE_SIZES = [1, 2, 3, 4, 63, 64, 0, 65, 128, 1023, 1024]                                   # (an empty point between two full ones)
DISTINCTIVE_SEED = 47800
del _r


def _camera(corb, k):
    return corb.TrackCamera.make(k["fx"], k["fy"], k["cx"], k["cy"], k["bf"], float(np.float32(k["bf"]) / np.float32(k["fx"])), 0.0, W, 0.0, H, SCALE)


def _put_map(corb, rec, lists, max_obs=2, index=True):
    MP = corb.MapPointStore(len(rec), max_obs)
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    flat = [o for l in lists for o in l]
    rec = rec.copy(); rec["n_obs"] = np.diff(off)
    MP.put(0, rec, off, np.array([a for a, _ in flat], np.uint64), np.array([b for _, b in flat], np.uint32))
    if index:
        MP.build_index(0, len(rec))
    return MP


def _put_frame(KF, slot, fr, intr, Tcw, kid):
    KF.put(slot, fr["keys"], fr["desc"], fr["ur"], None, keyframe_id=kid)
    KF.set_meta(slot, id=kid, client_id=1, flags=0, fx=intr["fx"], fy=intr["fy"], cx=intr["cx"], cy=intr["cy"], bf=intr["bf"], nlevels=8,
                Tcw=np.asarray(Tcw, np.float32).reshape(16), inv_level_sigma2=np.concatenate([INV_S2, np.zeros(8, np.float32)]))
    KF.set_map_points(slot, fr["mp_id"])
    KF.set_flags(slot, fr["flags"])


def _frame_view(fr, claimed):
    return dict(keys_un=fr["keys"], u_right=fr["ur"], desc=fr["desc"], claimed=claimed, min_x=0.0, min_y=0.0, max_x=W, max_y=H, scale=SCALE)


# ---------------------------------------------------------------- TrackPoseOptimization ----------------------------------------------------------------
def track_pose_problem(synth, c):
    rng = np.random.default_rng(c["seed"])
    n, E = c["n"], c["edges"]
    q = synth.pose_opt_problem(seed=c["seed"], n=n, outlier_frac=float(rng.uniform(0.1, 0.3)))
    truth = q["outlier_truth"]
    if E >= 10 and E < 20:                            # a small graph holds two of the gross observations and otherwise clean ones
        edge = np.concatenate([rng.permutation(np.nonzero(truth)[0])[:2], rng.permutation(np.nonzero(~truth)[0])[: E - 2]])
    else:
        edge = rng.permutation(n)[:E]
    kinds = rng.choice([NO_POINT, BAD_POINT, UNKNOWN, DISCARDED, BOTH], n)
    kinds[edge] = np.where(rng.random(E) < 0.2, OUTLIER, GOOD)                       # (mvbOutlier of a held point is reset, it carries an edge)
    kinds[edge[-1:]] = OUTLIER
    q["obs"][edge[:1], 2] = -1.0                      # at least one monocular edge
    keys = np.zeros(n, R.KP_DTYPE); keys["x"] = q["obs"][:, 0]; keys["y"] = q["obs"][:, 1]
    keys["octave"] = np.rint(np.log(1.0 / q["inv_sigma2"].astype(np.float64)) / (2 * np.log(1.2))).astype(np.int32)
    assert np.array_equal(INV_S2[keys["octave"]], q["inv_sigma2"])
    ids = _ids(n, rng, R.id_table_cells(n) if c["collide"] else 0)
    if c["collide"]:                                  # the colliding ids are the first ones: spread them over the frame
        ids = ids[rng.permutation(n)]
    rec = _records(n, ids, q["points"], rng.integers(0, 256, (n, 32), dtype=np.uint8), rng)
    mp_id, flags = _hold(kinds, np.arange(n), rec, rng)
    fr = dict(keys=keys, ur=q["obs"][:, 2].copy(), desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), mp_id=mp_id, flags=flags)
    return dict(q=q, fr=fr, rec=rec, lists=_obs_lists(rec), slot_of=R.slot_dict(rec))


def track_pose_reference(pyorc, p):
    """the in-order edge list of the frame and what the oracle makes of it: (edges, result of pyorc.ba_solve_staged or None for fewer than 3 edges)"""
    q, fr = p["q"], p["fr"]
    e = R.pose_edges(fr["keys"], fr["ur"], fr["mp_id"], fr["flags"], p["rec"], p["slot_of"], INV_S2)
    if e["klass"] == 0:
        return e, None
    E = len(e["feat"])
    ed = np.zeros(E, pyorc.EDGE_DTYPE)
    ed["pose"] = 0; ed["point"] = np.arange(E); ed["u"] = e["obs"][:, 0]; ed["v"] = e["obs"][:, 1]; ed["ur"] = e["obs"][:, 2]; ed["inv_sigma2"] = e["w"]
    stages = pyorc.POSE_OPT_STAGES[: e["klass"]]     # fewer than 10 edges: the loop breaks after its first round (Optimizer.cc:470-471)
    return e, pyorc.ba_solve_staged(q["Tcw0"].reshape(1, 16), np.zeros(1, np.uint8), e["points"], np.ones(E, np.uint8), ed, q["fx"], q["fy"], q["cx"], q["cy"], q["bf"], stages)


@pytest.mark.parametrize("c", TRACK_POSE_CASES, ids=[_id("tpose", c, ("n", "edges", "F", "discard", "collide")) for c in TRACK_POSE_CASES])
def test_track_pose_optimization_random_case(corb, pyorc, synth, c):
    p = track_pose_problem(synth, c)
    q, fr, n = p["q"], p["fr"], c["n"]
    e, r = track_pose_reference(pyorc, p)
    assert len(e["feat"]) == c["edges"]
    KF = corb.KeyFrameStore(3, c["F"]); MP = _put_map(corb, p["rec"], p["lists"])
    T_rec0 = np.eye(4, dtype=np.float32); T_rec0[0, 3] = 9.0
    _put_frame(KF, 1, fr, q, T_rec0, 5)
    cam = _camera(corb, q)
    T, outl, inl = KF.TrackPoseOptimization(1, MP, cam, q["Tcw0"], discard_outliers=c["discard"])
    rej = np.zeros(len(e["feat"]), bool)
    if e["klass"] == 0:                               # `if(nInitialCorrespondences<3) return 0;`: the pose passes through, SetPose is not reached
        assert np.array_equal(np.asarray(T).reshape(16), q["Tcw0"].reshape(16)) and inl == 0 and not outl.any()
        assert np.array_equal(np.asarray(KF.get_meta(1)["Tcw"]).reshape(16), T_rec0.reshape(16))
    else:
        Tb, ob, ib = corb.Optimizer.PoseOptimizationBatch([(q["Tcw0"], e["points"], e["obs"], e["w"])], q["fx"], q["fy"], q["cx"], q["cy"], q["bf"])[0]
        rej = np.asarray(r["outlier"], bool)
        full = np.zeros(n, bool); full[e["feat"]] = rej
        print("%s: edges %d, oracle outliers %d, |T - oracle| %.3g" % (c["i"], len(rej), rej.sum(), np.abs(np.asarray(T) - r["poses"][0]).max()))
        assert np.array_equal(np.asarray(T).reshape(16), np.asarray(Tb).reshape(16))                       # the same sums in the same order as the in-order edge list
        assert np.array_equal(np.asarray(ob, bool), rej) and ib == len(rej) - int(rej.sum())
        assert np.array_equal(outl, full) and inl == len(rej) - int(rej.sum())                              # the flags sit on the features the oracle flags
        assert np.abs(np.asarray(T).reshape(4, 4) - r["poses"][0]).max() <= RTOL * max(1.0, np.abs(r["poses"][0]).max())
        assert np.array_equal(np.asarray(KF.get_meta(1)["Tcw"]).reshape(16), np.asarray(T).reshape(16))    # pFrame->SetPose
    assert np.array_equal(KF.get(1)["flags"], R.pose_writes(fr["flags"], e["feat"], rej, c["discard"]))
    assert np.array_equal(KF.get_map_points(1), fr["mp_id"])
    KF.close(); MP.close()


# ---------------------------------------------------------------- TrackSearchLastFrame ----------------------------------------------------------------
def _cut(s, n_cur):
    cur = s["cur"]
    return dict(keys=cur["keys_un"][:n_cur].copy(), ur=cur["u_right"][:n_cur].copy(), desc=cur["desc"][:n_cur].copy())


def _pool_holders(rng, n_cur, first_slot, n_pool, frac):
    """a fraction of the frame's features hold points of a pool of the map (slots first_slot ..), one feature per point: (kinds, point_of)"""
    kinds = np.full(n_cur, NO_POINT); point_of = np.full(n_cur, first_slot)
    h = rng.permutation(n_cur)[: min(max(3, int(n_cur * frac)), n_pool)]
    kinds[h] = rng.choice([GOOD, GOOD, GOOD, BAD_POINT, UNKNOWN, OUTLIER, DISCARDED, BOTH], len(h))
    point_of[h] = first_slot + rng.permutation(n_pool)[: len(h)]
    return kinds, point_of


def track_last_problem(synth, c):
    rng = np.random.default_rng(c["seed"])
    nc, nl = c["n_cur"], c["n_last"]
    s = synth.tracking_scene(seed=c["seed"], n=max(nc, nl))
    n_pool = max(8, nc // 6); n = nl + n_pool        # slots 0 .. nl-1: the last frame's points; the rest: what the current frame holds already
    ids = _ids(n, rng, R.id_table_cells(n) if c["collide"] else 0)
    world = np.concatenate([s["last"]["world"][:nl], rng.normal(0, 5, (n_pool, 3)).astype(np.float32)])
    rec = _records(n, ids, world, np.concatenate([s["last_desc"][:nl], rng.integers(0, 256, (n_pool, 32), dtype=np.uint8)]), rng)
    kl = rng.choice([GOOD] * 12 + [NO_POINT, NO_POINT, BAD_POINT, UNKNOWN, OUTLIER, DISCARDED, BOTH], nl)
    last_keys = np.zeros(nl, R.KP_DTYPE); last_keys["angle"] = s["last"]["angle"][:nl]; last_keys["octave"] = s["last"]["octave"][:nl]
    l_id, l_fl = _hold(kl, np.arange(nl), rec, rng)
    last = dict(keys=last_keys, ur=np.full(nl, -1, np.float32), desc=s["last_desc"][:nl].copy(), mp_id=l_id, flags=l_fl)
    kc, pc = _pool_holders(rng, nc, nl, n_pool, 0.08)
    cur = _cut(s, nc); cur["mp_id"], cur["flags"] = _hold(kc, pc, rec, rng)
    return dict(s=s, cur=cur, last=last, rec=rec, lists=_obs_lists(rec), slot_of=R.slot_dict(rec))


def track_last_reference(pyorc, c, p):
    s, cur, last = p["s"], p["cur"], p["last"]
    lastp, ldesc, claimed = R.last_frame_view(last["keys"], last["mp_id"], last["flags"], cur["mp_id"], cur["flags"], p["rec"], p["slot_of"])
    m, n = pyorc.search_by_projection_frame(_frame_view(cur, claimed), s["Tcw"], s["Tlw"], s["fx"], s["fy"], s["cx"], s["cy"], s["bf"], s["mb"], lastp, ldesc,
                                            c["th"], int(c["mono"]), int(c["ori"]))
    return m, n, lastp, claimed


@pytest.mark.parametrize("c", TRACK_LAST_CASES, ids=[_id("tlast", c, ("n_cur", "n_last", "th", "nnratio", "mono", "ori", "collide")) for c in TRACK_LAST_CASES])
def test_track_search_last_frame_random_case(corb, pyorc, synth, c):
    p = track_last_problem(synth, c)
    s, cur, last = p["s"], p["cur"], p["last"]
    m_ref, n_ref, _, _ = track_last_reference(pyorc, c, p)
    n_max = max(c["n_cur"], c["n_last"])
    KF = corb.KeyFrameStore(3, n_max + (0, 1, 37)[c["i"] % 3]); MP = _put_map(corb, p["rec"], p["lists"])
    _put_frame(KF, 2, last, s, s["Tlw"], 8); _put_frame(KF, 0, cur, s, s["Tcw"], 9)
    m, n = KF.TrackSearchLastFrame(0, 2, MP, s["Tcw"], s["Tlw"], _camera(corb, s), c["th"], mono=c["mono"], nnratio=c["nnratio"], check_orientation=c["ori"])
    assert n == n_ref and np.array_equal(m, m_ref) and n_ref > 0
    ids, fl = R.matched_writes(cur["mp_id"], cur["flags"], m_ref, last["mp_id"])
    assert np.array_equal(KF.get_map_points(0), ids) and np.array_equal(KF.get(0)["flags"], fl)
    assert np.array_equal(KF.get_map_points(2), last["mp_id"]) and np.array_equal(KF.get(2)["flags"], last["flags"])       # the last frame is untouched
    KF.close(); MP.close()


# ---------------------------------------------------------------- TrackSearchLocalPoints ----------------------------------------------------------------
def track_local_problem(synth, c):
    rng = np.random.default_rng(c["seed"])
    nc, nq = c["n_cur"], c["n_local"]
    n = max(nc, nq)
    s = synth.tracking_scene(seed=c["seed"], n=n)
    cells = R.id_table_cells(nc)
    n_rec = n if not c["collide"] else max(n, cells // 4 + 1)                         # (the store's table then has as many cells as the call's in-frame table)
    ids = _ids(n_rec, rng, cells if c["collide"] else 0)
    assert not c["collide"] or R.id_table_cells(n_rec) == cells
    world = np.concatenate([s["last"]["world"], rng.normal(0, 5, (n_rec - n, 3)).astype(np.float32)])
    rec = _records(n_rec, ids, world, np.concatenate([s["last_desc"], rng.integers(0, 256, (n_rec - n, 32), dtype=np.uint8)]), rng)
    # normal and distance range as MapPoint::UpdateNormalAndDepth leaves them for an observer at the last frame's centre; a sixth of the points is out of range
    Tl = s["Tlw"].astype(np.float64); C0 = -Tl[:3, :3].T @ Tl[:3, 3]
    PO = world.astype(np.float64) - C0; dist = np.linalg.norm(PO, axis=1)
    octv = np.concatenate([s["last"]["octave"], np.zeros(n_rec - n, np.int32)])
    rec["normal"] = (PO / dist[:, None]).astype(np.float32)
    rec["max_distance"] = (dist * SCALE[octv] * 1.3 * np.where(rng.random(n_rec) < 1 / 6, 0.3, 1.0)).astype(np.float32)
    rec["min_distance"] = (rec["max_distance"] / SCALE[7] / np.float32(1.5)).astype(np.float32)
    # the frame holds a quarter of its features' worth of map points (TrackWithMotionModel's matches), in every way a feature can hold one
    kinds = np.full(nc, NO_POINT); point_of = np.zeros(nc, np.int64)
    h = rng.permutation(nc)[: max(4, nc // 4)]
    kinds[h] = BAD_POINT if c["only_bad"] else rng.choice([GOOD, GOOD, GOOD, BAD_POINT, UNKNOWN, OUTLIER, DISCARDED, BOTH], len(h))
    point_of[h] = np.arange(len(h)) if c["collide"] else rng.permutation(n)[: len(h)]           # (collide: the frame holds the colliding ids)
    cur = _cut(s, nc); cur["mp_id"], cur["flags"] = _hold(kinds, point_of, rec, rng)
    if not c["only_bad"]:                             # a discarded feature whose point is bad as well: still seen in the frame, and it stays in the record
        d = h[kinds[h] == DISCARDED][:1]; rec["flags"][point_of[d]] |= R.MP_BAD
    local = rng.permutation(n)[: nq - 3]
    local_ids = np.concatenate([rec["id"][local], np.uint64(UNKNOWN0 + 77) + np.arange(3, dtype=np.uint64)])[rng.permutation(nq)]
    return dict(s=s, cur=cur, rec=rec, lists=_obs_lists(rec), slot_of=R.slot_dict(rec), local_ids=local_ids)


def track_local_reference(pyorc, c, p):
    s, cur, rec = p["s"], p["cur"], p["rec"]
    after, cand, claimed = R.local_points_view(cur["mp_id"], cur["flags"], p["local_ids"], rec, p["slot_of"])
    ls = np.maximum(R.slots_of(p["local_ids"], p["slot_of"]), 0)
    exp = pyorc.is_in_frustum(s["Tcw"], rec["world_pos"][ls], rec["normal"][ls], rec["min_distance"][ls], rec["max_distance"][ls], s["fx"], s["fy"], s["cx"], s["cy"], s["bf"],
                              0.0, W, 0.0, H, LOGS, 8)
    exp["valid"] &= cand; exp["claims"] = (rec["n_obs"][ls] > 0) & exp["valid"].astype(bool)
    for k in ("proj_x", "proj_y", "proj_xr", "view_cos", "level"):
        exp[k] = np.where(exp["valid"], exp[k], 0)
    desc = np.where(exp["valid"][:, None].astype(bool), rec["descriptor"][ls], 0).astype(np.uint8)
    m, n = pyorc.search_by_projection_map(_frame_view(cur, claimed), exp, desc, c["th"], c["nnratio"])
    return m, n, exp, after


@pytest.mark.parametrize("c", TRACK_LOCAL_CASES, ids=[_id("tlocal", c, ("n_cur", "n_local", "th", "nnratio", "only_bad", "collide")) for c in TRACK_LOCAL_CASES])
def test_track_search_local_points_random_case(corb, pyorc, synth, c):
    p = track_local_problem(synth, c)
    s, cur = p["s"], p["cur"]
    m_ref, n_ref, exp, after = track_local_reference(pyorc, c, p)
    KF = corb.KeyFrameStore(2, c["n_cur"] + (0, 1, 37)[c["i"] % 3]); MP = _put_map(corb, p["rec"], p["lists"])
    _put_frame(KF, 1, cur, s, s["Tcw"], 9)
    m, n, inview, tr = KF.TrackSearchLocalPoints(1, MP, p["local_ids"], _camera(corb, s), s["Tcw"], LOGS, th=c["th"], nnratio=c["nnratio"], want_tracked=True)
    assert np.array_equal(tr["valid"], exp["valid"]) and inview == int(exp["valid"].sum()) and 0 < inview < c["n_local"]
    for k in ("proj_x", "proj_y", "proj_xr", "view_cos"):
        assert np.array_equal(tr[k].view(np.uint32), exp[k].view(np.uint32)), k
    assert np.array_equal(tr["level"], exp["level"]) and np.array_equal(tr["claims"], exp["claims"])
    assert n == n_ref and np.array_equal(m, m_ref) and n_ref > 0
    ids, fl = R.matched_writes(after, cur["flags"], m_ref, p["local_ids"])
    assert np.array_equal(KF.get_map_points(1), ids) and np.array_equal(KF.get(1)["flags"], fl)
    KF.close(); MP.close()


# ---------------------------------------------------------------- the keyframe scenes ----------------------------------------------------------------
def _kf_frame(k, mp_id, flags=None):
    n = len(k["keys_un"])
    return dict(keys=k["keys_un"], ur=k["u_right"], desc=k["desc"], mp_id=np.asarray(mp_id, np.uint64), flags=np.zeros(n, np.uint8) if flags is None else flags)


def _kf_records(first_id, pts, desc, rng, kid):
    rec = _records(len(pts), np.uint64(first_id) + np.uint64(3) * np.arange(len(pts), dtype=np.uint64), pts["world"], desc, rng, unobserved=0.0)
    for k in ("normal", "min_distance", "max_distance"):
        rec[k] = pts[k]
    rec["ref_kf_id"] = kid
    return rec


def rec_reloc_problem(synth, c):
    """CurrentFrame = KF2's features, pKF = KF1: features of pKF without a MapPoint, with a bad one, with one the frame holds already (sAlreadyFound), with an id the
    store does not know; frame features that hold pKF's points, unknown ids, and discarded ones (which hold nothing: their point stays a candidate)"""
    rng = np.random.default_rng(c["seed"]); n = c["n"]
    sc = synth.keyframe_scene(c["seed"], n=n, span=c["span"])
    rec = _kf_records(1000, sc["pts1"], sc["desc1"], rng, 11)
    cause = rng.choice([GOOD] * 14 + [NO_POINT, BAD_POINT, UNKNOWN, 7, 7, 8], n)                   # 7: already found by the frame, 8: held by a discarded frame feature
    ids1, _ = _hold(np.where(cause >= 7, GOOD, cause), np.arange(n), rec, rng)
    ci = rng.permutation(np.nonzero(sc["claimed2"])[0]) if sc["claimed2"].sum() >= 4 else rng.permutation(n)[: max(4, n // 10)]
    found = np.nonzero(cause == 7)[0][: len(ci) // 2]; disc = np.nonzero(cause == 8)[0][: len(ci) // 4]
    ids2 = np.full(n, NONE, np.uint64); fl2 = np.zeros(n, np.uint8)
    ids2[ci] = np.uint64(UNKNOWN0) + ci.astype(np.uint64)                                          # held ids the store does not know
    ids2[ci[: len(found)]] = rec["id"][found]
    ids2[ci[len(found): len(found) + len(disc)]] = rec["id"][disc]; fl2[ci[len(found): len(found) + len(disc)]] = R.DISCARDED
    ids2[ci[-1]] = rec["id"][found[0]] if len(found) else ids2[ci[-1]]; fl2[ci[-1]] |= R.OUTLIER   # an outlier mark does not unhold a point
    return dict(sc=sc, rec=rec, lists=_obs_lists(rec, 11), slot_of=R.slot_dict(rec), kf=_kf_frame(sc["kf1"], ids1), cur=_kf_frame(sc["kf2"], ids2, fl2))


def rec_reloc_reference(pyorc, c, p):
    sc, kf, cur = p["sc"], p["kf"], p["cur"]
    v, d, claimed = R.reloc_view(kf["keys"], kf["mp_id"], cur["mp_id"], cur["flags"], p["rec"], p["slot_of"])
    return pyorc.search_by_projection_reloc(sc["kf2"], claimed, sc["T2w"], v, d, c["th"], c["dist"], int(c["ori"])) + (v, claimed)


@pytest.mark.parametrize("c", REC_RELOC_CASES, ids=[_id("rreloc", c, ("n", "cur_smaller", "span", "th", "dist", "ori")) for c in REC_RELOC_CASES])
def test_reloc_on_records_random_case(corb, pyorc, synth, c):
    p = rec_reloc_problem(synth, c)
    sc, kf, cur, n = p["sc"], p["kf"], p["cur"], c["n"]
    m_ref, n_ref, _, _ = rec_reloc_reference(pyorc, c, p)
    F_small, F_big = n + 3, n + 131                  # the frame and the keyframe live in stores with different record layouts
    F_cur, F_kf = (F_small, F_big) if c["cur_smaller"] else (F_big, F_small)
    KFc = corb.KeyFrameStore(4, F_cur); KFk = corb.KeyFrameStore(4, F_kf); MP = _put_map(corb, p["rec"], p["lists"])
    _put_frame(KFc, 0, cur, sc["kf2"], sc["T2w"], 22); _put_frame(KFk, 0, kf, sc["kf1"], sc["T1w"], 11)
    m, cnt = KFc.TrackSearchReloc(0, KFk, 0, MP, _camera(corb, sc["kf2"]), sc["T2w"], LOGS, c["th"], c["dist"], c["ori"])
    assert np.array_equal(m, m_ref) and cnt == n_ref and n_ref > 0
    ids, fl = R.matched_writes(cur["mp_id"], cur["flags"], m_ref, kf["mp_id"])
    assert np.array_equal(KFc.get_map_points(0), ids) and np.array_equal(KFc.get(0)["flags"], fl)
    assert np.array_equal(KFk.get_map_points(0), kf["mp_id"])
    KFc.close(); KFk.close(); MP.close()


def rec_scw_problem(synth, c):
    """pKF = KF2's record, vpPoints = KF1's map points by slot in a shuffled order (the call is order dependent), vpMatched = ids per feature of pKF: unrelated ids the
    store does not know and points of vpPoints (spAlreadyFound); bad points"""
    rng = np.random.default_rng(c["seed"]); n = c["n"]
    sc = synth.crowd_keyframe_scene(synth.keyframe_scene(c["seed"], n=n, span=c["span"]), c["seed"])
    rec = _kf_records(1000, sc["pts1"], sc["desc1"], rng, 11)
    cause = rng.choice([GOOD] * 8 + [BAD_POINT, 7], n)
    rec["flags"][cause == BAD_POINT] |= R.MP_BAD
    ci = rng.permutation(n)[: max(3, n // 8)]
    found = np.nonzero(cause == 7)[0][: len(ci) // 2]
    matched = np.full(n, NONE, np.uint64); matched[ci] = np.uint64(UNKNOWN0) + ci.astype(np.uint64); matched[ci[: len(found)]] = rec["id"][found]
    S = sc["T2w"].copy(); S[:3, :] *= np.float32(c["scale"])
    return dict(sc=sc, rec=rec, lists=_obs_lists(rec, 11), matched=matched, order=rng.permutation(n).astype(np.int32), S=S)


def rec_scw_reference(pyorc, c, p):
    v, d, claimed = R.scw_view(p["matched"], p["order"], p["rec"])
    return pyorc.search_by_projection_scw(p["sc"]["kf2"], claimed, p["S"], v, d, c["th"])


@pytest.mark.parametrize("c", REC_SCW_CASES, ids=[_id("rscw", c, ("n", "span", "th", "scale")) for c in REC_SCW_CASES])
def test_scw_on_records_random_case(corb, pyorc, synth, c):
    p = rec_scw_problem(synth, c)
    sc, n = p["sc"], c["n"]
    m_ref, n_ref = rec_scw_reference(pyorc, c, p)
    KF = corb.KeyFrameStore(2, n + (0, 1, 37)[c["i"] % 3]); MP = _put_map(corb, p["rec"], p["lists"], index=False)
    _put_frame(KF, 1, _kf_frame(sc["kf2"], np.full(n, NONE, np.uint64)), sc["kf2"], sc["T2w"], 22)
    ids_after, m, cnt = KF.SearchByProjectionScw(1, MP, p["order"], _camera(corb, sc["kf2"]), p["S"], LOGS, p["matched"], c["th"])
    assert np.array_equal(m, m_ref) and cnt == n_ref and n_ref > 0
    want = p["matched"].copy(); hit = m_ref >= 0; want[hit] = p["rec"]["id"][p["order"][m_ref[hit]]]
    assert np.array_equal(ids_after, want)                                                          # vpMatched[bestIdx] = pMP
    KF.close(); MP.close()


KF1_ID, KF2_ID = 11, 22


def rec_sim3_problem(synth, c):
    """both keyframes in one store; vpMatches12 on entry names points whose observation of KF2 sits first, in the middle and last in lists of max_obs entries, one
    whose index in KF2 is past its features, and one id the store does not know"""
    rng = np.random.default_rng(c["seed"]); n, O = c["n"], c["max_obs"]
    sc = synth.keyframe_scene(c["seed"], n=n, span=c["span"])
    rec = np.concatenate([_kf_records(1000, sc["pts1"], sc["desc1"], rng, KF1_ID), _kf_records(500000, sc["pts2"], sc["desc2"], rng, KF2_ID)])
    lists = [[(KF1_ID, i)] for i in range(n)] + [[(KF2_ID, i)] for i in range(n)]
    k1 = rng.choice([GOOD] * 8 + [NO_POINT, BAD_POINT, UNKNOWN], n); k2 = rng.choice([GOOD] * 8 + [NO_POINT, BAD_POINT, UNKNOWN], n)
    ids1, _ = _hold(k1, np.arange(n), rec, rng); ids2, _ = _hold(k2, n + np.arange(n), rec, rng)
    pre = rng.permutation(n)[: max(6, n // 6)]                                                      # features of KF1 that enter as matched
    pts = n + rng.permutation(n)[: len(pre)]                                                        # ... to these points (slots), seen by KF2 at feature `at`
    at = rng.permutation(n)[: len(pre)]
    matched = np.full(n, NONE, np.uint64); matched[pre] = rec["id"][pts]
    for j, (s_, f) in enumerate(zip(pts, at)):
        where = (0, O // 2, O - 1)[j % 3]                                                           # position of KF2's entry in a full list that ascends in the keyframe id
        lists[s_] = [(KF2_ID - where + k, int(rng.integers(0, n))) for k in range(where)] + [(KF2_ID, int(f))] + [(KF2_ID + 1 + k, int(rng.integers(0, n))) for k in range(O - 1 - where)]
    lists[pts[0]] = [(a, b if a != KF2_ID else n + 7) for a, b in lists[pts[0]]]                    # GetIndexInKeyFrame(pKF2) >= N2
    matched[pre[1]] = np.uint64(UNKNOWN0 + 5)
    return dict(sc=sc, rec=rec, lists=lists, slot_of=R.slot_dict(rec), ids1=ids1, ids2=ids2, matched=matched, pre=pre, at=at)


def rec_sim3_reference(pyorc, c, p, matched):
    sc = p["sc"]
    (v1, d1), (v2, d2) = R.sim3_views(p["ids1"], p["ids2"], matched, p["rec"], p["slot_of"], p["lists"], KF2_ID)
    return pyorc.search_by_sim3(sc["kf1"], sc["kf2"], sc["T1w"], sc["T2w"], v1, d1, v2, d2, sc["s12"], sc["R12"], sc["t12"], 7.5) + (v1, v2)


@pytest.mark.parametrize("c", REC_SIM3_CASES, ids=[_id("rsim3", c, ("n", "span", "max_obs")) for c in REC_SIM3_CASES])
def test_sim3_on_records_random_case(corb, pyorc, synth, c):
    p = rec_sim3_problem(synth, c)
    sc, n = p["sc"], c["n"]
    KF = corb.KeyFrameStore(3, n + (0, 1, 37)[c["i"] % 3]); MP = _put_map(corb, p["rec"], p["lists"], max_obs=c["max_obs"])
    _put_frame(KF, 0, _kf_frame(sc["kf1"], p["ids1"]), sc["kf1"], sc["T1w"], KF1_ID); _put_frame(KF, 2, _kf_frame(sc["kf2"], p["ids2"]), sc["kf2"], sc["T2w"], KF2_ID)
    cam = _camera(corb, sc["kf1"])
    for matched in (None, p["matched"]):
        m_ref, n_ref, v1, v2 = rec_sim3_reference(pyorc, c, p, matched)
        m, ids, cnt = KF.SearchBySim3(0, 2, MP, cam, LOGS, sc["T1w"], sc["T2w"], sc["s12"], sc["R12"], sc["t12"], 7.5, matched12_ids=matched)
        assert np.array_equal(m, m_ref) and cnt == n_ref and n_ref > 0
        hit = m_ref >= 0
        assert np.array_equal(ids[hit], p["ids2"][m_ref[hit]]) and (ids[~hit] == NONE).all()
    assert (m[p["pre"]] == -1).all() and not np.isin(p["at"][2:], m[hit]).any()
    KF.close(); MP.close()


def rec_fuse_problem(synth, c):
    """pKF = KF2's record, vpMapPoints = KF1's map points: bad points, points KF2 observes already (IsInKeyFrame), a later observer (the new entry goes in the middle of
    the list); features of KF2 that hold a MapPoint already (Replace pending)"""
    rng = np.random.default_rng(c["seed"]); n, O = c["n"], c["max_obs"]
    sc = synth.keyframe_scene(c["seed"], n=n, span=c["span"])
    rec = _kf_records(1000, sc["pts1"], sc["desc1"], rng, KF1_ID)
    rec["flags"][rng.random(n) < 0.12] |= R.MP_BAD
    in_kf2 = rng.random(n) < 0.1; later = (rng.random(n) < 0.5) & ~(in_kf2 & (O == 2)) & c["later"]
    lists = [[(KF1_ID, i)] + ([(KF2_ID, 0)] if in_kf2[i] else []) + ([(KF2_ID + 4, 5)] if later[i] else []) for i in range(n)]
    held = np.where(sc["claimed2"] != 0, np.uint64(UNKNOWN0) + np.arange(n, dtype=np.uint64), NONE)
    return dict(sc=sc, rec=rec, lists=lists, held=held)


def rec_fuse_reference(pyorc, c, p):
    sc = p["sc"]
    v, d = R.fuse_view(np.arange(c["n"]), p["rec"], p["lists"], KF2_ID)
    return pyorc.fuse(sc["kf2"], sc["T2w"], NP.camera_centre(sc["T2w"]), 0, v, d, c["th"])


@pytest.mark.parametrize("c", REC_FUSE_CASES, ids=[_id("rfuse", c, ("n", "span", "apply", "max_obs", "later", "th")) for c in REC_FUSE_CASES])
def test_fuse_on_records_random_case(corb, pyorc, synth, c):
    p = rec_fuse_problem(synth, c)
    sc, n, O = p["sc"], c["n"], c["max_obs"]
    bi, bd, nf = rec_fuse_reference(pyorc, c, p)
    mp, act, lists = R.fuse_writes(bi, p["held"], p["rec"]["id"], p["lists"], KF2_ID)
    full = [i for i in range(n) if act[i] == 1 and len(p["lists"][i]) >= O]                         # no room for the new observation
    KF = corb.KeyFrameStore(2, n + (0, 1, 37)[c["i"] % 3]); MP = _put_map(corb, p["rec"], p["lists"], max_obs=O, index=False)
    _put_frame(KF, 1, _kf_frame(sc["kf2"], p["held"]), sc["kf2"], sc["T2w"], KF2_ID)
    a = (1, MP, np.arange(n), _camera(corb, sc["kf2"]), sc["T2w"], LOGS, c["th"])
    assert nf > 0 and (act == 1).sum() > 0
    if c["apply"] and full:                           # "they were not added": the points without room keep their lists and do not enter their features
        with pytest.raises(corb.CorbError, match="no room"):
            KF.Fuse(*a, apply=True)
        for i in full:
            mp[bi[i]] = NONE; lists[i] = p["lists"][i]
    else:
        g = KF.Fuse(*a, apply=c["apply"])
        assert np.array_equal(g[0], bi) and np.array_equal(g[1], bd) and g[2] == nf and np.array_equal(g[3], act)
    if not c["apply"]:
        mp, lists = p["held"], p["lists"]
    assert np.array_equal(KF.get_map_points(1), mp)
    r2, okf, oidx = MP.get(0, n)
    for i in range(n):
        L = len(lists[i])
        assert r2["n_obs"][i] == L and [(int(x), int(y)) for x, y in zip(okf[i, :L], oidx[i, :L])] == lists[i], i
    b = r2.copy(); b["n_obs"] = p["rec"]["n_obs"]; e = p["rec"].copy()
    assert b.tobytes() == e.tobytes()                                                               # nothing else in the headers moved
    KF.close(); MP.close()


# ---------------------------------------------------------------- Replace, distinctive descriptors ----------------------------------------------------------------
def tie_descriptors(rng, shape, p_random=0.06, lead=0):
    """descriptors from an alphabet of three values, one of them frequent, plus a few random ones: equal descriptors have equal rows in the distance matrix, so
    the rows of the frequent value share the least median.  lead: that many first rows are kept off the frequent value, so the first row with the least median
    comes after them"""
    alphabet = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    d = alphabet[rng.choice(3, shape, p=(0.8, 0.12, 0.08))]
    r = rng.random(shape) < p_random
    d[r] = rng.integers(0, 256, (int(r.sum()), 32), dtype=np.uint8)
    if lead:
        d[:lead] = alphabet[rng.integers(1, 3, lead)]; d[lead:] = np.where(r[lead:, None], d[lead:], alphabet[0])
    return d


REPLACE_NKF, REPLACE_F, REPLACE_O = 96, 8, 80


def replace_problem(c):
    """two observation lists whose merged list holds c["merged"] observers that are non-bad keyframes of the store, next to the kinds of the fixed-size test: observers
    outside the store, bad keyframes, keyframes both points share, mnId 0"""
    rng = np.random.default_rng(c["seed"]); L = c["merged"]
    kf_ids = np.concatenate([[0], np.sort(rng.permutation(5000)[: REPLACE_NKF - 1] + 1)]).tolist()
    bad_kf = set(rng.permutation(kf_ids[1:])[:8].tolist())
    good = [k for k in kf_ids if k not in bad_kf]
    outside = [6001, 6002, 6003]
    S = sorted(rng.permutation(good)[:L].tolist())
    if L >= 2 and 0 not in S:
        S[0] = 0
    room = REPLACE_O - L
    extra = (rng.permutation(sorted(bad_kf))[: min(3, room)].tolist() + outside)[:room]
    members = S + extra
    into = [k for k in members if rng.random() < 0.5]; this = [k for k in members if k not in into]
    if not into and L == 1:
        into, this = list(S), [k for k in this if k not in S]
    this += rng.permutation(into)[: min(4, len(into))].tolist()                                    # shared keyframes: erased in the keyframe, not moved
    obs = lambda ks: [(int(k), int(rng.integers(0, REPLACE_F))) for k in sorted(set(ks))]
    descs = dict(zip(kf_ids, tie_descriptors(rng, (REPLACE_NKF, REPLACE_F))))
    return dict(kf_ids=kf_ids, bad_kf=bad_kf, descs=descs, this=obs(this), into=obs(into), third=obs(rng.permutation(good)[:2]), counters=rng.integers(0, 50, (3, 2)),
                own_desc=rng.integers(0, 256, (3, 32), dtype=np.uint8))


def replace_rows(p, into_after):
    """the descriptors pMP->ComputeDistinctiveDescriptors() collects: its observations in non-bad keyframes of the store, in list order"""
    return [p["descs"][k][i] for k, i in into_after if k in p["descs"] and k not in p["bad_kf"]]


@pytest.mark.parametrize("c", REPLACE_CASES, ids=[_id("replace", c, ("merged",)) for c in REPLACE_CASES])
def test_replace_long_lists_random_case(corb, pyorc, c):
    p = replace_problem(c)
    kf_ids, O, F = p["kf_ids"], REPLACE_O, REPLACE_F
    KF = corb.KeyFrameStore(REPLACE_NKF + 2, F); MP = corb.MapPointStore(4, O)
    for s_, kid in enumerate(kf_ids):
        kp = np.zeros(F, corb.KP_DTYPE); kp["x"] = np.arange(F)
        KF.put(s_, kp, p["descs"][kid], None, None, keyframe_id=kid)
        KF.set_meta(s_, id=kid, client_id=1, flags=(corb.KF_BAD if kid in p["bad_kf"] else 0), fx=700.0, fy=700.0, cx=600.0, cy=180.0, bf=380.0, nlevels=8, Tcw=np.eye(4, dtype=np.float32).reshape(16))
    obs = {100: p["this"], 200: p["into"], 300: p["third"]}
    rec = np.zeros(3, corb.MP_RECORD_DTYPE); rec["id"] = [100, 200, 300]; rec["ref_kf_id"] = 3; rec["client_id"] = 1; rec["descriptor"] = p["own_desc"]
    flat = [o for pid in (100, 200, 300) for o in obs[pid]]
    off = np.concatenate([[0], np.cumsum([len(obs[pid]) for pid in (100, 200, 300)])]).astype(np.int32)
    rec["n_obs"] = np.diff(off)
    MP.put(0, rec, off, np.array([a for a, _ in flat], np.uint64), np.array([b for _, b in flat], np.uint32))
    cnt = p["counters"]; MP.set_counters(0, cnt[:, 0].tolist(), cnt[:, 1].tolist())
    held = {}
    for pid in (300, 200, 100):
        for kid, idx in obs[pid]:
            if kid in p["descs"]:
                held[(kid, idx)] = pid
    for s_, kid in enumerate(kf_ids):
        full = np.full(F, NONE, np.uint64)
        for (k_, idx), pid in held.items():
            if k_ == kid:
                full[idx] = pid
        KF.set_map_points(s_, full)
    st, into, act, cinto = pyorc.mappoint_replace(100, 200, obs[100], obs[200], O, tuple(cnt[0]), tuple(cnt[1]))
    rows = replace_rows(p, into)
    assert st == 0 and len(rows) == c["merged"]
    assert MP.Replace(0, 1, KF, 0, REPLACE_NKF + 2) == 0
    for (kid, idx), a in zip(obs[100], act):
        if kid in p["descs"]:
            if a == 1:
                held[(kid, idx)] = 200
            else:
                held.pop((kid, idx), None)
    r, k, i_ = MP.get(0, 3); cn = MP.get_counters(0, 3)
    assert r["n_obs"][0] == 0 and (r["flags"][0] & corb.MP_BAD) and cn["replaced_by"][0] == 201 and not k[0].any()
    assert r["n_obs"][1] == len(into) and [(int(x), int(y)) for x, y in zip(k[1, : len(into)], i_[1, : len(into)])] == into
    assert (cn["n_visible"][1], cn["n_found"][1]) == cinto and cn["replaced_by"][1] == 0 and not (r["flags"][1] & corb.MP_BAD)
    best = pyorc.distinctive_descriptors(np.stack(rows), np.array([0, len(rows)], np.int32))[0]
    assert np.array_equal(r["descriptor"][1], rows[best])
    assert r[2].tobytes() == rec[2].tobytes()                                                       # a bystander
    for s_, kid in enumerate(kf_ids):
        a = KF.get_map_points(s_)
        assert [int(x) for x in a] == [held.get((kid, idx), int(NONE)) for idx in range(F)], kid
    KF.close(); MP.close()


def distinctive_problem():
    rng = np.random.default_rng(DISTINCTIVE_SEED)
    offset = np.concatenate([[0], np.cumsum(DISTINCTIVE_SIZES)]).astype(np.int32)
    lead = {65: 32, 128: 64, 1023: 65, 1024: 300}      # 128: the first 64 rows lose, the other 64 tie -- the first row with the least median opens the second wave
    desc = np.concatenate([tie_descriptors(rng, N, p_random=0.0 if N == 128 else 0.06, lead=lead.get(N, 0)) for N in DISTINCTIVE_SIZES])
    return desc, offset


def test_distinctive_descriptors_with_median_ties(corb, pyorc):
    desc, offset = distinctive_problem()
    g = corb.ComputeDistinctiveDescriptors(desc, offset)
    r = pyorc.distinctive_descriptors(desc, offset)
    assert np.array_equal(g, r), (g, r)

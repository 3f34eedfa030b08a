"""GPU parity: ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) on records (corb_fuse_sim3_store).  The search equals the oracle's Fuse with sim3 = 1 on the same
scene; actions, replace_slot and, with apply, the records equal the action layer of tests/loopfix_reference.py.  The scene is tests/test_gpu_fuse_store.py's, with a pair
of points that compete for one feature, a feature that holds a bad point, a feature that holds a good point of the map (which therefore takes no part) and features
whose ids have no record."""
import numpy as np
import pytest

import loopfix_reference as XR
from test_gpu_fuse_store import _scene_on_records, KF2_ID

pytestmark = pytest.mark.gpu
NONE = np.uint64(XR.NO_ID)


def test_fuse_with_scw_on_records(corb, pyorc, synth):
    n = 150
    sc, KF, MP, rec, (off, okf, oidx), held, view, cam, T, Ow = _scene_on_records(corb, synth, 5300, n, 1.0)
    k2 = sc["kf2"]; nf = len(k2["keys_un"])
    s = np.float32(0.8)
    Scw = T.copy(); Scw[:3] *= s                                 # Converter::toCvMat(g2oScw): [sR | st]
    lists = [list(zip(okf[off[i]: off[i + 1]], oidx[off[i]: off[i + 1]])) for i in range(n)]
    bad = rec["flags"] != 0
    # a first look at who goes where, to place the special cases on features that are used
    probe = view.copy(); probe["valid"] = (~bad).astype(np.uint8)
    b0 = pyorc.fuse(k2, Scw, None, 1, probe, sc["desc1"], 4.0)[0]
    fused = [i for i in range(n) if b0[i] >= 0]
    assert len(fused) > 40
    a = fused[0]; c = next(i for i in fused if b0[i] != b0[a]); e = next(i for i in fused if b0[i] not in (b0[a], b0[c]))      # three different features
    twin = next(i for i in range(n) if b0[i] < 0 and not bad[i])                      # becomes a copy of point e: both are fused into e's feature
    rec["world_pos"][twin] = rec["world_pos"][e]; rec["normal"][twin] = rec["normal"][e]; rec["min_distance"][twin] = rec["min_distance"][e]
    rec["max_distance"][twin] = rec["max_distance"][e]; rec["descriptor"][twin] = rec["descriptor"][e]
    dead = next(i for i in range(n) if bad[i]); good = next(i for i in range(n) if b0[i] < 0 and not bad[i] and i != twin)
    held = held.copy()
    held[b0[a]] = rec["id"][dead]                                # a's feature holds a bad point
    held[b0[c]] = rec["id"][good]                                # c's feature holds a good point of the list: that point is in the record and takes no part
    held[b0[e]] = NONE                                           # e and its twin compete for an empty feature
    MP.put(0, rec, np.array(off, np.int32), np.array(okf, np.uint64), np.array(oidx, np.uint32)); MP.build_index(0, n)
    KF.set_map_points(1, held)
    desc = rec["descriptor"]
    v = np.zeros(n, view.dtype)
    for k in ("world", "normal", "min_distance", "max_distance"):
        v[k] = rec[{"world": "world_pos"}.get(k, k)]
    v["valid"] = XR.fuse_sim3_takes_part(rec["id"], bad, held).astype(np.uint8)
    assert v["valid"][good] == 0
    r = pyorc.fuse(k2, Scw, None, 1, v, desc, 4.0)
    slot_of = {int(i): k for k, i in enumerate(rec["id"])}
    want_held, act, rep, want_lists = XR.fuse_sim3_actions(r[0], held, [int(i) for i in rec["id"]], slot_of, {int(i) for i in rec["id"][bad]}, lists, KF2_ID)
    assert act[a] == 4 and (act[c], rep[c]) == (2, good) and sorted([(act[e], rep[e]), (act[twin], rep[twin])]) == [(1, -1), (2, min(e, twin))]
    assert (act == 1).sum() > 10 and ((act == 2) & (rep < 0)).sum() > 0
    assert any(act[i] == 1 and KF2_ID in [k for k, _ in lists[i]] for i in range(n))              # a point the keyframe observes but does not hold enters a feature
    before = MP.get(0, n)[0].tobytes()
    g = KF.FuseSim3(1, MP, np.arange(n), cam, Scw, k2["log_scale_factor"], 4.0, apply=False)
    assert np.array_equal(g[0], r[0]) and np.array_equal(g[1], r[1]) and g[2] == r[2] == (r[0] >= 0).sum()
    assert np.array_equal(g[3], act) and np.array_equal(g[4], rep)
    assert MP.get(0, n)[0].tobytes() == before and np.array_equal(KF.get_map_points(1), held)          # apply = False: the records are as they were
    g = KF.FuseSim3(1, MP, np.arange(n), cam, Scw, k2["log_scale_factor"], 4.0, apply=True)
    assert np.array_equal(g[0], r[0]) and np.array_equal(g[3], act) and np.array_equal(g[4], rep)
    assert np.array_equal(KF.get_map_points(1), want_held)
    r2, k2o, i2o = MP.get(0, n)
    for i in range(n):
        assert r2["n_obs"][i] == len(want_lists[i]) and [int(x) for x in k2o[i, : len(want_lists[i])]] == [x for x, _ in want_lists[i]] \
            and [int(x) for x in i2o[i, : len(want_lists[i])]] == [y for _, y in want_lists[i]], i
    b = r2.copy(); b["n_obs"] = rec["n_obs"]
    assert b.tobytes() == rec.tobytes()                                                              # nothing else in the headers moved
    KF.close(); MP.close()

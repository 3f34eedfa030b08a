"""A handle that grew gives the bits of a fresh one.  The handles keep their buffers between calls and replace them when a call needs more (csrc/owned.h: the old
allocation goes, a larger one comes, the contents are lost); every call writes what it reads.  Each test serves a small call, a call large enough to replace
buffers, and the small call again, and holds the third call to the bits of a fresh handle that served only it."""
import threading

import numpy as np
import pytest

import kfinsert_cases as KG
import kfinsert_stores as KS
import publish_cases as G
import publish_stores as S

pytestmark = pytest.mark.gpu
F, O = 64, 4


def _publish(corb, srv, cli, reader, c):
    """pack on the server's stores, apply on the client's: (message bytes, outputs, the client's records afterwards)"""
    cl = c["client"]
    SKF, SMP = S.to_stores(corb, c["server"]["kfs"], c["server"]["mps"], c["F"], c["O"]); CKF, CMP = S.client_stores(corb, cl, c["F"], c["O"])
    try:
        srv.pack(SKF, mp=SMP, **c["pack"])
        m = srv.message(); raw = srv.message_bytes().tobytes()
        out = cli.apply(m, cl["client_id"], CKF, cl["kf_first"], cl["kf_n"], cl["kf_free_first"], cl["kf_room"], CMP, cl["mp_first"], cl["mp_n"], cl["mp_free_first"], cl["mp_room"], apply=True)
        return raw, out, S.raw_of(corb, reader, CKF, len(cl["kfs"]), CMP, len(cl["mps"]))
    finally:
        for s in (SKF, SMP, CKF, CMP):
            s.close()


def test_map_publisher(corb):
    """1 keyframe record, then 8, then 1 again: one record of F = 64 exceeds the 4096-byte floor of the handle's buffers, so the second message does not fit"""
    assert S.kf_layout(F)["bytes"] > 4096
    one = G.make_case(seed=101, nA=1, F=F, O=O); eight = G.make_case(seed=102, nA=8, F=F, O=O)
    srv, cli, reader = corb.MapPublisher(), corb.MapPublisher(), corb.MapPublisher()
    fresh_srv, fresh_cli = corb.MapPublisher(), corb.MapPublisher()
    try:
        first = _publish(corb, srv, cli, reader, one)
        large = _publish(corb, srv, cli, reader, eight)
        third = _publish(corb, srv, cli, reader, one)
        want = _publish(corb, fresh_srv, fresh_cli, reader, one)
        assert len(large[0]) > 8 * 4096 > len(first[0]) + len(first[0]) // 4            # (the first buffer: a quarter more than the first message)
        assert first[1]["n_kf_inserted"] + large[1]["n_kf_inserted"] > 0                # the calls did something
        for got in (first, third):
            assert got[0] == want[0] and S.same_outputs(got[1], want[1]) is None and S.same_outputs(want[1], got[1]) is None and got[2] == want[2]
        p = one["pack"]                                                                  # ... and the fresh handle gives the definition's message
        msg = G.R.pack(one["server"]["kfs"], p["new_kf_slots"], p["upd_kf_slots"], one["server"]["mps"], p["new_mp_slots"], p["upd_mp_slots"], p["trans"])
        assert want[0] == S.message_raw(corb, msg, F, O)[0]
    finally:
        for h in (srv, cli, reader, fresh_srv, fresh_cli):
            h.close()


def test_keyframe_inserter(corb):
    """process_new_keyframe with 1 keyframe slot at hand, then 200 (the handle's id table of the keyframes grows from 64 to 512 entries), then 1 again"""
    sc, a = KG.assoc_case("n65")
    rng = np.random.default_rng(7)
    sc = dict(sc, kfs=sc["kfs"] + [KG.keyframe(rng, 100000 + i, 0) for i in range(200)])                # slots 6 .. 205: no features, no keyframes
    small = dict(slot=a["slot"], kf_first=a["slot"], kf_n=1, scale_factor=a["scale_factor"]); large = dict(small, kf_first=1, kf_n=200)
    grown, fresh = corb.KeyframeInserter(KG.F, 8), corb.KeyframeInserter(KG.F, 8)
    stores = [KS.to_stores(corb, sc) for _ in range(2)]
    try:
        (KF, MP), (KF2, MP2) = stores
        dry = lambda h, kf, mp, w: h.ProcessNewKeyFrame(kf, w["slot"], mp, w["kf_first"], w["kf_n"], w["scale_factor"], apply=False)
        first = dry(grown, KF, MP, small)
        dry(grown, KF, MP, large)
        third = grown.ProcessNewKeyFrame(KF, small["slot"], MP, small["kf_first"], small["kf_n"], small["scale_factor"], apply=True)
        want = fresh.ProcessNewKeyFrame(KF2, small["slot"], MP2, small["kf_first"], small["kf_n"], small["scale_factor"], apply=True)
        for got in (first, third):
            assert sorted(got) == sorted(want)
            for k, v in want.items():
                assert np.array_equal(np.asarray(got[k]), np.asarray(v)), k
        assert KS.state(KF, MP) == KS.state(KF2, MP2)
    finally:
        grown.close(); fresh.close()
        for kf, mp in stores:
            kf.close(); mp.close()


def _push(comms, src, slots, dst):
    """rank 1 sends the records `slots` of src to rank 0, which files them from slot 0 of dst on"""
    out = [None, None]

    def run(r):
        try:
            out[r] = comms[r].map_push(dst if r == 0 else src, [] if r == 0 else slots, root=0, dst_first=[0, 0])
        except Exception as e:                                       # noqa: BLE001
            out[r] = e
    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(60)
    assert not any(t.is_alive() for t in th), "a rank is stuck in the collective"
    assert not any(isinstance(o, Exception) for o in out), out
    assert list(out[0]) == [0, len(slots)]


def test_in_process_comm(corb):
    """a map push of 1 record, then of enough F = 64 records to pass the 1 MB floor of the staging buffer, then of 1 record"""
    rec_bytes = S.kf_layout(F)["bytes"]; n = (1 << 20) // rec_bytes + 8
    rng = np.random.default_rng(11)
    kfs = [G.kf_record(rng, 1000 + i, 2, 0, F) for i in range(n)]
    SRC, SMP = S.to_stores(corb, kfs, [], F, O); DST, DMP = S.to_stores(corb, [], [], F, O, extra_kf=n); DST2, DMP2 = S.to_stores(corb, [], [], F, O, extra_kf=n)
    grown, fresh = corb.Comm.local(2), corb.Comm.local(2)
    reader = corb.MapPublisher()
    try:
        assert n * rec_bytes > 1 << 20 and SRC.record_bytes() == rec_bytes
        _push(grown, SRC, [3], DST)
        _push(grown, SRC, list(range(n - 1, -1, -1)), DST)                                               # (descending: no contiguous run)
        assert [DST.get(s)["id"] for s in (0, 1, n - 1)] == [kfs[s]["id"] for s in (n - 1, n - 2, 0)]
        _push(grown, SRC, [7], DST)
        _push(fresh, SRC, [7], DST2)
        assert DST.get(0)["id"] == DST2.get(0)["id"] == kfs[7]["id"]                                     # (the read also brings the host's feature count up to date)
        got = S.raw_of(corb, reader, DST, 1, DMP, 0); want = S.raw_of(corb, reader, DST2, 1, DMP2, 0)
        assert got == want == S.kf_raw(corb, kfs[7], F)
    finally:
        for c in grown + fresh:
            c.close()
        reader.close()
        for s in (SRC, SMP, DST, DMP, DST2, DMP2):
            s.close()


def test_map_point_store_local_ba(corb, synth):
    """LocalBundleAdjustmentStore on a window of 3 keyframes, then of 12, then of the 3 again on the restored records: the scratch the call keeps in the map-point
    store (sized by what earlier calls asked for) does not reach the estimates"""
    K = 12
    prob = synth.local_ba_problem(seed=2300, n_local=6, n_fixed=6, pts_per_kf=25, outlier_frac=0.1, max_obs=5)
    cm = synth.client_maps(prob, 1, K)[0]
    M = len(cm["mp_records"])
    KF = corb.KeyFrameStore(K, max(len(k["kp"]) for k in cm["kf"]) + 3); MP = corb.MapPointStore(M, 16)

    def restore():
        for s, k in enumerate(cm["kf"]):
            KF.put(s, k["kp"], k["desc"], k["ur"], None, keyframe_id=k["id"])
            cam = k["cam"]
            KF.set_meta(s, id=k["id"], client_id=1, flags=0, fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3], bf=cam[4], nlevels=8, Tcw=k["Tcw"].reshape(16),
                        inv_level_sigma2=np.concatenate([k["inv_level_sigma2"], np.zeros(8, np.float32)]))
            KF.set_map_points(s, k["mp_id"])
        MP.put(0, cm["mp_records"], cm["obs_off"], cm["obs_kf"], cm["obs_idx"])

    def records():
        return tuple(x.tobytes() for x in MP.get(0, M)) + tuple(KF.get_meta(s).tobytes() for s in range(K))

    window = [0, 1, 2]; ids = [cm["kf"][s]["id"] for s in window]
    seen = np.add.reduceat(np.isin(cm["obs_kf"], ids).astype(np.int64), cm["obs_off"][:-1])              # (every point has an observation: no empty segment)
    points = np.flatnonzero(seen >= 2)
    assert np.all(np.diff(cm["obs_off"]) > 0) and len(points) >= 20
    try:
        restore(); pristine = records()
        first = corb.LocalBundleAdjustmentStore(KF, window, 2, MP, points); after_first = records()
        restore(); assert records() == pristine
        large = corb.LocalBundleAdjustmentStore(KF, np.arange(K), 6, MP, np.arange(M))
        restore(); assert records() == pristine
        third = corb.LocalBundleAdjustmentStore(KF, window, 2, MP, points)
        assert first["iters_done"] > 0 and large["iters_done"] > 0 and after_first != pristine
        assert third["poses"].tobytes() == first["poses"].tobytes() and third["points"].tobytes() == first["points"].tobytes()
        assert third["erase"].tobytes() == first["erase"].tobytes() and records() == after_first
    finally:
        KF.close(); MP.close()

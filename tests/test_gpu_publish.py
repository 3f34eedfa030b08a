"""The map publish on records (include/corb_map_publish.h) against its definition (tests/publish_reference.py) on the seeded cases of tests/publish_cases.py: pack on a
server's stores, apply on a client's.  Checked per case: the message's bytes; every kind array, count and destination slot; EVERY BYTE of every record of both client
stores, untouched and stale records included (tests/publish_stores.py restates the record layouts); apply == 0 and CORB_ERR_CAPACITY leave the bytes alone and return
complete outputs -- each on a fresh pair of handles and on a pair that has just served the largest case."""
import numpy as np
import pytest

import publish_cases as G
import publish_reference as R
import publish_stores as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reader(corb):
    h = corb.MapPublisher()
    yield h
    h.close()


class Dirty:
    """a server and a client handle that have just served the largest case"""

    def __init__(self, corb):
        self.corb = corb; self.srv = corb.MapPublisher(); self.cli = corb.MapPublisher()
        c = G.case("n513")
        self.stores = S.to_stores(corb, c["server"]["kfs"], c["server"]["mps"], c["F"], c["O"]) + S.client_stores(corb, c["client"], c["F"], c["O"])

    def serve(self):
        c = G.case("n513"); SKF, SMP, CKF, CMP = self.stores
        self.srv.pack(SKF, mp=SMP, **c["pack"])
        _apply(self.cli, self.srv.message(), c["client"], CKF, CMP, apply=False)
        return self.srv, self.cli


@pytest.fixture(scope="module")
def dirty(corb):
    d = Dirty(corb)
    yield d
    d.srv.close(); d.cli.close()
    for s in d.stores:
        s.close()


def _apply(h, m, cl, KF, MP, apply=True, **over):
    a = dict(cl, **over)
    return h.apply(m, a["client_id"], KF, a["kf_first"], a["kf_n"], a["kf_free_first"], a["kf_room"], MP, a["mp_first"], a["mp_n"], a["mp_free_first"], a["mp_room"], apply=apply)


def _raw(corb, reader, KF, MP, cl):
    return S.raw_of(corb, reader, KF, len(cl["kfs"]), MP, len(cl["mps"]))


def _expected(corb, cl, c):
    return S.raw_expected(corb, cl["kfs"], cl["mps"], c["F"], c["O"])


@pytest.mark.parametrize("which", ["fresh", "dirty"])
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_pack_and_apply_equal_the_definition(corb, reader, dirty, name, which):
    c = G.case(name); msg = G.message(name); cl = c["client"]
    srv, cli = (corb.MapPublisher(), corb.MapPublisher()) if which == "fresh" else dirty.serve()
    SKF, SMP = S.to_stores(corb, c["server"]["kfs"], c["server"]["mps"], c["F"], c["O"])
    CKF, CMP = S.client_stores(corb, cl, c["F"], c["O"])
    try:
        srv.pack(SKF, mp=SMP, **c["pack"])
        m = srv.message()
        want_bytes, counts = S.message_raw(corb, msg, c["F"], c["O"])
        assert m["counts"].tolist() == counts and m["bytes"] == len(want_bytes)
        assert srv.message_bytes().tobytes() == want_bytes
        before = _raw(corb, reader, CKF, CMP, cl)
        assert before == _expected(corb, cl, c)                     # the stores hold what the definition starts from, byte for byte
        want, after = R.apply(msg, cl)
        got = _apply(cli, m, cl, CKF, CMP, apply=False)
        assert S.same_outputs(got, want) is None, (which, S.same_outputs(got, want))
        assert _raw(corb, reader, CKF, CMP, cl) == before
        got = _apply(cli, m, cl, CKF, CMP, apply=True)
        assert S.same_outputs(got, want) is None, (which, S.same_outputs(got, want))
        now = _raw(corb, reader, CKF, CMP, cl)
        if want["capacity_error"]:
            assert now == before
        else:
            exp = _expected(corb, dict(after, kfs=after["kfs"][: len(cl["kfs"])], mps=after["mps"][: len(cl["mps"])]), c)
            assert len(now) == len(exp)
            if now != exp:
                d = np.flatnonzero(np.frombuffer(now, np.uint8) != np.frombuffer(exp, np.uint8))
                raise AssertionError("%s / %s: %d bytes differ, the first at %d" % (name, which, len(d), d[0]))
            # the host's mirror of the new keyframe slots is current: the feature counts are the records'
            for s, k in zip(want["kf_new_slots"], [a for a, kd in zip(msg["A"], want["kind_kf_new"]) if kd == 3]):
                assert len(CKF.get(int(s))["kp"]) == len(k["kp"])
    finally:
        if which == "fresh":
            srv.close(); cli.close()
        for s in (SKF, SMP, CKF, CMP):
            s.close()


def test_an_all_empty_message_applies_nothing(corb):
    c = G.case("n1"); cl = c["client"]
    srv = corb.MapPublisher(); cli = corb.MapPublisher()
    CKF, CMP = S.client_stores(corb, cl, c["F"], c["O"])
    srv.pack(None)
    m = srv.message()
    assert m["bytes"] == 0 and m["counts"].tolist() == [0] * 5 and m["ptr"] is None
    got = _apply(cli, m, cl, CKF, CMP)
    assert all(int(np.sum(v)) == 0 for v in got.values())
    srv.close(); cli.close(); CKF.close(); CMP.close()


def test_a_second_identical_apply_inserts_nothing_and_the_index_is_current(corb, reader):
    c = G.case("f64"); msg = G.message("f64"); cl = c["client"]
    srv = corb.MapPublisher(); cli = corb.MapPublisher(); ins = corb.KeyframeInserter(c["F"], 8)
    SKF, SMP = S.to_stores(corb, c["server"]["kfs"], c["server"]["mps"], c["F"], c["O"])
    CKF, CMP = S.client_stores(corb, cl, c["F"], c["O"])
    srv.pack(SKF, mp=SMP, **c["pack"]); m = srv.message()
    want, after = R.apply(msg, cl)
    # before: a frame whose features name the points phase B is about to insert resolves none of them
    new_ids = [msg["B"][i]["id"] for i in np.flatnonzero(want["kind_mp_new"] == 3)]
    frame = max(range(cl["kf_n"]), key=lambda s: len(cl["kfs"][s]["kp"])); n = len(cl["kfs"][frame]["kp"]); assert len(new_ids) >= 4 and n >= 4
    ids = np.full(n, corb.NO_MAP_POINT, np.uint64); ids[: min(n, len(new_ids))] = new_ids[: min(n, len(new_ids))]
    CKF.set_map_points(frame, ids)
    close = int((np.asarray(cl["kfs"][frame]["depth"])[: min(n, len(new_ids))] > 0).sum()); assert close >= 1
    all_close = int((np.asarray(cl["kfs"][frame]["depth"]) > 0).sum())
    assert ins.NeedKeyFrameCounts(CKF, frame, CMP, 1e9, CKF, -1, 0, 0, cl["kf_n"])[:2] == (0, all_close)
    got = _apply(cli, m, cl, CKF, CMP)
    assert S.same_outputs(got, want) is None
    # after: the same call resolves them through the index the apply left current -- no corb_mp_store_build_index in between
    assert ins.NeedKeyFrameCounts(CKF, frame, CMP, 1e9, CKF, -1, 0, 0, cl["kf_n"])[:2] == (close, all_close - close)
    CKF.set_map_points(frame, cl["kfs"][frame]["mp_id"])
    # the second apply: the slots the first one filled are held now
    again = dict(after, kf_n=cl["kf_n"] + want["n_kf_inserted"], kf_free_first=cl["kf_free_first"] + want["n_kf_inserted"], kf_room=1,
                 mp_free_first=after["mp_n"], mp_room=1)
    want2, after2 = R.apply(msg, again)
    assert not (set(want2["kind_kf_new"].tolist()) | set(want2["kind_mp_new"].tolist())) & {3} and want2["n_kf_updated"] >= want["n_kf_updated"]
    first = _raw(corb, reader, CKF, CMP, cl)
    got2 = _apply(cli, m, again, CKF, CMP)
    assert S.same_outputs(got2, want2) is None
    assert _raw(corb, reader, CKF, CMP, cl) == first == _expected(corb, dict(after2, kfs=after2["kfs"][: len(cl["kfs"])], mps=after2["mps"][: len(cl["mps"])]), c)
    for h in (srv, cli, ins, SKF, SMP, CKF, CMP):
        h.close()


def test_arguments(corb):
    c = G.case("n1"); cl = c["client"]; p = c["pack"]
    srv = corb.MapPublisher(); cli = corb.MapPublisher()
    SKF, SMP = S.to_stores(corb, c["server"]["kfs"], c["server"]["mps"], c["F"], c["O"], extra_kf=1)
    CKF, CMP = S.client_stores(corb, cl, c["F"], c["O"])
    srv.pack(SKF, mp=SMP, **p); m = srv.message(); kept = srv.message_bytes().tobytes()
    for bad in (dict(p, new_kf_slots=[len(c["server"]["kfs"])]),                   # an empty slot
                dict(p, upd_kf_slots=[len(c["server"]["kfs"]) + 1]),               # out of range
                dict(p, new_mp_slots=[-1]),
                dict(p, trans=list(p["trans"]) + [p["trans"][0]]),                 # a client named twice
                dict(p, trans=[(7, np.zeros((4, 4), np.float32))])):              # no inverse
        with pytest.raises(corb.CorbError):
            srv.pack(SKF, mp=SMP, **bad)
        assert srv.message_bytes().tobytes() == kept                               # nothing was packed
    with pytest.raises(corb.CorbError):
        _apply(cli, dict(m, kf_record_bytes=m["kf_record_bytes"] + 64), cl, CKF, CMP)      # the records differ in size
    with pytest.raises(corb.CorbError):
        _apply(cli, m, cl, CKF, CMP, kf_free_first=cl["kf_n"] - 1, kf_room=2)      # the free slots overlap the resolved ones
    with pytest.raises(corb.CorbError):
        _apply(cli, m, cl, CKF, CMP, mp_n=cl["mp_n"] - 1)                          # not the range the index covers
    with pytest.raises(corb.CorbError):
        _apply(cli, m, cl, CKF, CMP, kf_room=len(cl["kfs"]))                       # beyond the store
    rec, okf, oi = CMP.get(0, 1); CMP.put(0, rec, np.array([0, int(rec["n_obs"][0])], np.int32), okf[0, : int(rec["n_obs"][0])], oi[0, : int(rec["n_obs"][0])])
    with pytest.raises(corb.CorbError):
        _apply(cli, m, cl, CKF, CMP)                                               # a put since the index was built
    for h in (srv, cli, SKF, SMP, CKF, CMP):
        h.close()


def _window_stores(corb, cm):
    """the window of tests/test_gpu_local_ba_store.py filed in a pair of stores"""
    F = max(len(k["kp"]) for k in cm["kf"]) + 3
    KF = corb.KeyFrameStore(len(cm["kf"]), F); MP = corb.MapPointStore(len(cm["mp_records"]), 16)
    for s, k in enumerate(cm["kf"]):
        KF.put(s, k["kp"], k["desc"], k["ur"], None, keyframe_id=k["id"])
        cam = k["cam"]
        KF.set_meta(s, id=k["id"], client_id=1, flags=0, fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3], bf=cam[4], nlevels=8, Tcw=k["Tcw"].reshape(16),
                    inv_level_sigma2=np.concatenate([k["inv_level_sigma2"], np.zeros(8, np.float32)]))
        KF.set_map_points(s, k["mp_id"])
    MP.put(0, cm["mp_records"], cm["obs_off"], cm["obs_kf"], cm["obs_idx"])
    return KF, MP


def test_local_ba_keeps_an_inserted_keyframe_fixed(corb, synth):
    """a local keyframe of a bundle-adjustment window arrives from the server: corb_local_ba_store optimises the window around it and leaves its pose alone"""
    n_local, s0 = 6, 5
    prob = synth.local_ba_problem(seed=2100, n_local=n_local, n_fixed=4, pts_per_kf=25, outlier_frac=0.12, max_obs=5)
    cm = synth.client_maps(prob, 1, n_local + 4)[0]; K, M = len(cm["kf"]), len(cm["mp_records"])
    SKF, SMP = _window_stores(corb, cm); CKF, CMP = _window_stores(corb, cm)
    T = G.pose(np.random.default_rng(4)); k0 = cm["kf"][s0]
    SKF.set_meta(s0, Tcw=R.mul44(k0["Tcw"].reshape(4, 4), T).reshape(16))                     # the server holds it in the global frame
    CKF.put(s0, k0["kp"][:1], k0["desc"][:1], k0["ur"][:1], None, keyframe_id=987654321)       # the client does not hold it yet: a stale record in the free slot
    srv = corb.MapPublisher(); cli = corb.MapPublisher()
    srv.pack(SKF, new_kf_slots=[s0], trans={2: T})
    got = cli.apply(srv.message(), 2, CKF, 0, s0, s0, 1)
    assert got["kind_kf_new"].tolist() == [3] and got["kf_new_slots"].tolist() == [s0] and not got["capacity_error"]
    m = CKF.get_meta(s0)
    want = R.mul44(R.mul44(k0["Tcw"].reshape(4, 4), T), R.inverse4(T))
    assert int(m["id"]) == int(k0["id"]) and int(m["flags"]) & corb.KF_FIXED and np.array_equal(m["Tcw"].view(np.uint32), want.reshape(16).view(np.uint32))
    assert np.array_equal(CKF.get_map_points(s0), np.asarray(k0["mp_id"], np.uint64))           # the features came with the record, and the host knows their number
    before = [CKF.get_meta(s)["Tcw"].copy() for s in range(K)]
    g = corb.LocalBundleAdjustmentStore(CKF, np.arange(K), n_local, CMP, np.arange(M), scale_factor=1.2)
    after = [CKF.get_meta(s)["Tcw"].copy() for s in range(K)]
    assert np.array_equal(after[s0].view(np.uint32), before[s0].view(np.uint32)) and np.array_equal(g["poses"][s0].reshape(16).view(np.uint32), before[s0].view(np.uint32))
    assert sum(not np.array_equal(after[s], before[s]) for s in range(n_local)) >= 3              # the free local keyframes moved
    for h in (srv, cli, SKF, SMP, CKF, CMP):
        h.close()

"""corb_map_publish over the in-process transport: Comm.local(4), one host thread per rank on one GPU, root 0 and three clients whose frames differ.  Every client's
stores end equal to the definition (tests/publish_reference.py), byte for byte; a rank with a wrong record size makes all four ranks return the same error with every
store untouched; an all-empty publish returns zeros; a world of one over RCCL (if librccl.so loads) publishes to nobody.  The multi-GPU RCCL leg needs more than one
card: its posting order is covered by the recording fake of tests/test_publish_plan.py only."""
import copy
import threading

import numpy as np
import pytest

import publish_cases as G
import publish_reference as R
import publish_stores as S

pytestmark = pytest.mark.gpu
W, ROOT = 4, 0


def _run(fns):
    """one thread per rank; returns the results, exceptions included"""
    out = [None] * len(fns)

    def go(r):
        try:
            out[r] = fns[r]()
        except Exception as e:                                     # (returned, compared by the caller)
            out[r] = e
    th = [threading.Thread(target=go, args=(r,), daemon=True) for r in range(len(fns))]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not any(t.is_alive() for t in th), "a rank did not return"
    return out


def _clients(c):
    """three clients with the case's stores: ids 2 (the case's own), 3 and 4 -- for 3 and 4 nothing of the message is their own, and 4 is not in the table"""
    cls = []; rng = np.random.default_rng(99)
    for cid in (G.CLIENT, 3, 4):
        cl = copy.deepcopy(c["client"]); cl["client_id"] = cid
        if cid != G.CLIENT:                                        # (what is client 2's own is foreign to them: room for every entry, in stale records of other ids)
            cl["kfs"] += [G.kf_record(rng, 10 ** 15 + k, G.OTHER, 0, c["F"]) for k in range(len(c["pack"]["new_kf_slots"]))]
            cl["mps"] += [G.mp_record(rng, 10 ** 15 + k, G.OTHER, 0, c["O"]) for k in range(len(c["pack"]["new_mp_slots"]))]
        cl["kf_room"] = len(cl["kfs"]) - cl["kf_free_first"]; cl["mp_room"] = len(cl["mps"]) - cl["mp_free_first"]
        cls.append(cl)
    return cls


def _args(cl, KF, MP):
    return dict(client_id=cl["client_id"], kf=KF, kf_first=cl["kf_first"], kf_n=cl["kf_n"], kf_free_first=cl["kf_free_first"], kf_room=cl["kf_room"],
                mp=MP, mp_first=cl["mp_first"], mp_n=cl["mp_n"], mp_free_first=cl["mp_free_first"], mp_room=cl["mp_room"])


def test_four_ranks_publish(corb):
    c = G.case("f64"); msg = G.message("f64"); counts = [len(msg[k]) for k in "ABCD"]
    comms = corb.Comm.local(W); pubs = [corb.MapPublisher() for _ in range(W)]; reader = corb.MapPublisher()
    SKF, SMP = S.to_stores(corb, c["server"]["kfs"], c["server"]["mps"], c["F"], c["O"])
    cls = _clients(c); stores = [S.client_stores(corb, cl, c["F"], c["O"]) for cl in cls]
    before = [S.raw_of(corb, reader, KF, len(cl["kfs"]), MP, len(cl["mps"])) for cl, (KF, MP) in zip(cls, stores)]
    pack = dict(c["pack"], kf=SKF, mp=SMP)
    raw = lambda k: S.raw_of(corb, reader, stores[k][0], len(cls[k]["kfs"]), stores[k][1], len(cls[k]["mps"]))

    # 1. an all-empty publish: nothing is exchanged, zeros come back
    res = _run([lambda: comms[0].map_publish(pubs[0], ROOT, pack=dict(kf=SKF, mp=SMP))] +
               [lambda k=k: comms[k + 1].map_publish(pubs[k + 1], ROOT, apply=_args(cls[k], *stores[k]), max_counts=counts) for k in range(3)])
    assert res[0] is None
    for k in range(3):
        assert not isinstance(res[k + 1], Exception), res[k + 1]
        assert all(int(np.sum(v)) == 0 for v in res[k + 1].values()) and raw(k) == before[k]

    # 2. a rank whose map-point records differ in size: the same error on all four ranks, every store untouched
    ODD = corb.MapPointStore(len(cls[1]["mps"]), c["O"] + 16)      # (records of another size: the layout rounds to 64 bytes)
    assert ODD.record_bytes() != stores[1][1].record_bytes()
    res = _run([lambda: comms[0].map_publish(pubs[0], ROOT, pack=pack)] +
               [lambda k=k: comms[k + 1].map_publish(pubs[k + 1], ROOT, apply=dict(_args(cls[k], *stores[k]), mp=ODD if k == 1 else stores[k][1]), max_counts=counts) for k in range(3)])
    assert all(isinstance(r, corb.CorbError) and "(-1)" in str(r) for r in res), res
    assert all(raw(k) == before[k] for k in range(3))
    # ... and a client that names the root's source store as its destination
    res = _run([lambda: comms[0].map_publish(pubs[0], ROOT, pack=pack)] +
               [lambda k=k: comms[k + 1].map_publish(pubs[k + 1], ROOT, apply=dict(_args(cls[k], *stores[k]), kf=SKF if k == 2 else stores[k][0]), max_counts=counts) for k in range(3)])
    assert all(isinstance(r, corb.CorbError) and "(-1)" in str(r) for r in res), res
    assert all(raw(k) == before[k] for k in range(3))

    # 3. the publish: every client's stores end as the definition says
    res = _run([lambda: comms[0].map_publish(pubs[0], ROOT, pack=pack)] +
               [lambda k=k: comms[k + 1].map_publish(pubs[k + 1], ROOT, apply=_args(cls[k], *stores[k]), max_counts=counts) for k in range(3)])
    assert res[0] is None
    for k, cl in enumerate(cls):
        assert not isinstance(res[k + 1], Exception), res[k + 1]
        want, after = R.apply(msg, cl)
        assert not want["capacity_error"] and S.same_outputs(res[k + 1], want) is None, (k, S.same_outputs(res[k + 1], want))
        assert raw(k) == S.raw_expected(corb, after["kfs"][: len(cl["kfs"])], after["mps"][: len(cl["mps"])], c["F"], c["O"]), k
    assert raw(2) == before[2] and raw(0) != before[0] and raw(1) != before[1]            # client 4 is not in the table

    # 4. one client's CORB_ERR_CAPACITY does not undo another's apply
    cls2 = _clients(c); stores2 = [S.client_stores(corb, cl, c["F"], c["O"]) for cl in cls2]
    cls2[1]["kf_room"] = 0
    res = _run([lambda: comms[0].map_publish(pubs[0], ROOT, pack=pack)] +
               [lambda k=k: comms[k + 1].map_publish(pubs[k + 1], ROOT, apply=_args(cls2[k], *stores2[k]), max_counts=counts) for k in range(3)])
    assert res[0] is None and not res[1]["capacity_error"] and res[2]["capacity_error"] and res[1]["n_kf_inserted"] > 0
    assert S.raw_of(corb, reader, stores2[1][0], len(cls2[1]["kfs"]), stores2[1][1], len(cls2[1]["mps"])) == before[1]
    assert S.raw_of(corb, reader, stores2[0][0], len(cls2[0]["kfs"]), stores2[0][1], len(cls2[0]["mps"])) == raw(0)
    for h in comms + pubs + [reader, SKF, SMP, ODD] + [s for p in stores + stores2 for s in p]:
        h.close()


def test_a_world_of_one_over_rccl(corb):
    try:
        uid = corb.Comm.unique_id()
    except corb.CorbError as e:
        pytest.skip("librccl.so does not load here: %s" % e)
    c = G.case("n1")
    comm = corb.Comm(uid, 0, 1); pub = corb.MapPublisher()
    SKF, SMP = S.to_stores(corb, c["server"]["kfs"], c["server"]["mps"], c["F"], c["O"])
    assert comm.map_publish(pub, 0, pack=dict(c["pack"], kf=SKF, mp=SMP)) is None
    want_bytes, counts = S.message_raw(corb, G.message("n1"), c["F"], c["O"])
    assert pub.message_bytes().tobytes() == want_bytes             # the root packed; there was nobody to send to
    for h in (comm, pub, SKF, SMP):
        h.close()

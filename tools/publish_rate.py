"""Host-to-host time of the map publish on records (include/corb_map_publish.h) at the size of a global BA's result: by default 50 000 keyframe pose packets and
5 000 000 map-point position packets, 64 new keyframes and a table of 8 clients.  corb_pub_pack on the server's stores and corb_pub_apply on a client's that holds
every entity as a fixed one (received earlier), each call with its one synchronisation and read-back inside, so a host clock around it is the call's time.

Beside the times stand the bytes the algorithm has to move, computed from the shapes:
  pack    per pose packet 72 B read from the header + 72 B written, per position packet 20 B read + 24 B written, per new record its size read and written
  apply   per pose packet 72 B read, 4 B of flags read, 64 B of pose written; per position packet 24 B + 4 B read, 12 B written; per new record its size twice
(id-table probes, the kind arrays and the read-back are on top and are not counted: the rates are lower bounds of what the memory system did.)
No target is set: nobody has measured this path before.  The numbers go to profiles/publish_rate.json and are printed as one JSON line.
      python tools/publish_rate.py [--poses 50000] [--positions 5000000] [--new-keyframes 64] [--repeats 5]"""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import corbload                                                            # noqa: E402
import publish_cases as G                                                  # noqa: E402

F, O, CHUNK = 8, 4, 250000


def fill_keyframes(corb, KF, first, ids, client_id, flags, rng):
    for at in range(0, len(ids), CHUNK):
        part = ids[at: at + CHUNK]; n = len(part)
        meta = np.zeros(n, corb.KF_META_DTYPE); meta["id"] = part; meta["client_id"] = client_id; meta["flags"] = flags; meta["nlevels"] = 8
        T = np.tile(np.eye(4, dtype=np.float32).reshape(16), (n, 1)); T[:, [3, 7, 11]] = rng.uniform(-100, 100, (n, 3)); meta["Tcw"] = T; meta["TcwGBA"] = T
        KF.put_batch(first + at, meta, np.arange(n + 1, dtype=np.int32), np.zeros(n, corb.KP_DTYPE))


def fill_map_points(corb, MP, first, ids, client_id, flags, rng):
    for at in range(0, len(ids), CHUNK):
        part = ids[at: at + CHUNK]; n = len(part)
        rec = np.zeros(n, corb.MP_RECORD_DTYPE); rec["id"] = part; rec["client_id"] = client_id; rec["flags"] = flags; rec["world_pos"] = rng.uniform(-100, 100, (n, 3))
        MP.put(first + at, rec, np.zeros(n + 1, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=50000); ap.add_argument("--positions", type=int, default=5000000); ap.add_argument("--new-keyframes", type=int, default=64)
    ap.add_argument("--clients", type=int, default=8); ap.add_argument("--repeats", type=int, default=5); ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "publish_rate.json"))
    a = ap.parse_args()
    corb = corbload.load_pkg()
    if corb.device_count() < 1:
        raise SystemExit("publish_rate: no MI355X visible; a time needs the device")
    rng = np.random.default_rng(a.seed)
    nC, nD, nA = a.poses, a.positions, a.new_keyframes
    kf_ids = np.arange(1, nC + nA + 1, dtype=np.uint64) * 7 + 3; mp_ids = np.arange(1, nD + 1, dtype=np.uint64) * 11 + 5
    SKF = corb.KeyFrameStore(nC + nA, F); SMP = corb.MapPointStore(nD, O)
    CKF = corb.KeyFrameStore(nC + nA, F); CMP = corb.MapPointStore(nD, O)
    fill_keyframes(corb, SKF, 0, kf_ids, G.OTHER, 0, rng); fill_map_points(corb, SMP, 0, mp_ids, G.OTHER, 0, rng)
    fill_keyframes(corb, CKF, 0, kf_ids[:nC], G.OTHER, corb.KF_FIXED, rng); fill_map_points(corb, CMP, 0, mp_ids, G.OTHER, corb.MP_FIXED, rng)
    CMP.build_index(0, nD)
    srv = corb.MapPublisher(); cli = corb.MapPublisher()
    trans = [(c + 1, G.pose(rng, 1.0 + 0.05 * c)) for c in range(a.clients)]
    kf_bytes, mp_bytes = SKF.record_bytes(), SMP.record_bytes()
    bytes_pack = nC * (72 + 72) + nD * (20 + 24) + nA * 2 * kf_bytes
    bytes_apply = nC * (72 + 4 + 64) + nD * (24 + 4 + 12) + nA * 2 * kf_bytes
    new_kf, upd_kf, upd_mp = np.arange(nC, nC + nA, dtype=np.int32), np.arange(nC, dtype=np.int32), np.arange(nD, dtype=np.int32)      # (the slot lists exist before the clock starts)
    t_pack, t_apply, t_dry = [], [], []
    out = None
    for rep in range(a.repeats + 2):                                        # two warm-up rounds: code objects, the handles' buffers at their final size
        t0 = time.perf_counter()
        srv.pack(SKF, new_kf_slots=new_kf, upd_kf_slots=upd_kf, mp=SMP, upd_mp_slots=upd_mp, trans=trans)
        t1 = time.perf_counter()
        m = srv.message()
        t2 = time.perf_counter()
        dry = cli.apply(m, G.CLIENT, CKF, 0, nC, nC, nA, CMP, 0, nD, nD, 0, apply=False)
        t3 = time.perf_counter()
        out = cli.apply(m, G.CLIENT, CKF, 0, nC, nC, nA, CMP, 0, nD, nD, 0, apply=True)
        t4 = time.perf_counter()
        assert out["n_kf_inserted"] == nA and out["n_kf_updated"] == nC and out["n_mp_updated"] == nD and dry["n_mp_updated"] == nD, "the publish did not reach every entity"
        fill_keyframes(corb, CKF, nC, kf_ids[nC:] + np.uint64(1), G.OTHER, 0, rng)      # the free slots hold other keyframes again
        if rep >= 2:
            t_pack.append(t1 - t0); t_dry.append(t3 - t2); t_apply.append(t4 - t3)

    def stat(v, nbytes):
        v = np.array(v)
        return dict(median_ms=round(float(np.median(v)) * 1e3, 3), min_ms=round(float(v.min()) * 1e3, 3), max_ms=round(float(v.max()) * 1e3, 3),
                    algorithmic_MB=round(nbytes / 1e6, 2), GBps_at_median=round(nbytes / float(np.median(v)) / 1e9, 1))
    res = dict(poses=nC, positions=nD, new_keyframes=nA, clients=a.clients, repeats=a.repeats, kf_record_bytes=kf_bytes, mp_record_bytes=mp_bytes, message_MB=round(m["bytes"] / 1e6, 2),
               pack=stat(t_pack, bytes_pack), apply=stat(t_apply, bytes_apply), apply_dry_run=stat(t_dry, nC * 76 + nD * 28))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as o:
        json.dump(res, o, indent=1); o.write("\n")
    print(json.dumps(res))
    for h in (srv, cli, SKF, SMP, CKF, CMP):
        h.close()


if __name__ == "__main__":
    main()

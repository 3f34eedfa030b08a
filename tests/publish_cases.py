"""Seeded cases of the map publish (include/corb_map_publish.h) at the smallest shapes that can go wrong; shared by the CPU and the GPU tests.  A case is
dict(F, O, server = dict(kfs, mps), pack = dict(new_kf_slots, upd_kf_slots, new_mp_slots, upd_mp_slots, trans), client = the client dict of tests/publish_reference.py).

Every section of a case with more than a handful of entries mixes, by position, the kinds the rules tell apart:
  A / B   the client's own record; an id the client holds; a new id; a second record with a new id that came earlier (the lowest position is accepted)
  C / D   a held and fixed entity; a held entity of the client's own (not fixed); an unknown id; an id phase A / B of the same call accepts; a second packet
          for a fixed entity that came earlier (the highest position's value stays)
Ids come from records_reference.colliding_ids for the table the kernels build over the section, so probe chains wrap past the last cell.  The client's free slots hold
stale records (every byte of an accepted record has to be overwritten), and their number is exactly what the case accepts (room) unless the case says one less."""
import numpy as np

import publish_reference as R
import records_reference as RR

f32 = np.float32
KP_DTYPE = RR.KP_DTYPE
NO_MAP_POINT = RR.NO_MAP_POINT
CLIENT, OTHER = 2, 5                                    # the client that applies; the client whose records are foreign to it


def _rot(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q); w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def pose(rng, scale=1.0, spread=20.0):
    T = np.eye(4); T[:3, :3] = scale * _rot(rng); T[:3, 3] = rng.uniform(-spread, spread, 3)
    return T.astype(f32)


def kf_record(rng, kid, client_id, flags, F, n=None):
    n = int(rng.integers(1, F + 1)) if n is None else n
    kp = np.zeros(n, KP_DTYPE)
    kp["x"] = rng.uniform(0, 1241, n); kp["y"] = rng.uniform(0, 376, n); kp["size"] = 31; kp["angle"] = rng.uniform(0, 360, n); kp["response"] = rng.uniform(0, 200, n)
    kp["octave"] = rng.integers(0, 8, n); kp["class_id"] = -1
    ids = rng.integers(1, 1 << 40, n, dtype=np.uint64); ids[rng.random(n) < 0.3] = NO_MAP_POINT
    return dict(id=int(kid), client_id=int(client_id), kf_flags=int(flags), nlevels=8, fx=f32(718.856), fy=f32(718.856), cx=f32(607.1928), cy=f32(185.2157), bf=f32(386.1448),
                Tcw=pose(rng), TcwGBA=pose(rng), ba_global_for_kf=int(rng.integers(0, 1000)), inv_level_sigma2=(1 / 1.44 ** np.arange(16)).astype(f32),
                kp=kp, desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), u_right=rng.uniform(-1, 1241, n).astype(f32), depth=rng.uniform(-1, 80, n).astype(f32), mp_id=ids)


def mp_record(rng, pid, client_id, flags, O):
    n_obs = int(rng.integers(0, O + 1))
    kfs = np.sort(rng.choice(np.arange(1, 10000), n_obs, replace=False))
    nrm = rng.normal(size=3); nrm /= np.linalg.norm(nrm)
    return dict(id=int(pid), ref_kf_id=int(kfs[0]) if n_obs else 0, descriptor=rng.integers(0, 256, 32, dtype=np.uint8), client_id=int(client_id), flags=int(flags),
                world_pos=rng.uniform(-50, 50, 3).astype(f32), normal=nrm.astype(f32), min_distance=f32(rng.uniform(0.5, 2)), max_distance=f32(rng.uniform(20, 60)),
                pos_gba=rng.uniform(-50, 50, 3).astype(f32), ba_global_for_kf=int(rng.integers(0, 1000)),
                obs=[(int(k), int(rng.integers(0, 2000))) for k in kfs], n_visible=int(rng.integers(1, 50)), n_found=int(rng.integers(0, 50)), replaced_by=0)


def _side(rng, n_new, n_upd, n_held, make, all_own):
    """one entity kind: (server records, new slots, upd slots, the client's held records)"""
    need = n_held + 2 * n_new + 2 * n_upd + 40
    ids = [int(x) for x in RR.colliding_ids(need, RR.id_table_cells(max(n_new, n_upd, 1)), rng)]
    rng.shuffle(ids)
    take = iter(ids)
    # the client holds: even positions fixed (received from the server earlier), odd ones its own
    held = [make(next(take), OTHER if k % 2 == 0 else CLIENT, R.KF_FIXED if k % 2 == 0 else 0) for k in range(n_held)]
    fixed_ids = [h["id"] for h in held if h["flags_"] & R.KF_FIXED]; own_ids = [h["id"] for h in held if not h["flags_"] & R.KF_FIXED]
    server, new_slots, upd_slots, fresh = [], [], [], []
    for i in range(n_new):
        t = i % 5
        if all_own or t == 1:
            rec = make(next(take), CLIENT, 0)                                   # kind 1
        elif t == 2 and held:
            rec = make(held[i % len(held)]["id"], OTHER, 0)                     # kind 2: held
        elif t == 4 and fresh:
            rec = make(fresh[(i * 7) % len(fresh)], OTHER, 0)                   # kind 2: the id came earlier in this section
        else:
            rec = make(next(take), OTHER, R.KF_BAD if i % 11 == 10 else 0); fresh.append(rec["id"])      # kind 3 (a bad flag is not consulted)
        new_slots.append(len(server)); server.append(rec)
    moved = []
    for i in range(n_upd):
        t = i % 6
        if t == 0 and fixed_ids:
            kid = fixed_ids[(i // 6) % len(fixed_ids)]; moved.append(kid)       # kind 2
        elif t == 1 and own_ids:
            kid = own_ids[(i // 6) % len(own_ids)]                              # kind 1
        elif t == 2 and fresh and not all_own:
            kid = fresh[(i // 6) % len(fresh)]                                  # kind 2: accepted by phase A / B of this call
        elif t == 3 and moved:
            kid = moved[(i * 5) % len(moved)]                                   # kind 2 again: this later value stays
        elif t == 4 and fresh and not all_own:
            kid = fresh[(i * 3) % len(fresh)]
        else:
            kid = next(take)                                                    # kind 0
        upd_slots.append(len(server)); server.append(make(kid, OTHER, 0))
    return server, new_slots, upd_slots, held, list(take)


def make_case(seed, nA=0, nB=0, nC=0, nD=0, F=64, O=4, held=9, scale=1.0, table=(1, CLIENT, 3), all_own=False, kf_short=0, mp_short=0):
    rng = np.random.default_rng(seed)

    def mk_kf(kid, cid, fl):
        r = kf_record(rng, kid, cid, fl, F); r["flags_"] = fl
        return r

    def mk_mp(pid, cid, fl):
        r = mp_record(rng, pid, cid, fl, O); r["flags_"] = fl
        return r
    s_kf, a_slots, c_slots, held_kf, spare_kf = _side(rng, nA, nC, held, mk_kf, all_own)
    s_mp, b_slots, d_slots, held_mp, spare_mp = _side(rng, nB, nD, held, mk_mp, all_own)
    for r in s_kf + s_mp + held_kf + held_mp:
        del r["flags_"]
    if held_kf:
        held_kf[-1]["kp"] = held_kf[-1]["kp"][:0]                              # a held slot without features is no keyframe
        for k in ("desc", "u_right", "depth", "mp_id"):
            held_kf[-1][k] = held_kf[-1][k][:0]
    trans = [(cid, pose(rng, scale * (1 + 0.1 * k))) for k, cid in enumerate(table)]
    pack = dict(new_kf_slots=a_slots, upd_kf_slots=c_slots, new_mp_slots=b_slots, upd_mp_slots=d_slots, trans=trans)
    client = dict(client_id=CLIENT, kfs=list(held_kf), mps=list(held_mp), kf_first=0, kf_n=len(held_kf), kf_free_first=len(held_kf), kf_room=1 << 30,
                  mp_first=0, mp_n=len(held_mp), mp_free_first=len(held_mp), mp_room=1 << 30)
    msg = R.pack(s_kf, a_slots, c_slots, s_mp, b_slots, d_slots, trans)
    out, _ = R.apply(msg, client)
    client["kf_room"] = max(out["n_kf_inserted"] - kf_short, 0); client["mp_room"] = max(out["n_mp_inserted"] - mp_short, 0)
    # the free slots (and one beyond them) hold stale records of other ids
    client["kfs"] += [kf_record(rng, spare_kf[k], OTHER, 0, F) for k in range(client["kf_room"] + 1)]
    client["mps"] += [mp_record(rng, spare_mp[k], OTHER, 0, O) for k in range(client["mp_room"] + 1)]
    return dict(F=F, O=O, server=dict(kfs=s_kf, mps=s_mp), pack=pack, client=client)


CASES = {
    "empty": dict(seed=1),
    "n1": dict(seed=2, nA=1, nB=1, nC=1, nD=1),
    "n255": dict(seed=3, nA=255, nB=255, nC=255, nD=255, F=16),
    "n256": dict(seed=4, nA=256, nB=256, nC=256, nD=256, F=16),
    "n257": dict(seed=5, nA=257, nB=257, nC=257, nD=257, F=16),
    "n513": dict(seed=6, nA=513, nB=513, nC=513, nD=513, F=16),
    "f64": dict(seed=7, nA=12, nB=40, nC=14, nD=44, F=64, O=6),
    "f257": dict(seed=8, nA=7, nB=12, nC=9, nD=13, F=257, O=5),
    "updates_only": dict(seed=9, nC=70, nD=300),
    "inserts_only": dict(seed=10, nA=9, nB=130),
    "kf_room_plus_one": dict(seed=11, nA=12, nB=20, nC=8, nD=9, kf_short=1),
    "mp_room_plus_one": dict(seed=12, nA=12, nB=20, nC=8, nD=9, mp_short=1),
    "all_own": dict(seed=13, nA=10, nB=33, nC=12, nD=20, all_own=True),
    "no_transform": dict(seed=14, nA=10, nB=33, nC=12, nD=20, table=(1, 3, 4)),
    "empty_table": dict(seed=15, nA=3, nB=3, nC=3, nD=3, table=()),
    "scaled": dict(seed=16, nA=10, nB=33, nC=12, nD=20, scale=0.37),
    "nothing_held": dict(seed=17, nA=10, nB=33, nC=12, nD=20, held=0),
}
_cache = {}


def case(name):
    """the case (built once; treat it as read-only)"""
    if name not in _cache:
        _cache[name] = make_case(**CASES[name])
    return _cache[name]


def message(name):
    c = case(name); p = c["pack"]
    key = ("msg", name)
    if key not in _cache:
        _cache[key] = R.pack(c["server"]["kfs"], p["new_kf_slots"], p["upd_kf_slots"], c["server"]["mps"], p["new_mp_slots"], p["upd_mp_slots"], p["trans"])
    return _cache[key]

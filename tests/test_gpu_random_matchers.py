"""GPU parity of the matchers on seeded random scenes (bit-exact index arrays and counts against the oracle): the two order-dependent matchers of
SearchByProjection(KeyFrame*, Scw, ...) and SearchForInitialization drawn as tools/stress_matchers.py draws them, SearchByProjection (map and frame
overloads) and SearchByBoW at sizes below one wave and above 2 048 features, and every matcher entry point with an empty query side and an empty
candidate side -- an empty frame once with its camera's bounds and once with bounds left at zero."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _draw_scw_init(n_cases, seed0):
    rng = np.random.default_rng(99)
    scw, init = [], []
    for it in range(n_cases):
        seed = seed0 + it; n = int(rng.integers(300, 3000)); span = float(rng.choice([1.0, 0.5, 0.3, 0.2]))
        scale = float(np.float32(rng.choice([1.0, 1.05, 0.93]))); th = float(rng.choice([10.0, 4.0, 15.0]))
        scw.append(dict(i=it, seed=seed, n=n, span=span, crowd=bool(it & 1), frac=float(rng.choice([0.3, 0.6])), scale=scale, th=th, claimed=bool(it % 3)))
        init.append(dict(i=it, seed=seed, n=n, span=span, crowd=bool(it & 1), steal=float(rng.choice([0.0, 0.15, 0.4])), ratio=float(rng.choice([0.9, 0.7])),
                         win=int(rng.choice([100, 40, 160])), ori=bool(it & 2)))
    return scw, init


SCW_CASES, INIT_CASES = _draw_scw_init(12, 46000)
_r = np.random.default_rng(460)
MAP_CASES = [dict(i=i, seed=46100 + i, n=n, dense=bool(i & 1), th=float(_r.choice([1.0, 3.0, 5.0])), ratio=float(_r.choice([0.6, 0.8, 0.9])))
             for i, n in enumerate([40, 63, 700, 2100, 2900])]
FRAME_CASES = [dict(i=i, seed=46200 + i, n=n, motion=tuple(float(x) for x in _r.uniform(-0.9, 0.9, 3) * [0.3, 0.1, 1.0]), mono=int(_r.integers(0, 2)),
                    th=float(_r.choice([7.0, 15.0])), ori=bool(_r.integers(0, 2))) for i, n in enumerate([50, 900, 2600])]
BOW_CASES = [dict(i=i, seed=46300 + i, n1=n1, n2=n2, nodes=max(1, min(int(_r.integers(1, 60)), n1 // 10)), ratio=float(_r.choice([0.6, 0.75, 0.9])), ori=bool(_r.integers(0, 2)))
             for i, (n1, n2) in enumerate([(40, 63), (63, 2100), (2500, 1800), (3000, 3000)])]
del _r


def _id(prefix, c, keys):
    return "%s-%03d-" % (prefix, c["i"]) + "-".join("%s_%s" % (k, c[k]) for k in keys)


@pytest.mark.parametrize("c", SCW_CASES, ids=[_id("scw", c, ("n", "span", "th", "crowd", "claimed")) for c in SCW_CASES])
def test_search_by_projection_scw_random_case(corb, pyorc, synth, c):
    sc = synth.keyframe_scene(c["seed"], n=c["n"], span=c["span"])
    if c["crowd"]:
        sc = synth.crowd_keyframe_scene(sc, c["seed"], frac=c["frac"])
    S = sc["T2w"].copy(); S[:3, :] *= np.float32(c["scale"])
    claimed = sc["claimed2"] if c["claimed"] else np.zeros(c["n"], np.uint8)
    g = corb.ORBmatcher(0.6, True).SearchByProjection_Scw(sc["kf2"], claimed, S, sc["pts1"], sc["desc1"], c["th"])
    r = pyorc.search_by_projection_scw(sc["kf2"], claimed, S, sc["pts1"], sc["desc1"], c["th"])
    assert np.array_equal(g[0], r[0]) and g[1] == r[1]
    assert r[1] > 0


@pytest.mark.parametrize("c", INIT_CASES, ids=[_id("init", c, ("n", "span", "steal", "ratio", "win", "ori")) for c in INIT_CASES])
def test_search_for_initialization_random_case(corb, pyorc, synth, c):
    f1, f2, pm, _ = synth.monocular_init_pair(c["seed"], n=c["n"], span=c["span"], crowd=c["crowd"], steal_frac=c["steal"])
    g = corb.ORBmatcher(c["ratio"], c["ori"]).SearchForInitialization(f1, f2, pm, c["win"])
    r = pyorc.search_for_initialization(f1, f2, pm, c["win"], c["ratio"], c["ori"])
    assert np.array_equal(g[0], r[0]) and np.array_equal(g[1], r[1]) and g[2] == r[2]
    assert r[2] > 0


@pytest.mark.parametrize("c", MAP_CASES, ids=[_id("map", c, ("n", "dense", "th", "ratio")) for c in MAP_CASES])
def test_search_by_projection_map_random_case(corb, pyorc, synth, c):
    s = synth.tracking_scene(seed=c["seed"], n=c["n"], dense=c["dense"])
    g, gn = corb.ORBmatcher(c["ratio"], True).SearchByProjection(s["cur"], s["mps"], s["last_desc"], c["th"])
    r, rn = pyorc.search_by_projection_map(s["cur"], s["mps"], s["last_desc"], c["th"], c["ratio"])
    assert gn == rn and np.array_equal(g, r)
    assert rn > 0


@pytest.mark.parametrize("c", FRAME_CASES, ids=[_id("frame", c, ("n", "mono", "th", "ori")) for c in FRAME_CASES])
def test_search_by_projection_frame_random_case(corb, pyorc, synth, c):
    s = synth.tracking_scene(seed=c["seed"], n=c["n"], motion=c["motion"])
    a = (s["cur"], s["Tcw"], s["Tlw"], s["fx"], s["fy"], s["cx"], s["cy"], s["bf"], s["mb"], s["last"], s["last_desc"], c["th"], c["mono"])
    g, gn = corb.ORBmatcher(0.9, c["ori"]).SearchByProjection_Frame(*a)
    r, rn = pyorc.search_by_projection_frame(*a, int(c["ori"]))
    assert gn == rn and np.array_equal(g, r)
    assert rn > 0


def _bow_inputs(synth, c):
    from test_oracle_match import _make
    return _make(np.random.default_rng(c["seed"]), synth, c["n1"], c["n2"], c["nodes"])


@pytest.mark.parametrize("c", BOW_CASES, ids=[_id("bow", c, ("n1", "n2", "nodes", "ratio", "ori")) for c in BOW_CASES])
def test_search_by_bow_random_case(corb, pyorc, synth, c):
    d1, a1, v1, fv1, d2, a2, v2, fv2 = _bow_inputs(synth, c)
    m = corb.ORBmatcher(c["ratio"], c["ori"])
    g0, n0 = m.SearchByBoW(dict(desc=d1, angle=a1, valid=v1, fv=fv1), dict(desc=d2, angle=a2, valid=v2, fv=fv2))
    r0, rn0 = pyorc.search_by_bow(0, d1, a1, v1, pyorc.FeatVec(*fv1), d2, a2, v2, pyorc.FeatVec(*fv2), c["ratio"], c["ori"])
    assert np.array_equal(g0, r0) and n0 == rn0
    g1, n1 = m.SearchByBoW_KFKF(dict(desc=d1, angle=a1, valid=v1, fv=fv1), dict(desc=d2, angle=a2, valid=v2, fv=fv2))
    r1, rn1 = pyorc.search_by_bow(1, d1, a1, v1, pyorc.FeatVec(*fv1), d2, a2, v2, pyorc.FeatVec(*fv2), c["ratio"], c["ori"])
    assert np.array_equal(g1, r1) and n1 == rn1
    assert rn0 > 0 and rn1 > 0


# ---- empty inputs: every matcher entry point, the query side empty and then the candidate side; an empty frame with its camera's bounds and with zero bounds

def _empty_view(v, zero_bounds):
    """a view of the same camera without features (keys, descriptors and the per-feature arrays cut to 0); zero_bounds: min / max left at 0"""
    e = dict(v)
    for k in ("keys_un", "u_right", "desc", "claimed"):
        if k in e:
            e[k] = e[k][:0]
    if zero_bounds:
        e["min_x"] = e["min_y"] = e["max_x"] = e["max_y"] = 0.0
    return e


def _all_minus_one(a):
    return bool(np.all(np.asarray(a) == -1))


EMPTY_SIDES = [(side, zb) for side in ("query", "candidate") for zb in (False, True)]


@pytest.mark.parametrize("side,zero_bounds", EMPTY_SIDES, ids=["%s-empty%s" % (s, "-zero-bounds" if z else "") for s, z in EMPTY_SIDES])
def test_projection_matchers_on_empty_inputs(corb, pyorc, synth, side, zero_bounds):
    """SearchByProjection (map and frame), SearchByProjection_Reloc, SearchByProjection_Scw, Fuse (both overloads), SearchBySim3 and
    SearchForInitialization: no error, every slot -1 and a count of 0, as the oracle returns"""
    mt = corb.ORBmatcher(0.8, True)
    s = synth.tracking_scene(seed=46400, n=300)
    sc = synth.keyframe_scene(46401, n=300)
    f1, f2, pm, _ = synth.monocular_init_pair(46402, n=300)
    cur, mps, ldesc, last = s["cur"], s["mps"], s["last_desc"], s["last"]
    kf2, pts1, desc1, kf1, pts2, desc2 = sc["kf2"], sc["pts1"], sc["desc1"], sc["kf1"], sc["pts2"], sc["desc2"]
    claimed = sc["claimed2"]
    if side == "query":           # the map points / last frame / points to project / F1 empty; an empty F1 (or KF1) view also gets the bounds variant
        mps, ldesc, last = mps[:0], ldesc[:0], last[:0]
        pts1, desc1 = pts1[:0], desc1[:0]
        f1 = _empty_view(f1, zero_bounds); pm = pm[:0]
        kf1 = _empty_view(kf1, zero_bounds)
    else:                         # the frame / keyframe searched in empty
        cur = _empty_view(cur, zero_bounds)
        kf2 = _empty_view(kf2, zero_bounds); claimed = claimed[:0]
        f2 = _empty_view(f2, zero_bounds)
        pts2b, desc2b = pts2[:0], desc2[:0]
    # SearchByProjection(Frame&, vector<MapPoint*>)
    g = mt.SearchByProjection(cur, mps, ldesc, 3.0); r = pyorc.search_by_projection_map(cur, mps, ldesc, 3.0, 0.8)
    assert g[1] == r[1] == 0 and np.array_equal(g[0], r[0]) and _all_minus_one(g[0]) and len(g[0]) == len(cur["keys_un"])
    # SearchByProjection(Frame&, const Frame&)
    a = (cur, s["Tcw"], s["Tlw"], s["fx"], s["fy"], s["cx"], s["cy"], s["bf"], s["mb"], last, s["last_desc"][: len(last)], 7.0, 0)
    g = mt.SearchByProjection_Frame(*a); r = pyorc.search_by_projection_frame(*a, 1)
    assert g[1] == r[1] == 0 and np.array_equal(g[0], r[0]) and _all_minus_one(g[0])
    # SearchByProjection(Frame&, KeyFrame*, set, th, ORBdist) and (KeyFrame*, Scw, ...)
    cl = claimed if side == "candidate" else np.zeros(len(kf2["keys_un"]), np.uint8)
    g = mt.SearchByProjection_Reloc(kf2, cl, sc["T2w"], pts1, desc1, 10.0, 100); r = pyorc.search_by_projection_reloc(kf2, cl, sc["T2w"], pts1, desc1, 10.0, 100, True)
    assert g[1] == r[1] == 0 and np.array_equal(g[0], r[0]) and _all_minus_one(g[0])
    g = mt.SearchByProjection_Scw(kf2, cl, sc["T2w"], pts1, desc1, 10.0); r = pyorc.search_by_projection_scw(kf2, cl, sc["T2w"], pts1, desc1, 10.0)
    assert g[1] == r[1] == 0 and np.array_equal(g[0], r[0]) and _all_minus_one(g[0])
    # Fuse(KeyFrame*, vpMapPoints) and Fuse(KeyFrame*, Scw, ...)
    for sim3 in (False, True):
        g = mt.Fuse(kf2, sc["T2w"], sc["Ow2"], pts1, desc1, 3.0, sim3=sim3); r = pyorc.fuse(kf2, sc["T2w"], sc["Ow2"], int(sim3), pts1, desc1, 3.0)
        assert g[2] == r[2] == 0 and np.array_equal(g[0], r[0]) and np.array_equal(g[1], r[1]) and _all_minus_one(g[0])
    # SearchBySim3(KF1, KF2): KF1 (and its map points) or KF2 (and its map points) empty
    if side == "query":
        a = (kf1, sc["kf2"], sc["T1w"], sc["T2w"], pts1, desc1, pts2, desc2, sc["s12"], sc["R12"], sc["t12"], 7.5)
    else:
        a = (sc["kf1"], kf2, sc["T1w"], sc["T2w"], sc["pts1"], sc["desc1"], pts2b, desc2b, sc["s12"], sc["R12"], sc["t12"], 7.5)
    g = mt.SearchBySim3(*a); r = pyorc.search_by_sim3(*a)
    assert g[1] == r[1] == 0 and np.array_equal(g[0], r[0]) and _all_minus_one(g[0])
    # SearchForInitialization(F1, F2)
    g = mt.SearchForInitialization(f1, f2, pm, 100); r = pyorc.search_for_initialization(f1, f2, pm, 100, 0.8, True)
    assert g[2] == r[2] == 0 and np.array_equal(g[0], r[0]) and np.array_equal(g[1], r[1]) and _all_minus_one(g[0])


@pytest.mark.parametrize("side", ["query", "candidate"])
def test_descriptor_matchers_on_empty_inputs(corb, pyorc, synth, side):
    """SearchByBoW (both variants) and SearchForTriangulation with one side empty: no error, no match, as the oracle"""
    rng = np.random.default_rng(46500)
    d1, a1, v1, fv1, d2, a2, v2, fv2 = _bow_inputs(synth, dict(seed=46500, n1=200, n2=180, nodes=9))
    empty_fv = (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32))
    if side == "query":
        d1, a1, v1, fv1 = d1[:0], a1[:0], v1[:0], empty_fv
    else:
        d2, a2, v2, fv2 = d2[:0], a2[:0], v2[:0], empty_fv
    m = corb.ORBmatcher(0.75, True)
    for variant in (0, 1):
        call = m.SearchByBoW if variant == 0 else m.SearchByBoW_KFKF
        g, gn = call(dict(desc=d1, angle=a1, valid=v1, fv=fv1), dict(desc=d2, angle=a2, valid=v2, fv=fv2))
        r, rn = pyorc.search_by_bow(variant, d1, a1, v1, pyorc.FeatVec(*fv1), d2, a2, v2, pyorc.FeatVec(*fv2), 0.75, True)
        assert gn == rn == 0 and np.array_equal(g, r) and _all_minus_one(g)
    n1, n2 = len(d1), len(d2)
    kp1 = np.zeros(n1, corb.KP_DTYPE); kp2 = np.zeros(n2, corb.KP_DTYPE)
    kp1["x"] = rng.uniform(0, 1241, n1); kp1["y"] = rng.uniform(0, 376, n1); kp2["x"] = rng.uniform(0, 1241, n2); kp2["y"] = rng.uniform(0, 376, n2)
    ur1 = np.full(n1, -1, np.float32); ur2 = np.full(n2, -1, np.float32); mp1 = np.zeros(n1, np.uint8); mp2 = np.zeros(n2, np.uint8)
    scale = (np.float32(1.2) ** np.arange(8)).astype(np.float32); sigma2 = scale * scale
    F12 = np.array([[0, -1e-4, 0.02], [1e-4, 0, -0.06], [-0.02, 0.06, 1.0]], np.float32)
    gp, gn = m.SearchForTriangulation(dict(desc=d1, kp=kp1, u_right=ur1, has_mp=mp1, fv=fv1), dict(desc=d2, kp=kp2, u_right=ur2, has_mp=mp2, fv=fv2),
                                      F12, 600.0, 180.0, scale, sigma2, False)
    rp, rn = pyorc.search_for_triangulation(d1, kp1, ur1, mp1, pyorc.FeatVec(*fv1), d2, kp2, ur2, mp2, pyorc.FeatVec(*fv2), F12, 600.0, 180.0, scale, sigma2, False, True)
    assert gn == rn == 0 and len(gp) == len(rp) == 0

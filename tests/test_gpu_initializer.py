"""GPU tests: the monocular Initializer on the device (corb_mono_initialize, the Initializer class) against tests/initializer_reference.py, bit for bit: every field of
CorbInitResult except `parallax` (NaN equal to NaN: payloads are not part of a reading), vP3D, vbTriangulated, both inlier sets and the scores of every hypothesis.
`parallax` is held to the host formula applied to the returned cosine.  Cases (tests/gpu_init_cases.py): N = 8 (every draw set a permutation), 9, 63, 64, 65 (around
the 64-match mask words and the 50-point threshold), 129 and 200; 1 and 200 iterations; general, planar, pure-rotation and degenerate scenes; the forced tie; the NaN
flow of coincident keys; a batch of three problems with strides larger than needed; the argument errors; the class; and one comparison with ground truth."""
import ctypes as C
import numpy as np
import pytest
import initializer_reference as R
import gpu_init_cases as G

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b).astype(a.dtype)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))
    return bool(np.array_equal(a, b))


def check(name, got, want):
    e = got["result"]
    for k in R.RESULT_DTYPE.names:
        if k != "parallax":
            assert same_bits(e[k], np.asarray(want[k], R.RESULT_DTYPE[k].base)), (name, k, e[k], want[k])
    n_hyp = 0 if e["status"] in (R.NO_MODEL, R.H_DEGENERATE) else (4 if e["model"] else 8)
    par = [R.parallax_of(c) if k < n_hyp else np.float32(0) for k, c in enumerate(e["cos_parallax"])]
    assert same_bits(e["parallax"], np.array(par, np.float32)), (name, e["parallax"], par)
    for k in ("p3d", "triangulated", "inliers_h", "inliers_f", "scores"):
        assert same_bits(got[k], want[k]), (name, k)


def run(corb, cases, **kw):
    p = dict(cases[0]["params"])
    return corb.MonoInitialize([c["problem"] for c in cases], np.stack([c["rand"] for c in cases]), **p, **kw)


@pytest.mark.parametrize("name", sorted(G.cases()))
def test_initialize_is_the_definition_bit_for_bit(corb, name):
    case = G.cases()[name]
    check(name, run(corb, [case])[0], G.expected(name))


def test_the_cases_cover_every_status_and_both_models():
    seen = {(G.expected(n)["status"], G.expected(n)["model"]) for n in G.cases()}
    assert {s for s, _ in seen} == set(range(6)) and {(R.OK, 0), (R.OK, 1)} <= seen


def test_batch_of_three_with_larger_strides(corb):
    cases = G.batch()
    n1 = max(len(c["problem"]["keys1"]) for c in cases); N = max(int((c["problem"]["matches12"] >= 0).sum()) for c in cases)
    got = run(corb, cases, p3d_stride=n1 + 13, flags_stride=N + 70)
    for c, g in zip(cases, got):
        check(c["name"], g, G.expected(c["name"]))
        k1 = len(c["problem"]["keys1"]); n = int((c["problem"]["matches12"] >= 0).sum())
        assert not g["raw"]["p3d"][k1:].any() and not g["raw"]["triangulated"][k1:].any() and not g["raw"]["inliers_h"][n:].any() and not g["raw"]["inliers_f"][n:].any()
    assert len({g["result"]["n_matches"] for g in got}) == 3


def test_forced_tie_keeps_the_earlier_iteration(corb):
    g = run(corb, [G.cases()["tie65"]])[0]
    sc = g["scores"]
    assert same_bits(sc[2], sc[0]) and same_bits(sc[3], sc[1]) and (sc[:2] > 0).all()
    assert g["result"]["best_it_h"] in (0, 1) and g["result"]["best_it_f"] in (0, 1)


def test_failed_status_keeps_diagnostics_and_zeroes_the_motion(corb):
    g = run(corb, [G.cases()["rotation129"]])[0]; e = g["result"]
    assert e["status"] == R.LOW_PARALLAX and e["n_good"][:8].max() > 50 and e["score_h"] > 0 and g["inliers_h"].sum() == e["n_inliers"]
    assert not e["R21"].any() and not e["t21"].any() and not g["p3d"].any() and not g["triangulated"].any() and e["n_triangulated"] == 0


def test_argument_errors_write_nothing(corb):
    case = G.cases()["general65"]; pr = case["problem"]; p = case["params"]
    L = corb.load(); its = p["max_iterations"]

    def call(pr, rand, sigma=1.0, its=its):
        k1, k2 = corb._keys(pr["keys1"]), corb._keys(pr["keys2"]); m = np.ascontiguousarray(pr["matches12"], np.int32)
        arr = (corb._InitProblem * 1)(corb._InitProblem(corb._p(k1), len(k1), corb._p(k2), len(k2), corb._p(m), *[float(np.float32(v)) for v in pr["K"]]))
        res = np.zeros(1, corb.INIT_RESULT_DTYPE).view(np.uint8); res[:] = 0xAB
        p3d = np.full((len(k1), 3), 5.0, np.float32); tri = np.full(len(k1), 9, np.uint8); ih = np.full(len(m), 9, np.uint8); i_f = ih.copy()
        sc = np.full((max(its, 1), 2), 5.0, np.float32); rv = np.ascontiguousarray(rand, np.int32)
        rc = L.corb_mono_initialize(C.cast(arr, C.c_void_p), 1, sigma, its, 1.0, 50, corb._p(rv), len(k1), len(m), corb._p(res), corb._p(p3d), corb._p(tri), corb._p(ih),
                                    corb._p(i_f), corb._p(sc), 0)
        untouched = (res == 0xAB).all() and (p3d == 5.0).all() and (tri == 9).all() and (ih == 9).all() and (i_f == 9).all() and (sc == 5.0).all()
        return rc, untouched

    assert call(pr, case["rand"])[0] == 0
    few = dict(pr); m = pr["matches12"].copy(); m[np.nonzero(m >= 0)[0][7:]] = -1; few["matches12"] = m             # N = 7
    bad_index = dict(pr); m = pr["matches12"].copy(); m[np.nonzero(m >= 0)[0][3]] = len(pr["keys2"]); bad_index["matches12"] = m
    below = dict(pr); m = pr["matches12"].copy(); m[0] = -2; below["matches12"] = m
    bad_rand = case["rand"].copy().astype(np.int64); bad_rand[5, 3] = -1
    for args in ((few, case["rand"]), (bad_index, case["rand"]), (below, case["rand"]), (pr, case["rand"], 0.0), (pr, case["rand"], -1.0), (pr, case["rand"], 1.0, 0),
                 (pr, np.zeros((65536, 8), np.int32), 1.0, 65536), (pr, bad_rand)):
        rc, untouched = call(*args)
        assert rc == -1 and untouched, args[2:]                                                                     # CORB_ERR_ARG


def test_initializer_class_equals_a_direct_call(corb):
    case = G.cases()["general129"]; pr = case["problem"]
    direct = run(corb, [case])[0]
    ini = corb.Initializer(pr["keys1"], pr["K"], sigma=1.0, iterations=200)
    ok, R21, t21, vP3D, vbTriangulated = ini.Initialize(pr["keys2"], pr["matches12"], case["rand"])
    e = direct["result"]
    assert ok and e["status"] == R.OK
    assert same_bits(R21.reshape(9), e["R21"]) and same_bits(t21, e["t21"]) and same_bits(vP3D, direct["p3d"]) and np.array_equal(vbTriangulated, direct["triangulated"])
    assert ini.last["result"].tobytes() == e.tobytes()


def test_device_answer_against_ground_truth(corb):
    """the general N = 129 scene against the scene's own motion and points, within the bars of test_initializer_reference.py (measured there on the definition)"""
    import test_initializer_reference as T
    pr, truth = G.scene(105, 129, "general")
    g = corb.MonoInitialize([pr], R.draws(105, 1, 200), **G.PARAMS)[0]; e = g["result"]
    assert e["status"] == R.OK and e["model"] == 1
    rot, direction, points = T.truth_errors(e["R21"], e["t21"], g["p3d"], g["triangulated"], truth)
    print("rotation %.3g direction %.3g points %.3g" % (rot, direction, points))
    assert rot <= T.BAR_ROTATION and direction <= T.BAR_DIRECTION and points <= T.BAR_POINTS

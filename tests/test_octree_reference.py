"""tests/octree_reference.py against the serial oracle (CPU only): the kinds that tests/test_gpu_octree_kinds.py counts are kinds of the oracle's own run only
if the reference keeps exactly the keys pyorc.distribute_octree keeps, in the same order -- on every level of every GPU case, and on seeded random key
sets as in the self-test of tools/octree_proto.py (whose formulation the reference restates: both are run and must agree)."""
import importlib.util
import os
import numpy as np

import octree_cases as OC
import octree_reference as OR


def _proto():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "octree_proto.py")
    spec = importlib.util.spec_from_file_location("octree_proto", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _check(pyorc, proto, kps, W, H, N, what):
    want = pyorc.distribute_octree(kps, 16, 16 + W, 16, 16 + H, N)
    sel, kinds = OR.distribute(kps["x"], kps["y"], kps["response"], 16, 16 + W, 16, 16 + H, N)
    got = kps[sel]
    assert len(got) == len(want) and got.tobytes() == want.tobytes(), "%s: the reference keeps other keys than the oracle (%d / %d)" % (what, len(got), len(want))
    if proto is not None:
        assert np.array_equal(proto.distribute(kps["x"], kps["y"], kps["response"], 16, 16 + W, 16, 16 + H, N), sel), "%s: the reference and tools/octree_proto.py disagree" % what
    return kinds


def test_reference_equals_oracle_on_every_case_level(pyorc):
    proto = _proto()
    for name in OC.CASES:
        c = OC.classified(pyorc, name)
        scale = c.ref.tables()["scale"]
        off = 0
        for l in range(c.nlevels):
            w, h = c.sizes[l]
            cd = c.cands[l]
            assert c.kinds[l]["n"] == len(cd)
            if len(cd) == 0:
                assert c.counts[l] == 0 and len(c.sel[l]) == 0
                continue
            assert cd["x"].max() <= w - 32 - 4 and cd["y"].max() <= h - 32 - 4          # FAST leaves a 3-px ring inside the detection area: no key reaches x / hX == nIni
            k = _check(pyorc, proto, cd, w - 32, h - 32, int(c.quota[l]), "%s level %d" % (name, l))
            assert k == c.kinds[l]
            # the final keypoints of the level ARE these keys, in this order: the quadtree result travels in them
            kept, fin = cd[c.sel[l]], c.kps[off:off + c.counts[l]]
            assert len(kept) == c.counts[l] and (fin["octave"] == l).all()
            fx, fy = (kept["x"] + np.float32(16)), (kept["y"] + np.float32(16))
            if l:
                fx, fy = fx * scale[l], fy * scale[l]
            assert np.array_equal(fin["x"], fx) and np.array_equal(fin["y"], fy) and np.array_equal(fin["response"], kept["response"]), "%s level %d" % (name, l)
            off += c.counts[l]
        assert off == len(c.kps)


def test_reference_equals_oracle_on_random_key_sets(pyorc):
    """300 seeded key sets as in tools/octree_proto.py (distinct pixels, few response values on every third), every seventh small; every fifth also holds keys ON
    the right border (x == W), the only way to x / hX == nIni: the extractor never produces one, so the clamp is pinned to the oracle here and nowhere else."""
    proto = _proto()
    rng = np.random.default_rng(1)
    total = {}
    for t in range(300):
        W = int(rng.integers(40, 1300)); H = int(rng.integers(40, 400))
        if W < H // 2:
            W = H
        n = int(rng.integers(1, 3000)) if t % 7 else int(rng.integers(1, 30))
        N = int(rng.integers(1, 500))
        cells = rng.choice(W * H, size=min(n, W * H), replace=False)
        x = (cells % W).astype(np.float32); y = (cells // W).astype(np.float32)
        if t % 5 == 0:
            x[rng.integers(0, len(x), 3)] = W
        order = np.lexsort((x, y)); x, y = x[order], y[order]
        kps = np.zeros(len(x), pyorc.KP_DTYPE)
        kps["x"], kps["y"], kps["response"] = x, y, rng.integers(7, 60 if t % 3 else 12, size=len(x)).astype(np.float32)
        kps["class_id"] = np.arange(len(x))                     # keys at one position (two keys moved to x == W in one row) stay distinguishable
        OR.add_kinds(total, _check(pyorc, proto if t % 4 == 0 else None, kps, W, H, N, "trial %d" % t))
    print("\nquadtree kinds over 300 random key sets:", total)
    for kd in ("ini_clamp", "empty_ini", "passes_B", "b_stop_mid", "b_tie_at_stop", "b_tie_any", "end_by_stall", "end_by_quota_A", "end_by_quota_B", "best_tie", "single_key"):
        assert total[kd] > 0, "no random key set is of kind '%s'" % kd

"""Seeded cases for the local-map tests: the maps of tests/covis_cases.py with a spanning tree grown by UpdateConnections, current frames that hold points of a run
of keyframes, and culling sequences.  tests/test_localmap_reference.py checks that these generators reach every event the readings are about (localmap_reference's
Map.stats); the GPU tests then compare the device routes with localmap_reference on exactly these cases."""
import numpy as np

import covis_cases as G
import localmap_reference as LR

NO_ID = LR.NO_ID
FRAME_ID = 77777777             # mnId of the current frame's record: no keyframe of the maps, no observer of a point


def grown_map(seed, tree=None, **kw):
    """a random map whose keyframes were all connected once, in ascending id: rows and tree as UpdateConnections leaves them.  tree = "chain": the tree is then
    replaced by the chain of the ids (every keyframe the child of the one before it), as a map loaded from an archive may deliver it -- no parent of a voter but the
    first one's lies outside a run of voters, so the neighbour walk goes on; tree = "star": every keyframe is a child of the first."""
    m = G.random_map(seed=seed, **kw)
    for k in sorted(m.kfs):
        LR.update_connections(m, k)
    retree(m, tree)
    return m


def retree(m, tree):
    """replaces the tree of the whole map: "chain" or "star" (grown_map); None leaves it"""
    ids = sorted(m.kfs)
    for a, k in enumerate(ids):
        if tree == "chain":
            LR.set_tree(m, k, ids[a - 1] if a else None, False, ids[a + 1: a + 2])
        elif tree == "star":
            LR.set_tree(m, k, ids[0] if a else None, False, ids[1:] if a == 0 else [])


def frame_for(m, seed, n_feat, first, width, p_none=0.1, p_dangling=0.05, only_bad=False):
    """a current frame of n_feat features whose points are drawn from the keyframes first .. first + width (positions in ascending id): the points of TrackWithMotionModel /
    TrackReferenceKeyFrame.  p_none: features without a point; p_dangling: ids no record has.  only_bad: bad points, dangling ids and NULLs only (an empty counter)."""
    rng = np.random.default_rng(seed)
    if first == "bad":                                          # the run starts at the first bad keyframe: with width 1 it holds the most votes
        first = next(a for a, k in enumerate(sorted(m.kfs)) if m.kfs[k].bad)
    ids = sorted(m.kfs)[first: first + width]
    pool = sorted({p for k in ids for p in m.kfs[k].mp_ids if p != NO_ID and p in m.mps and (m.mps[p].bad or not only_bad)})
    out = []
    for _ in range(n_feat):
        u = rng.random()
        if u < p_none or not pool:
            out.append(NO_ID)
        elif u < p_none + p_dangling:
            out.append(600000000 + int(rng.integers(0, 1000)))
        else:
            out.append(pool[int(rng.integers(len(pool)))])
    return LR.Frame(out)


# name -> (map arguments, [(frame seed, features, first keyframe, width, extra)]): stores of 8 to 128 keyframes with 32 to 64 features
LOCALMAP_CASES = {
    "k8": (dict(seed=31, n_kf=8, F=32, span=3, p_bad_kf=0.15), [(1, 32, 0, 3, {}), (2, 40, 2, 6, {}), (3, 16, 0, 8, dict(only_bad=True))]),
    "k20": (dict(seed=32, n_kf=20, F=48, span=5, sparse=(7,), p_bad_kf=0.15, p_unknown=0.3), [(4, 64, 3, 6, {}), (5, 320, 0, 20, {}), (6, 50, 10, 4, {}), (7, 8, 5, 2, {}), (15, 40, "bad", 1, {})]),
    "k20_chain": (dict(seed=35, n_kf=20, F=48, span=5, p_bad_kf=0.15, p_unknown=0.3, tree="chain"), [(16, 24, 0, 2, {}), (17, 64, 0, 6, {}), (18, 40, 4, 3, {})]),
    "k20_star": (dict(seed=36, n_kf=20, F=48, span=5, p_bad_kf=0.2, tree="star"), [(19, 24, 0, 3, {}), (20, 64, 0, 8, {})]),
    "k40_id0": (dict(seed=33, n_kf=40, F=64, span=8, max_obs=10, id0=True, p_bad_kf=0.2), [(8, 64, 0, 5, {}), (9, 200, 12, 20, {}), (10, 33, 30, 10, {})]),
    "k128": (dict(seed=34, n_kf=128, F=40, span=4, p_bad_kf=0.05), [(11, 320, 0, 75, {}), (12, 320, 10, 118, dict(p_none=0.0, p_dangling=0.0)), (13, 320, 40, 70, {}), (14, 64, 100, 28, {})]),
    "k128_chain": (dict(seed=37, n_kf=128, F=40, span=4, p_bad_kf=0.05, tree="chain"), [(21, 320, 0, 72, {}), (22, 320, 0, 60, {})]),
}


def culling_sequence(m, seed, n):
    """n keyframes to cull one after the other (never mnId 0): ids in the order SetBadFlag meets them"""
    rng = np.random.default_rng(seed)
    ids = [k for k in sorted(m.kfs) if k != 0]
    return [ids[int(i)] for i in rng.permutation(len(ids))[:n]]                # (indices: ids spread over 64 bits do not survive a numpy array of mixed width)


def set_bad_flag(m, kid):
    """KeyFrame::SetBadFlag as the callers of the device route order it: the connections (covis_reference.erase_connections), the tree, then the flag the caller sets
    whatever the reference's `if` of :658 decided (LocalMapping culls the keyframe either way)"""
    G.R.erase_connections(m, kid)
    r = LR.reparent_children(m, kid)
    m.kfs[kid].bad = True
    return r


def trees(m, kf_order):
    """every tree state as corb_covis_get_tree returns it: [(parent or NO_ID, first, [children])] in slot order"""
    out = []
    for k in kf_order:
        p, f, c = LR.get_tree(m, k)
        out.append((NO_ID if p is None else p, f, c))
    return out

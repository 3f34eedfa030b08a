"""Seeded training cases shared by the vocabulary-training tests (host program and device), and the definition's answer for each, computed once per process."""
import functools
import struct
import numpy as np

import voctrain_reference as V

# name -> (k, L, features, images, kind, seed, max_iterations)
CASES = {
    "k2L1n3": (2, 1, 3, 1, "uniform", 11, 100),
    "k2L2n5": (2, 2, 5, 2, "uniform", 12, 100),
    "k3L3n200": (3, 3, 200, 7, "clustered", 13, 100),
    "k10L3n3000": (10, 3, 3000, 12, "clustered", 14, 100),
    "k20L2n1500": (20, 2, 1500, 5, "clustered", 15, 100),
    "n1": (3, 2, 1, 1, "uniform", 16, 100),
    "nk": (3, 2, 3, 1, "uniform", 17, 100),
    "nk1": (3, 2, 4, 3, "uniform", 18, 100),
    "lowent": (4, 5, 600, 4, "lowent", 19, 100),
    "repeat": (10, 3, 1200, 3, "repeat", 20, 100),
    "cap1": (10, 3, 3000, 12, "clustered", 14, 1),
    "cap2": (10, 3, 3000, 12, "clustered", 14, 2),
    "cap2small": (3, 3, 200, 7, "clustered", 13, 2),
}
CORE = ["k2L1n3", "k2L2n5", "k3L3n200", "k10L3n3000", "k20L2n1500", "n1", "nk", "nk1"]


def descriptors(kind, n, rng):
    if kind == "uniform":
        return rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if kind == "clustered":                                     # noisy copies of a few centres, so that the tree is not degenerate
        centres = rng.integers(0, 256, (max(2, n // 60), 32), dtype=np.uint8)
        noise = np.packbits(rng.random((n, 256)) < 0.08, axis=1)
        return np.bitwise_xor(centres[rng.integers(0, len(centres), n)], noise)
    if kind == "lowent":                                        # only the first two bytes vary: distance ties and exact-half majorities
        d = np.zeros((n, 32), np.uint8); d[:, :2] = rng.integers(0, 256, (n, 2), dtype=np.uint8)
        return d
    if kind == "repeat":                                        # 40 distinct descriptors, each 30 times: dist_sum == 0, trivial nodes, single-member clusters
        base = rng.integers(0, 256, (40, 32), dtype=np.uint8)
        return base[rng.permutation(np.repeat(np.arange(40), n // 40))]
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (sets, k, L, seed, max_iterations); with more than two images, the second one is empty"""
    k, L, n, images, kind, seed, max_it = CASES[name]
    rng = np.random.default_rng(1000 + seed)
    d = descriptors(kind, n, rng)
    free = [i for i in range(images) if not (images > 2 and i == 1)]
    cuts = np.sort(rng.integers(0, n + 1, len(free) - 1)) if len(free) > 1 else np.zeros(0, np.int64)
    sizes = np.diff(np.concatenate([[0], cuts, [n]])).astype(int)
    sets, at, j = [], 0, 0
    for i in range(images):
        m = int(sizes[j]) if i in free else 0
        j += i in free
        sets.append(d[at:at + m].copy()); at += m
    assert at == n
    return sets, k, L, seed, max_it


@functools.lru_cache(maxsize=None)
def expected(name):
    """the definition's (flat, stats); callers must not modify it"""
    sets, k, L, seed, max_it = inputs(name)
    return V.create(sets, k, L, seed, max_it)


def write_case(o, sets, k, L, seed, max_it):
    off = np.zeros(len(sets) + 1, "<i4"); off[1:] = np.cumsum([len(s) for s in sets])
    o.write(struct.pack("<4iQ", k, L, max_it, len(sets), seed)); o.write(off.tobytes())
    for s in sets:
        o.write(np.ascontiguousarray(s, np.uint8).tobytes())


def result_text(flat, st):
    """one case as tests/host/voctrain_main.cpp prints it"""
    n = len(flat["parent"])
    return ["C %d" % n, "p" + "".join(" %d" % p for p in flat["parent"]), "l" + "".join(" %d" % p for p in flat["is_leaf"]), "d " + flat["descriptor"].tobytes().hex(),
            "w" + "".join(" %016x" % int(x) for x in flat["weight"].view(np.uint64)), "s" + "".join(" %d" % st[f] for f in V.STAT_FIELDS),
            "ln" + "".join(" %d" % x for x in st["level_nodes"]), "li" + "".join(" %d" % x for x in st["level_max_iterations"])]


def same_flat(a, b):
    return (a["k"], a["L"]) == (b["k"], b["L"]) and np.array_equal(a["parent"], b["parent"]) and np.array_equal(a["is_leaf"], b["is_leaf"]) and \
        np.array_equal(a["descriptor"], b["descriptor"]) and np.array_equal(np.asarray(a["weight"], np.float64).view(np.uint64), np.asarray(b["weight"], np.float64).view(np.uint64))


def digest(flat, stats):
    """a vocabulary and the integer statistics the definition shares with the device, as one comparable value"""
    import hashlib
    h = hashlib.sha256()
    for key in ("parent", "is_leaf", "descriptor", "weight"):
        h.update(np.ascontiguousarray(flat[key]).tobytes())
    return [flat["k"], flat["L"], len(flat["parent"]), h.hexdigest()] + [int(stats[f]) for f in V.STAT_FIELDS] + [int(x) for x in stats["level_nodes"]] + \
        [int(x) for x in stats["level_max_iterations"]]


if __name__ == "__main__":
    # a fresh process per value of CORB_VOC_TRAIN_SMALL (the library reads it at load): trains the named cases and prints their digests and kernel families as JSON
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import corbload
    corb = corbload.load_pkg()
    out = {}
    for name in sys.argv[1:]:
        sets, k, L, seed, max_it = inputs(name)
        v = corb.Vocabulary.train(sets, k, L, seed, max_it)
        st = v.train_stats
        out[name] = dict(digest=digest(v.flat(), st), small=sum(st["level_small_nodes"]), large=sum(st["level_large_nodes"]), small_limit=st["small_limit"])
        v.close()
    print(json.dumps(out))

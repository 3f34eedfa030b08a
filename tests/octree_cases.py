"""Images for the quadtree tests (tests/test_octree_reference.py on the CPU, tests/test_gpu_octree_kinds.py on the GPU) and their classification by the
oracle: per level the oracle's candidates go through tests/octree_reference.py, which reports the branches the level takes.

name: (image builder, nfeatures, levels); scale 1.2, thresholds 20 / 7 everywhere."""
import numpy as np

import octree_reference as OR

INI_TH, MIN_TH, SCALE = 20, 7, 1.2


def _noise(w, h, seed, values=None):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w), dtype=np.uint8) if values is None else rng.choice(np.array(values, np.uint8), (h, w))


def noise_403():
    """Uniform byte noise: more than 8192 candidates on level 0 and 4097 .. 8192 on level 1 (asserted by the tests)."""
    return _noise(403, 263, 5)


def near_square():
    """W / H of the detection area rounds to 1: a single initial node."""
    return _noise(140, 130, 6, [0, 64, 128, 192, 255])


def wide_strip():
    """A 74-px-high strip with 9 initial nodes on level 0; the column band of initial node 3 is flat (with 6 px to spare, so that no ring of a pixel
    inside the band reaches the noise): that node starts empty and is erased."""
    img = _noise(400, 74, 7, [0, 64, 128, 192, 255])
    hX = np.float32(400 - 32) / np.float32(9)
    img[:, 16 + int(hX * np.float32(3)) - 6:16 + int(hX * np.float32(4)) + 6] = 128
    return img


# Sparse images, 200 x 130 on 3 levels, flat 128.  What a feature gives on each level is the oracle's to say (the tests assert the counts): an isolated pixel
# 8 grey levels up is a corner at the second threshold on level 0 and is gone after one resize; a flat 2 x 2 or 3 x 3 block is NO corner on level 0 (its
# pixels score alike and the non-maximum suppression is strict), but has a single peak after one / two resizes.
_DOTS = [(40, 30), (80, 30), (120, 30), (160, 30), (40, 65), (100, 65), (160, 65)]
_BLOBS3 = [(60, 97), (102, 97), (144, 97)]


def _sparse(single):
    img = np.full((130, 200), 128, np.uint8)
    for x, y in _DOTS:
        img[y, x] = 136
    for x, y in _BLOBS3:
        img[y:y + 3, x:x + 3] = 180
    if single:
        img[48:50, 58:60] = 136
    return img


def sparse_gap():
    """Levels 0 and 2 hold a few keys (fewer than their quota), level 1 none."""
    return _sparse(False)


def sparse_one():
    """As sparse_gap, and level 1 holds exactly one key."""
    return _sparse(True)


def binary_noise():
    """{0, 255} noise: responses pile up on a few values and the nodes hold small, often equal, numbers of keys."""
    return _noise(200, 130, BINARY_SEED, [0, 255])


BINARY_SEED = 0
CASES = {
    "noise_403": (noise_403, 900, 2),
    "near_square": (near_square, 990, 2),             # two phase-B iterations on level 0
    "wide_strip": (wide_strip, 400, 2),
    "sparse_gap": (sparse_gap, 300, 3),
    "sparse_one": (sparse_one, 300, 3),
    "binary_noise": (binary_noise, 350, 2),           # ties at the stop point of phase B on both levels, two iterations on level 0
    "binary_stall": (binary_noise, 400, 2),           # level 0: phase B runs out of candidates below the quota
    "binary_tiny": (binary_noise, 5, 2),              # quotas 3 and 2: the first pass reaches them
}
_cache = {}


class Classified:
    """A case run through the oracle: image, final keypoints / descriptors, and per level the candidates, the quota, the kinds and the kept keys."""
    def __init__(self, pyorc, name):
        build, self.nfeatures, self.nlevels = CASES[name]
        self.name, self.img = name, build()
        self.ref = pyorc.Extractor(self.nfeatures, SCALE, self.nlevels, INI_TH, MIN_TH)
        self.kps, self.desc = self.ref.extract(self.img)
        self.quota = self.ref.tables()["quota"]
        self.sizes = [self.ref.level(l).shape[::-1] for l in range(self.nlevels)]
        self.cands = [self.ref.candidates(l) for l in range(self.nlevels)]
        self.counts = [self.ref.level_count(l) for l in range(self.nlevels)]
        self.kinds, self.sel = [], []
        for l in range(self.nlevels):
            sel, k = OR.distribute_level(self.cands[l], self.sizes[l][0], self.sizes[l][1], int(self.quota[l]))
            self.kinds.append(k); self.sel.append(sel)


def classified(pyorc, name):
    if name not in _cache:
        _cache[name] = Classified(pyorc, name)
    return _cache[name]


def kinds_table(pyorc):
    """One line per (case, level) and the totals over all cases."""
    lines, total = [], {}
    for name in CASES:
        c = classified(pyorc, name)
        for l, k in enumerate(c.kinds):
            OR.add_kinds(total, k)
            lines.append("%-13s L%d %3d x %-3d N %3d  " % (name, l, c.sizes[l][0], c.sizes[l][1], c.quota[l]) + " ".join("%s=%d" % (kd, k[kd]) for kd in OR.KIND_NAMES if k[kd]))
    return lines, total

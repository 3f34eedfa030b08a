"""The definition of vocabulary training for this project: DBoW2's TemplatedVocabulary::create(training_features, k, L) for TF_IDF / L1_NORM, restated literally and
recursively (depth first, as the source runs) in plain Python from the reference tree (C = corbslam_client):
    create            C/Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:558-587
    HKmeansStep       :642-819          initiateClustersKMpp  :833-913
    createWords       :918-938          setNodeWeights        :943-996
    FORB::meanValue   FORB.cpp:28-77    saveToTextFile        :1429-1449
Everything the product computes (csrc/voctrain_math.h level by level on the host, csrc/voctrain_kernels.hip on the device) is held bit-equal to this file.

Readings chosen where the source leaves a choice (DESIGN.md section 2 repeats them):
  * random numbers: the source draws from rand() in depth-first order after a time seed.  Here every k-means node has its own draws.  A node is named by its path:
    key(root) = 0 and the c-th child (0-based) of a node at depth d has key = key(parent) + (c + 1) * 21**d.  Draw j of node `key` is
    r = mix(seed + 0x9E3779B97F4A7C15 * (key * 256 + j + 1)) >> 33 (mod 2^64; mix is the splitmix64 finaliser), so r is in [0, 2^31 - 1] like glibc's rand().
    Draw 0 gives RandomInt(0, n - 1) = int((r / 2147483648.0) * n); each later draw gives cut_d = (r / 2147483647.0) * dist_sum, redrawn while cut_d == 0.0 (:887-891);
  * selection (:893-903): the first index whose running sum of min_dists is >= cut_d, the last index if none is; the sums are integers below 2^53;
  * dist_sum == 0 (:908): the node keeps fewer than k centres (a "short" node);
  * an empty cluster in a later iteration: the source releases the centre and then reads a null pointer; here the centre stays as it was and the event is counted;
  * the source has no iteration bound; here max_iterations >= 1 is an argument.  One iteration is one pass of step 2 of the while(goon) loop (:721-751), counting the
    first.  A pass after the first that changes no association ends the node; a node whose pass number max_iterations has not ended it keeps its last centres and groups
    and is counted as capped (so with max_iterations = 1 every k-means node is capped);
  * node ids are the source's: a node's clusters get consecutive ids when it finishes, then the recursion goes child by child (:786-818); word ids are the leaves in id order;
  * weights (:962-992): Ni counts the training images with at least one feature whose transform descent (dbow_reference.Vocabulary.descend on the finished tree, not the
    training assignment) ends in the word; weight = math.log(NDocs / Ni), 0.0 where Ni == 0; NDocs counts empty images too;
  * meanValue sets a bit iff sum >= n // 2 + n % 2, MSB first per byte; a single member is copied; assignment uses strict `<`, the first minimum wins (:734-745);
  * refused: k < 2 (the source divides by k - 1), k > 20, L < 1, L > 10, max_iterations < 1, no feature at all.
"""
import math
import numpy as np

import dbow_reference as R

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MAX_LEVELS = 10
STAT_FIELDS = ("nodes", "words", "kmeans_nodes", "trivial_nodes", "short_nodes", "max_iterations_seen", "capped_nodes", "empty_cluster_events")


def mix(z):
    """the splitmix64 finaliser"""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, key, j):
    return mix(seed + GOLDEN * (key * 256 + j + 1)) >> 33


def child_key(key, depth, c):
    return key + (c + 1) * 21 ** depth


def mean_value(members, stats=None):
    """FORB::meanValue on an [n, 32] uint8 array, n >= 1"""
    n = len(members)
    if n == 1:
        return members[0].copy()
    sums = np.unpackbits(members, axis=1).astype(np.int64).sum(axis=0)          # bit j*8 + b is bit (7 - b) of byte j: MSB first, as unpackbits
    n2 = n // 2 + n % 2
    if stats is not None and n % 2 == 0:
        stats["tie_bits"] += int((sums == n2).sum())
    return np.packbits((sums >= n2).astype(np.uint8))


def _distances(desc, centre):
    return R._POP[np.bitwise_xor(desc, centre[None, :])].sum(axis=1).astype(np.int64)


def seed_centres(desc, k, seed, key):
    """initiateClustersKMpp: the indices of the chosen features"""
    n = len(desc)
    j = 0
    first = int((draw(seed, key, j) / 2147483648.0) * n); j += 1
    chosen = [first]
    min_d = _distances(desc, desc[first])
    while len(chosen) < k:
        min_d = np.minimum(min_d, _distances(desc, desc[chosen[-1]]))
        dist_sum = int(min_d.sum())
        if dist_sum <= 0:
            break
        while True:
            cut_d = (draw(seed, key, j) / 2147483647.0) * float(dist_sum); j += 1
            if cut_d != 0.0:
                break
        up = 0; pick = n - 1
        for i in range(n):
            up += int(min_d[i])
            if float(up) >= cut_d:
                pick = i
                break
        chosen.append(pick)
    return chosen


def assign(desc, centres):
    best = _distances(desc, centres[0]); which = np.zeros(len(desc), np.int64)
    for c in range(1, len(centres)):
        d = _distances(desc, centres[c])
        better = d < best                                                       # strict: the first minimum wins
        best = np.where(better, d, best); which = np.where(better, c, which)
    return which


class _Trainer:
    def __init__(self, desc, k, L, seed, max_iterations):
        self.desc, self.k, self.L, self.seed, self.max_it = desc, k, L, seed, max_iterations
        self.parent, self.descriptor = [], []           # nodes 1 .. n
        self.members, self.settled = [], []             # per node: the features of its final group; whether its k-means node ended by itself (or was trivial)
        self.has_children = [False]                     # node 0 .. n
        self.stats = dict((f, 0) for f in STAT_FIELDS); self.stats["tie_bits"] = 0
        self.level_nodes = [0] * MAX_LEVELS; self.level_max_iterations = [0] * MAX_LEVELS

    def step(self, parent_id, idx, level, key):
        """HKmeansStep(parent_id, descriptors, current_level); idx are feature indices in original relative order"""
        if len(idx) == 0:
            return
        d = self.desc[idx]; k = self.k; st = self.stats; capped = False
        self.level_nodes[level - 1] += 1
        if len(idx) <= k:                                                       # :660 trivial: one cluster per feature
            st["trivial_nodes"] += 1
            centres = [d[i].copy() for i in range(len(idx))]; which = np.arange(len(idx))
        else:
            st["kmeans_nodes"] += 1
            centres = [d[i].copy() for i in seed_centres(d, k, self.seed, key)]
            if len(centres) < k:
                st["short_nodes"] += 1
            it = 0; last = None
            while True:
                it += 1
                if it > 1:
                    for c in range(len(centres)):
                        members = d[last == c]
                        if len(members) == 0:
                            st["empty_cluster_events"] += 1                     # chosen reading: the centre stays
                        else:
                            centres[c] = mean_value(members, st)
                which = assign(d, np.array(centres))
                if it > 1 and np.array_equal(which, last):
                    break
                if it == self.max_it:
                    st["capped_nodes"] += 1; capped = True
                    break
                last = which
            st["max_iterations_seen"] = max(st["max_iterations_seen"], it)
            self.level_max_iterations[level - 1] = max(self.level_max_iterations[level - 1], it)
        ids = []
        for ci, c in enumerate(centres):                                        # :786-793
            self.parent.append(parent_id); self.descriptor.append(c); self.has_children.append(False)
            self.members.append(idx[which == ci]); self.settled.append(not capped)
            ids.append(len(self.parent))
        self.has_children[parent_id] = True
        if level < self.L:                                                      # :796-818
            depth = level - 1
            for c, nid in enumerate(ids):
                members = idx[which == c]
                if len(members) > 1:
                    self.step(nid, members, level + 1, child_key(key, depth, c))


def check_arguments(k, L, max_iterations, n_features):
    if k < 2 or k > R.MAX_K:
        raise ValueError("k must be in [2, 20]")
    if L < 1 or L > R.MAX_L:
        raise ValueError("L must be in [1, 10]")
    if max_iterations < 1:
        raise ValueError("max_iterations must be at least 1")
    if n_features < 1:
        raise ValueError("no training feature")


def create(sets, k, L, seed, max_iterations=100, detail=False):
    """-> (flat, stats[, members, settled]): flat as dbow_reference.Vocabulary.flat(); stats: STAT_FIELDS as ints, level_nodes / level_max_iterations as lists of 10, and (definition only) tie_bits"""
    sets = [np.ascontiguousarray(s, np.uint8).reshape(-1, 32) for s in sets]
    desc = np.concatenate(sets) if sets else np.zeros((0, 32), np.uint8)
    check_arguments(k, L, max_iterations, len(desc))
    t = _Trainer(desc, int(k), int(L), int(seed) & M64, int(max_iterations))
    t.step(0, np.arange(len(desc)), 1, 0)
    n = len(t.parent)
    is_leaf = np.array([0 if t.has_children[i] else 1 for i in range(1, n + 1)], np.int32)
    flat = dict(k=int(k), L=int(L), scoring=0, weighting=0, parent=np.array(t.parent, np.int32), is_leaf=is_leaf, descriptor=np.array(t.descriptor, np.uint8).reshape(-1, 32),
                weight=np.zeros(n, np.float64))
    v = R.Vocabulary(**flat)
    ni = np.zeros(v.n_words, np.int64)
    for s in sets:                                                              # :968-983
        for w in set(v.descend(f, 0)[0] for f in s):
            ni[w] += 1
    for w in range(v.n_words):
        if ni[w] > 0:
            flat["weight"][v.words[w] - 1] = math.log(len(sets) / int(ni[w]))   # :990
    t.stats["nodes"] = n + 1; t.stats["words"] = v.n_words
    t.stats["level_nodes"] = t.level_nodes; t.stats["level_max_iterations"] = t.level_max_iterations
    return (flat, t.stats, t.members, t.settled) if detail else (flat, t.stats)


def save_text(flat, digits=0):
    """saveToTextFile (:1429-1449): header `k L  0 0`, a space after every descriptor byte and one more before the weight; weights as the stream default (%g), or %.17g"""
    fmt = "%g" if digits == 0 else "%%.%dg" % digits
    out = ["%d %d  0 0" % (flat["k"], flat["L"])]
    for p, lf, d, w in zip(flat["parent"], flat["is_leaf"], flat["descriptor"], flat["weight"]):
        out.append("%d %d %s  %s" % (p, 1 if lf else 0, " ".join(str(int(b)) for b in d), fmt % float(w)))
    return "\n".join(out) + "\n"

"""The definition of place recognition for this project: DBoW2's vocabulary transform, BowVector / FeatureVector, L1 score and the KeyFrameDatabase, restated
literally in numpy / plain Python from the reference tree (C = corbslam_client):
    transform        C/Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194 and :1218-1259
    BowVector        BowVector.cpp:34-84 (addWeight, normalize)        FeatureVector.cpp:31 (addFeature)
    L1 score         ScoringObject.cpp:23-68
    text loader      TemplatedVocabulary.h:1338-1424
    database         C/src/KeyFrameDatabase.cc:38-401                  minScore loop: C/src/LoopClosing.cc:122-137
Everything the product computes (csrc/bow_math.h on the host, csrc/bow_kernels.hip on the device) is held bit-equal to this file.

Readings chosen where the source leaves a choice (DESIGN.md section 2 repeats them):
  * only scoring 0 (L1_NORM) with weighting 0 (TF_IDF) exists; anything else is a ValueError;
  * blank trailing lines of a text vocabulary are skipped (the source's `while(!f.eof())` would make a garbage node of one);
  * a leaf reached at a smaller depth than L - levelsup: the source returns an uninitialised `nid`; here the leaf itself is recorded;
  * mLoopScore is missing from KeyFrame's initialiser list; here it starts at 0 like the other five fields.
"""
import numpy as np

MAX_K = 20          # the loader's bound (:1359)
MAX_L = 10
N_NEIGHBOURS = 10   # GetBestCovisibilityKeyFrames(10)

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    """DescriptorDistance of two 32-byte descriptors"""
    return int(_POP[np.bitwise_xor(a, b)].sum())


class Vocabulary:
    """Flat form: node ids 1 .. n in `parent` / `is_leaf` / `descriptor` / `weight` order (node 0 is the root), children in id order, word ids in id order of the leaves."""

    def __init__(self, k, L, scoring, weighting, parent, is_leaf, descriptor, weight):
        parent = np.asarray(parent, np.int64).reshape(-1); is_leaf = np.asarray(is_leaf, np.int64).reshape(-1)
        descriptor = np.ascontiguousarray(descriptor, np.uint8).reshape(-1, 32); weight = np.asarray(weight, np.float64).reshape(-1)
        n = len(parent)
        if not (len(is_leaf) == len(descriptor) == len(weight) == n):
            raise ValueError("vocabulary arrays differ in length")
        if k < 0 or k > MAX_K or L < 1 or L > MAX_L:                      # :1359
            raise ValueError("k or L outside the loader's bounds")
        if scoring != 0 or weighting != 0:
            raise ValueError("only L1_NORM scoring with TF_IDF weighting is supported")
        if n < 1:
            raise ValueError("empty vocabulary")
        self.k, self.L, self.n_nodes = int(k), int(L), n + 1
        self.parent = np.concatenate([[0], parent]); self.descriptor = np.concatenate([np.zeros((1, 32), np.uint8), descriptor])
        self.children = [[] for _ in range(n + 1)]
        self.word_id = np.full(n + 1, -1, np.int64); self.node_weight = np.concatenate([[0.0], weight])
        words = []
        for nid in range(1, n + 1):
            pid = int(self.parent[nid])
            if pid < 0 or pid >= nid:
                raise ValueError("node %d: parent %d is not before it" % (nid, pid))
            if self.word_id[pid] >= 0:
                raise ValueError("node %d: its parent %d is a leaf" % (nid, pid))
            self.children[pid].append(nid)                                # :1392
            if len(self.children[pid]) > self.k:
                raise ValueError("node %d has more than k children" % pid)
            if is_leaf[nid - 1] > 0:                                      # :1408-1415
                self.word_id[nid] = len(words); words.append(nid)
        for nid in range(1, n + 1):
            if self.word_id[nid] < 0 and not self.children[nid]:
                raise ValueError("node %d is neither a leaf nor a parent" % nid)
        self.words = np.array(words, np.int64)                           # word id -> node id
        self.n_words = len(words)
        self.is_leaf = (self.word_id[1:] >= 0).astype(np.int32)

    def flat(self):
        return dict(k=self.k, L=self.L, scoring=0, weighting=0, parent=self.parent[1:].astype(np.int32), is_leaf=self.is_leaf.copy(),
                    descriptor=self.descriptor[1:].copy(), weight=self.node_weight[1:].copy())

    # ---- text format of loadFromTextFile / saveToTextFile ----
    def to_text(self):
        out = ["%d %d 0 0" % (self.k, self.L)]
        for nid in range(1, self.n_nodes):
            out.append("%d %d %s %s" % (self.parent[nid], 1 if self.word_id[nid] >= 0 else 0, " ".join(str(int(b)) for b in self.descriptor[nid]), repr(float(self.node_weight[nid]))))
        return "\n".join(out) + "\n"

    @classmethod
    def from_text(cls, text):
        lines = text.split("\n")
        head = lines[0].split()
        if len(head) < 4:
            raise ValueError("not a vocabulary text file")
        k, L, n1, n2 = (int(v) for v in head[:4])
        parent, leaf, desc, weight = [], [], [], []
        for ln in lines[1:]:
            t = ln.split()
            if not t:                                                     # chosen reading: blank lines make no node
                continue
            if len(t) != 35:
                raise ValueError("a node line has %d fields, not 35" % len(t))
            parent.append(int(t[0])); leaf.append(int(t[1])); desc.append([int(v) for v in t[2:34]]); weight.append(float(t[34]))
        return cls(k, L, n1, n2, parent, leaf, np.array(desc, np.uint8).reshape(-1, 32), weight)

    # ---- transform of one feature (:1218-1259) ----
    def descend(self, d, levelsup):
        nid_level = self.L - levelsup
        nid = 0 if nid_level <= 0 else None
        final, level = 0, 0
        while True:
            level += 1
            nodes = self.children[final]
            final = nodes[0]
            best = hamming(d, self.descriptor[final])
            for c in nodes[1:]:
                dist = hamming(d, self.descriptor[c])
                if dist < best:                                           # strict: the first minimum wins
                    best, final = dist, c
            if level == nid_level:
                nid = final
            if not self.children[final]:
                break
        if nid is None:                                                   # chosen reading: a leaf above the recording level is recorded itself
            nid = final
        return int(self.word_id[final]), float(self.node_weight[final]), int(nid)

    # ---- transform of a feature set (:1127-1194 with BowVector.cpp:34-84) ----
    def transform(self, desc, levelsup, per_feature=False):
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        bow, fv = {}, {}
        fw = np.zeros(len(desc), np.int32); fn = np.zeros(len(desc), np.uint32)
        for i, d in enumerate(desc):
            wid, w, nid = self.descend(d, levelsup)
            fw[i], fn[i] = wid, nid
            if w > 0:                                                     # :1157 not stopped
                if wid in bow:
                    bow[wid] = bow[wid] + np.float64(w)                   # addWeight: one addition per feature, in feature order
                else:
                    bow[wid] = np.float64(w)
                fv.setdefault(nid, []).append(i)
        word = np.array(sorted(bow), np.uint32)
        value = np.array([bow[int(w)] for w in word], np.float64)
        norm = np.float64(0.0)
        for v in value:                                                   # BowVector::normalize(L1): ascending word order
            norm = norm + np.abs(v)
        if norm > 0.0:
            value = value / norm
        nodes = np.array(sorted(fv), np.uint32)
        off = np.zeros(len(nodes) + 1, np.int32); idx = []
        for j, n in enumerate(nodes):
            idx += fv[int(n)]; off[j + 1] = len(idx)
        out = (word, value, nodes, off, np.array(idx, np.uint32))
        return out + (fw, fn) if per_feature else out


def score(a, b):
    """L1Scoring::score on two (word[], value[]) BowVectors"""
    wa, va = a; wb, vb = b
    i = j = 0
    s = np.float64(0.0)
    while i < len(wa) and j < len(wb):
        if wa[i] == wb[j]:
            vi, wi = np.float64(va[i]), np.float64(vb[j])
            s = s + (np.abs(vi - wi) - np.abs(vi) - np.abs(wi))
            i += 1; j += 1
        elif wa[i] < wb[j]:
            i = int(np.searchsorted(wa, wb[j], "left"))                   # lower_bound
        else:
            j = int(np.searchsorted(wb, wa[i], "left"))
    return np.float64(-s / np.float64(2.0))


class KeyFrame:
    """What KeyFrameDatabase.cc reads and writes of a KeyFrame (or a Frame: mnId and mBowVec)"""

    def __init__(self, mnId, bow, name=None):
        self.mnId = int(mnId); self.bow = (np.asarray(bow[0], np.uint32), np.asarray(bow[1], np.float64)); self.name = name
        self.mnLoopQuery = 0; self.mnLoopWords = 0; self.mLoopScore = np.float32(0)
        self.mnRelocQuery = 0; self.mnRelocWords = 0; self.mRelocScore = np.float32(0)
        self.neighbours = []                                              # GetBestCovisibilityKeyFrames(10)
        self.connected = set()                                            # GetConnectedKeyFrames()

    def state(self):
        return (self.mnLoopQuery, self.mnLoopWords, np.float32(self.mLoopScore), self.mnRelocQuery, self.mnRelocWords, np.float32(self.mRelocScore))


class KeyFrameDatabase:
    def __init__(self, n_words):
        self.n_words = n_words
        self.inv = [[] for _ in range(n_words)]                           # mvInvertedFile

    def add(self, kf):                                                    # :38-46
        for w in kf.bow[0]:
            self.inv[int(w)].append(kf)

    def erase(self, kf):                                                  # :48-65
        for w in kf.bow[0]:
            lst = self.inv[int(w)]
            for p, o in enumerate(lst):
                if o is kf:
                    del lst[p]
                    break

    def clear(self):                                                      # :67-70
        self.inv = [[] for _ in range(self.n_words)]

    def DetectLoopCandidates(self, kf, minScore):                         # :73-187
        minScore = np.float32(minScore)
        connected = kf.connected
        sharing = []
        for w in kf.bow[0]:
            for o in self.inv[int(w)]:
                if o.mnLoopQuery != kf.mnId:
                    o.mnLoopWords = 0
                    if o not in connected:
                        o.mnLoopQuery = kf.mnId
                        sharing.append(o)
                o.mnLoopWords += 1
        if not sharing:
            return []
        maxCommon = 0
        for o in sharing:
            if o.mnLoopWords > maxCommon:
                maxCommon = o.mnLoopWords
        minCommon = int(np.float32(maxCommon) * np.float32(0.8))
        scored = []
        for o in sharing:
            if o.mnLoopWords > minCommon:
                si = np.float32(score(kf.bow, o.bow))
                o.mLoopScore = si
                if si >= minScore:
                    scored.append((si, o))
        if not scored:
            return []
        acc = []
        bestAcc = minScore
        for si, o in scored:
            bestScore = si; accScore = si; best = o
            for o2 in o.neighbours:
                if o2.mnLoopQuery == kf.mnId and o2.mnLoopWords > minCommon:
                    accScore = np.float32(accScore + o2.mLoopScore)
                    if o2.mLoopScore > bestScore:
                        best = o2; bestScore = o2.mLoopScore
            acc.append((accScore, best))
            if accScore > bestAcc:
                bestAcc = accScore
        return self._retain(acc, bestAcc)

    @staticmethod
    def _retain(acc, bestAcc):
        minRetain = np.float32(np.float32(0.75) * bestAcc)
        out = []
        for a, o in acc:
            if a > minRetain and not any(o is p for p in out):
                out.append(o)
        return out

    def _reloc(self, q):                                                  # :189-295 and :297-401: the same text twice
        sharing = []
        for w in q.bow[0]:
            for o in self.inv[int(w)]:
                if o.mnRelocQuery != q.mnId:
                    o.mnRelocWords = 0
                    o.mnRelocQuery = q.mnId
                    sharing.append(o)
                o.mnRelocWords += 1
        if not sharing:
            return []
        maxCommon = 0
        for o in sharing:
            if o.mnRelocWords > maxCommon:
                maxCommon = o.mnRelocWords
        minCommon = int(np.float32(maxCommon) * np.float32(0.8))
        scored = []
        for o in sharing:
            if o.mnRelocWords > minCommon:
                si = np.float32(score(q.bow, o.bow))
                o.mRelocScore = si
                scored.append((si, o))
        if not scored:
            return []
        acc = []
        bestAcc = np.float32(0)
        for si, o in scored:
            bestScore = si; accScore = si; best = o
            for o2 in o.neighbours:
                if o2.mnRelocQuery != q.mnId:
                    continue
                accScore = np.float32(accScore + o2.mRelocScore)          # (a neighbour that was not scored for this query adds its stale score)
                if o2.mRelocScore > bestScore:
                    best = o2; bestScore = o2.mRelocScore
            acc.append((accScore, best))
            if accScore > bestAcc:
                bestAcc = accScore
        return self._retain(acc, bestAcc)

    def DetectRelocalizationCandidates(self, frame):
        return self._reloc(frame)

    def DetectMapFusionCandidatesFromDB(self, kf):
        return self._reloc(kf)


def min_score(db_unused, kf, connected_in_order):
    """the minScore loop of LoopClosing::DetectLoop (C/src/LoopClosing.cc:122-137): the scores of the connected keyframes, for the caller's minimum"""
    return np.array([score(kf.bow, o.bow) for o in connected_in_order], np.float64)

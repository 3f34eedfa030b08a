"""Definition, in plain Python, of what the calls of include/corb_loop_detect.h compute: LoopClosing::DetectLoop (corbslam_client/src/LoopClosing.cc:100-231, cited as
:NN below) with the state LoopClosing keeps between calls, under the reference's member names.  It is built from the two definitions the device routes it chains are
already compared with: tests/dbow_reference.py (KeyFrameDatabase.DetectLoopCandidates, score, min_score) and tests/covis_reference.py (get_vector_covisibles and the
weight map of a keyframe).

A keyframe is named by its mnId.  `m` is a covis_reference.Map (m.kfs: the keyframes the cache holds, with .weights, .ordered and .bad); `bow` maps an id to its
dbow_reference.KeyFrame (mnId, BowVector, the six query fields, .neighbours) or has no entry for it: that keyframe has no BowVector the database could know."""
import numpy as np

import covis_reference as CR
import dbow_reference as DR

GAP, NONE, NOT_ENOUGH, DETECTED = 0, 1, 2, 3


class Unbound(Exception):
    """a covisible keyframe without a BowVector: the reference would read a vector that does not exist; the device route answers CORB_ERR_ARG with nothing changed"""


class Capacity(Exception):
    """more candidates or more new groups than the device object has room for: the keyframe is not processed"""


class LoopClosing:
    def __init__(self, m, db, bow, max_candidates=None, max_groups=None):
        self.m = m; self.mpKeyFrameDB = db; self.bow = bow
        self.mLastLoopKFid = 0                                       # :41
        self.mnCovisibilityConsistencyTh = 3                         # :42
        self.mvConsistentGroups = []                                 # [(set of ids, counter)]
        self.mvpEnoughConsistentCandidates = []
        self.mlpLoopKeyFrameQueue = []
        self.mpCurrentKF = None
        self.live = set()                                            # ids added to the database, for the tests
        self.max_candidates = max_candidates; self.max_groups = max_groups

    def InsertKeyFrame(self, kid):                                   # :87-92
        if kid != 0:
            self.mlpLoopKeyFrameQueue.append(kid)

    def CheckNewKeyFrames(self):                                     # :94-98
        return bool(self.mlpLoopKeyFrameQueue)

    def RequestReset(self):                                          # :647 -- the queue clears, mLastLoopKFid = 0, the groups stay
        self.mlpLoopKeyFrameQueue = []; self.mLastLoopKFid = 0

    def drop(self, kid):
        """corb_loop_detector_drop_slot: a keyframe that left the map can never match again"""
        for s, _ in self.mvConsistentGroups:
            s.discard(kid)

    def _add(self, kid):                                             # mpKeyFrameDB->add(mpCurrentKF) (:113, :147, :217)
        self.mpKeyFrameDB.add(self.bow[kid]); self.live.add(kid)

    def connected(self, kid):
        """KeyFrame::GetConnectedKeyFrames (KeyFrame.cc:188-197): the whole weight map, the keyframes the cache holds"""
        return set(i for i in self.m.kfs[kid].weights if i in self.m.kfs)

    def min_score(self, kid):
        """:122-137 -> np.float32"""
        cov = [i for i in CR.get_vector_covisibles(self.m, kid) if not self.m.kfs[i].bad]          # :122, :128
        if any(i not in self.bow for i in cov):
            raise Unbound(kid)
        minScore = np.float32(1)                                     # :124
        for s in DR.min_score(self.mpKeyFrameDB, self.bow[kid], [self.bow[i] for i in cov]):
            s = np.float32(s)                                        # :133 `float score = ...`
            if s < minScore:                                         # :135
                minScore = s
        return minScore

    def DetectLoop(self, kid=None):
        """one keyframe: dict(outcome, minScore (np.float32 or None), candidates (ids), enough (positions in candidates), groups)"""
        if kid is None:
            kid = self.mlpLoopKeyFrameQueue.pop(0)                   # :104-105
        self.mpCurrentKF = kid
        if kid < self.mLastLoopKFid + 10:                            # :111
            self._add(kid)                                           # :114
            return dict(outcome=GAP, minScore=None, candidates=[], enough=[], groups=self.groups())
        minScore = self.min_score(kid)
        q = self.bow[kid]
        q.mnId = kid; q.connected = set(self.bow[i] for i in self.connected(kid) if i in self.bow)
        vpCandidateKFs = [o.name for o in self.mpKeyFrameDB.DetectLoopCandidates(q, minScore)]       # :141
        if self.max_candidates is not None and len(vpCandidateKFs) > self.max_candidates:
            raise Capacity(len(vpCandidateKFs))
        if not vpCandidateKFs:                                       # :144-151
            self._add(kid)
            self.mvConsistentGroups = []
            return dict(outcome=NONE, minScore=minScore, candidates=[], enough=[], groups=[])
        enough = []                                                  # :157 mvpEnoughConsistentCandidates.clear()
        vCurrentConsistentGroups = []
        vbConsistentGroup = [False] * len(self.mvConsistentGroups)   # :160
        for i, cand in enumerate(vpCandidateKFs):                    # :161
            # :165-166; a candidate the cache does not hold has the empty group
            spCandidateGroup = (self.connected(cand) | {cand}) if cand in self.m.kfs else set()
            bEnoughConsistent = False; bConsistentForSomeGroup = False
            for iG, (sPreviousGroup, nPreviousConsistency) in enumerate(self.mvConsistentGroups):     # :170
                if spCandidateGroup & sPreviousGroup:                # :175-183
                    bConsistentForSomeGroup = True
                    nCurrentConsistency = nPreviousConsistency + 1   # :188
                    if not vbConsistentGroup[iG]:                    # :189-194
                        vCurrentConsistentGroups.append((set(spCandidateGroup), nCurrentConsistency))
                        vbConsistentGroup[iG] = True
                    if nCurrentConsistency >= self.mnCovisibilityConsistencyTh and not bEnoughConsistent:      # :195-199
                        enough.append(i); bEnoughConsistent = True
            if not bConsistentForSomeGroup:                          # :204-208
                vCurrentConsistentGroups.append((set(spCandidateGroup), 0))
        if self.max_groups is not None and len(vCurrentConsistentGroups) > self.max_groups:
            raise Capacity(len(vCurrentConsistentGroups))
        self.mvConsistentGroups = vCurrentConsistentGroups           # :212
        self.mvpEnoughConsistentCandidates = [vpCandidateKFs[i] for i in enough]
        self._add(kid)                                               # :217
        return dict(outcome=DETECTED if enough else NOT_ENOUGH, minScore=minScore, candidates=vpCandidateKFs, enough=enough, groups=self.groups())     # :219-227

    def groups(self):
        return [(sorted(s), c) for s, c in self.mvConsistentGroups]

    def DetectLoopQueue(self, kids):
        """corb_loop_detect_queue: the keyframes in order up to and with the first DETECTED (where Run() goes on to ComputeSim3, :70-78)"""
        out = []
        for kid in kids:
            out.append(self.DetectLoop(kid))
            if out[-1]["outcome"] == DETECTED:
                break
        return out


def closed_form(candidate_groups, previous, th=3):
    """The consistency pass (:157-212) as the device evaluates it, without the serial loop: (new groups, enough).  previous = [(set, counter)]."""
    cons = [[bool(c & p) for p, _ in previous] for c in candidate_groups]
    first = [next((i for i in range(len(candidate_groups)) if cons[i][g]), None) for g in range(len(previous))]
    new, enough = [], []
    for i, c in enumerate(candidate_groups):
        new += [(set(c), previous[g][1] + 1) for g in range(len(previous)) if first[g] == i]
        if not any(cons[i]):
            new.append((set(c), 0))
        if any(cons[i][g] and previous[g][1] + 1 >= th for g in range(len(previous))):
            enough.append(i)
    return new, enough

"""The covisibility graph of the reference, restated line by line as the definition the device routes (corb_covis_*) are compared with bit for bit.  Paths are under
corbslam_client/src of the reference.  The reference cannot be compiled for the tests (OpenCV, ROS), so its rules are written out here on plain Python containers:

  Map.kfs        the cache: id -> KeyFrame for the keyframes that are "in the cache" (Cache::KeyFrameInCache, Cache.cc:181-187); any other id is a keyframe the
                 cache does not hold (LightKeyFrame::getKeyFrame() is NULL)
  Map.mps        id -> MapPoint; an id that is not there is a LightMapPoint whose getMapPoint() is NULL
  KeyFrame.weights   mConnectedKeyFrameWeights: dict id -> weight (std::map<LightKeyFrame, int>: walked in ascending id)
  KeyFrame.ordered   mvpOrderedConnectedKeyFrames with mvOrderedWeights: list of (id, weight)
  MapPoint.obs       mObservations: dict keyframe id -> feature index (walked in ascending id)

Map.stats counts the events the seeded generators of tests/covis_cases.py must reach (tests/test_covis_reference.py asserts them)."""
import collections

NO_ID = 0xFFFFFFFFFFFFFFFF
TH_OBS = 3


class KeyFrame:
    def __init__(self, kid, mp_ids, octave=None, depth=None, u_right=None, bad=False):
        n = len(mp_ids)
        self.id = kid; self.mp_ids = list(mp_ids); self.bad = bad
        self.octave = list(octave) if octave is not None else [0] * n
        self.depth = list(depth) if depth is not None else [1.0] * n
        self.u_right = list(u_right) if u_right is not None else [-1.0] * n
        self.weights = {}; self.ordered = []


class MapPoint:
    def __init__(self, pid, obs, bad=False):
        self.id = pid; self.obs = dict(obs); self.bad = bad


class Map:
    def __init__(self):
        self.kfs = {}; self.mps = {}; self.stats = collections.Counter()

    def good_point(self, pid):
        """`MapPoint* pMP = ...getMapPoint(); if(!pMP) continue; if(pMP->isBad()) continue;` (KeyFrame.cc:418-424)"""
        if pid is None or pid == NO_ID or pid not in self.mps:
            return None
        if self.mps[pid].bad:
            self.stats["bad_point"] += 1
            return None
        return self.mps[pid]


def descending(pairs):
    """sort(vPairs) ascends in pair<int, LightKeyFrame> -- the weight, then LightKeyFrame::operator< on mnId -- and the lists are filled with push_front
    (KeyFrame.cc:158-164, :475-482): descending (weight, id).  pairs = [(weight, id)]; returns [(id, weight)]."""
    return [(i, w) for w, i in sorted(pairs, reverse=True)]


def update_best_covisibles(kf):
    """KeyFrame::UpdateBestCovisibles (KeyFrame.cc:150-168): the ordered list is rebuilt from the WHOLE weight map -- below the threshold and outside the cache included"""
    kf.ordered = descending([(w, i) for i, w in kf.weights.items()])


def add_connection(m, kf, other_id, weight):
    """KeyFrame::AddConnection (KeyFrame.cc:133-148)"""
    if other_id not in kf.weights:
        kf.weights[other_id] = weight
    elif kf.weights[other_id] != weight:
        kf.weights[other_id] = weight
    else:
        m.stats["early_return"] += 1
        return
    m.stats["resort"] += 1
    update_best_covisibles(kf)


def erase_connection(kf, other_id):
    """KeyFrame::EraseConnection (KeyFrame.cc:685-698)"""
    if other_id in kf.weights:
        del kf.weights[other_id]
        update_best_covisibles(kf)


def update_connections(m, kid, th=15):
    """KeyFrame::UpdateConnections (KeyFrame.cc:404-502).  Returns the front of the ordered list after the update (what mpParent becomes on the first connection of a
    keyframe with mnId != 0, :493-495), or None when the counter was empty or holds no keyframe of the cache."""
    kf = m.kfs[kid]
    counter = {}
    for pid in kf.mp_ids:                                       # :417-435
        mp = m.good_point(pid)
        if mp is None:
            continue
        for oid in sorted(mp.obs):
            if oid == kf.id:
                continue
            counter[oid] = counter.get(oid, 0) + 1
    if not counter:                                             # :438-439
        return None
    nmax, kfmax = 0, None
    pairs = []
    for oid in sorted(counter):                                 # :450-464
        if oid in m.kfs:
            if counter[oid] > nmax:
                nmax, kfmax = counter[oid], oid
            if counter[oid] >= th:
                pairs.append((counter[oid], oid))
                add_connection(m, m.kfs[oid], kf.id, counter[oid])
        else:
            m.stats["unknown"] += 1
    if not pairs:                                               # :466-469
        m.stats["fallback"] += 1
        if kfmax is None:
            # pKFmax is NULL and the reference dereferences it.  The device route defines this case: the weight map is replaced, the ordered list is empty.
            kf.weights = dict(counter); kf.ordered = []
            return None
        pairs.append((nmax, kfmax))
        add_connection(m, m.kfs[kfmax], kf.id, nmax)
    ws = [w for w, _ in pairs]
    if len(set(ws)) < len(ws):
        m.stats["tie"] += 1
    kf.weights = dict(counter)                                  # :489-491
    kf.ordered = descending(pairs)
    return kf.ordered[0][0]


def erase_connections(m, kid):
    """the connection part of KeyFrame::SetBadFlag (KeyFrame.cc:592-595, :604-605)"""
    kf = m.kfs[kid]
    for oid in sorted(kf.weights):
        if oid in m.kfs:
            erase_connection(m.kfs[oid], kf.id)
    kf.weights = {}; kf.ordered = []


def get_vector_covisibles(m, kid):
    """KeyFrame::GetVectorCovisibleKeyFrames (KeyFrame.cc:199-211): ids"""
    return [i for i, _ in m.kfs[kid].ordered if i in m.kfs]


def get_best_covisibles(m, kid, n):
    """KeyFrame::GetBestCovisibilityKeyFrames (KeyFrame.cc:213-230)"""
    v = get_vector_covisibles(m, kid)
    return v if len(v) < n else v[:n]


def get_covisibles_by_weight(m, kid, w):
    """KeyFrame::GetCovisiblesByWeight (KeyFrame.cc:232-260): ids, None for a keyframe the cache does not hold.  upper_bound with weightComp (a > b) is the first weight
    below w; when there is none (`it == mvOrderedWeights.end()`) the reference returns the EMPTY vector."""
    kf = m.kfs[kid]
    out = [i if i in m.kfs else None for i, _ in kf.ordered]
    if not out:
        return []
    n = next((k for k, (_, wk) in enumerate(kf.ordered) if w > wk), None)
    return [] if n is None else out[:n]


def get_weight(m, kid, other_id):
    """KeyFrame::GetWeight (KeyFrame.cc:262-269)"""
    return m.kfs[kid].weights.get(other_id, 0)


def held(m, oid, idx):
    """an observation whose keyframe the cache holds and whose feature index that keyframe has"""
    return oid in m.kfs and idx < len(m.kfs[oid].mp_ids)


def observations(m, mp):
    """MapPoint::Observations() (MapPoint.cc:250-253) = nObs as AddObservation keeps it (:153-158), derived from the list by the rule corb_local_ba_store documents:
    2 for an observation whose keyframe is held and has mvuRight[idx] >= 0, else 1"""
    return sum(2 if held(m, oid, idx) and m.kfs[oid].u_right[idx] >= 0 else 1 for oid, idx in mp.obs.items())


def keyframe_culling(m, cur_id, monocular, th_depth):
    """LocalMapping::KeyFrameCulling (LocalMapping.cc:590-648): [(id, nMPs, nRedundantObservations, cull)] per covisible keyframe; mnId == 0 is skipped (0, 0, False)"""
    out = []
    for kid in get_vector_covisibles(m, cur_id):
        kf = m.kfs[kid]
        if kf.id == 0:                                          # :600-601
            out.append((kid, 0, 0, False))
            continue
        n_red = n_mps = 0
        for i, pid in enumerate(kf.mp_ids):
            mp = m.good_point(pid)
            if mp is None:
                continue
            if not monocular and (kf.depth[i] > th_depth or kf.depth[i] < 0):      # :612-615
                continue
            n_mps += 1
            if observations(m, mp) > TH_OBS:                    # :618
                n_obs = 0
                for oid in sorted(mp.obs):                      # GetObservations(): the keyframes of the cache (MapPoint.cc:219-231)
                    if not held(m, oid, mp.obs[oid]) or oid == kf.id:
                        continue
                    if m.kfs[oid].octave[mp.obs[oid]] <= kf.octave[i] + 1:          # :630
                        n_obs += 1
                        if n_obs >= TH_OBS:
                            break
                if n_obs >= TH_OBS:
                    n_red += 1
        out.append((kid, n_mps, n_red, n_red > 0.9 * n_mps))    # :645
    return out


def local_window(m, kid):
    """the window of Optimizer::LocalBundleAdjustment (Optimizer.cc:493-544): (lLocalKeyFrames, lFixedCameras, lLocalMapPoints) as ids"""
    kf = m.kfs[kid]
    local_mark, fixed_mark = {kf.id}, set()
    l_local = [kf.id]
    for oid in get_vector_covisibles(m, kid):                   # :496-507
        if oid in local_mark:
            continue
        local_mark.add(oid)
        if not m.kfs[oid].bad:
            l_local.append(oid)
    l_points, point_mark = [], set()
    for lid in l_local:                                         # :511-525
        for pid in m.kfs[lid].mp_ids:
            mp = m.good_point(pid)
            if mp is not None and pid not in point_mark:
                l_points.append(pid); point_mark.add(pid)
    l_fixed = []
    for pid in l_points:                                        # :529-544
        for oid in sorted(m.mps[pid].obs):
            if oid not in m.kfs:
                continue
            if oid not in local_mark and oid not in fixed_mark:
                fixed_mark.add(oid)
                if not m.kfs[oid].bad:
                    l_fixed.append(oid)
    return l_local, l_fixed, l_points

"""Tracking::UpdateLocalMap and the spanning tree of the reference, restated line by line on top of tests/covis_reference.py: the definition the device routes
(corb_covis_set_tree .. corb_covis_reparent_children, corb_track_update_local_map) are compared with bit for bit.  Paths are under corbslam_client/src of the reference.

The tree lives on the covis_reference.KeyFrame objects as three more attributes (tree() adds them on first use):
  kf.parent      mpParent: an id or None
  kf.first       mbFirstConnection
  kf.children    mspChildrens: a set of ids (std::set<LightKeyFrame>: walked in ascending id).  It is NOT derived from the parent pointers -- ChangeParent never
                 removes the keyframe from its old parent's set (KeyFrame.cc:516-521)

Readings (stated in include/corb_accel.h and DESIGN.md section 2 as well): keyframeCounter is a map<KeyFrame*,int> and GetChilds() / GetObservations() return
pointer-keyed containers, so the reference's walk order depends on the allocator; here every such walk is in ascending keyframe id, the order LightKeyFrame gives
everywhere else.  Map.stats counts the events the generators of tests/localmap_cases.py must reach (tests/test_localmap_reference.py asserts them)."""
import covis_reference as R

NO_ID = R.NO_ID
MAX_LOCAL = 80          # `if(mvpLocalKeyFrames.size()>80) break;` (Tracking.cc:1313)


def tree(kf):
    if not hasattr(kf, "children"):
        kf.parent = None; kf.first = True; kf.children = set()
    return kf


def set_tree(m, kid, parent, first, children):
    kf = tree(m.kfs[kid]); kf.parent = parent; kf.first = bool(first); kf.children = set(children)


def get_tree(m, kid):
    kf = tree(m.kfs[kid])
    return kf.parent, kf.first, sorted(kf.children)


def add_child(m, kid, child_id):
    """KeyFrame::AddChild (KeyFrame.cc:504-508)"""
    tree(m.kfs[kid]).children.add(child_id)


def erase_child(m, kid, child_id):
    """KeyFrame::EraseChild (KeyFrame.cc:510-514)"""
    tree(m.kfs[kid]).children.discard(child_id)


def change_parent(m, kid, other_id):
    """KeyFrame::ChangeParent (KeyFrame.cc:516-521): the parent is set and the new parent gains the child -- the old parent keeps it"""
    tree(m.kfs[kid]).parent = other_id
    add_child(m, other_id, kid)


def first_connection(m, kid, front):
    """the tail of KeyFrame::UpdateConnections (KeyFrame.cc:493-499) for a keyframe whose ordered list now starts with `front` (None: the list is empty, the
    documented no-held-keyframe reading -- nothing changes)"""
    kf = tree(m.kfs[kid])
    if front is None:
        return
    if kf.first and kf.id != 0:                                 # :493
        kf.parent = front                                       # :494, whether or not the cache holds it
        if front in m.kfs:                                      # :495
            add_child(m, front, kid)                            # :496
            kf.first = False                                    # :497
            m.stats["first_held"] += 1
        else:
            m.stats["first_unheld"] += 1


def update_connections(m, kid, th=15):
    """KeyFrame::UpdateConnections (KeyFrame.cc:404-502) with its tree upkeep; returns what covis_reference.update_connections does (first_parent)"""
    front = R.update_connections(m, kid, th)
    first_connection(m, kid, front)
    return front


def reparent_children(m, kid):
    """the tree part of KeyFrame::SetBadFlag (KeyFrame.cc:607-668), after covis_reference.erase_connections(m, kid).  Returns (ChangeParent calls, whether the
    reference reaches `mbBad = true`)."""
    kf = tree(m.kfs[kid])
    n_changed = 0
    candidates = []                                             # sParentCandidates, the non-NULL ones (:609, :633); matched by mnId (:634)
    if kf.parent is not None and kf.parent in m.kfs:
        candidates.append(kf.parent)
    rounds = 0
    while kf.children:                                          # :613
        best = -1; pc = pp = None
        for cid in sorted(kf.children):                         # :620
            if cid not in m.kfs:                                # :623
                continue
            if m.kfs[cid].bad:                                  # :625
                continue
            for oid in R.get_vector_covisibles(m, cid):         # :629-630
                if oid in candidates:                           # :631-634
                    w = R.get_weight(m, cid, oid)               # :635
                    if w > best:                                # :636: the first best stays
                        pc, pp, best = cid, oid, w
        if pc is None:                                          # :653
            break
        change_parent(m, pc, pp); n_changed += 1               # :649
        candidates.append(pc)                                   # :650
        kf.children.discard(pc)                                 # :651-652
        rounds += 1
    if rounds >= 2:
        m.stats["reparent_two_rounds"] += 1
    sets_bad = False
    if kf.children and kf.parent is not None and kf.parent in m.kfs:      # :658
        for cid in sorted(kf.children):                         # :659
            if cid in m.kfs:                                    # :661 -- a bad child is not skipped here
                change_parent(m, cid, kf.parent); n_changed += 1
        erase_child(m, kf.parent, kid)                          # :665
        sets_bad = True                                         # :667
        m.stats["fallback_parent"] += 1
    m.stats["quirk_sets_bad" if sets_bad else "quirk_not_bad"] += 1
    return n_changed, sets_bad


class Frame:
    """mCurrentFrame: mvpMapPoints as ids (NO_ID = NULL)"""

    def __init__(self, mp_ids):
        self.mp_ids = list(mp_ids)


def voters(m, frame):
    """the counter of Tracking::UpdateLocalKeyFrames (Tracking.cc:1262-1281) without its side effect: {keyframe id: votes}"""
    counter = {}
    for pid in frame.mp_ids:
        if pid == NO_ID or pid not in m.mps or m.mps[pid].bad:
            continue
        for oid in sorted(m.mps[pid].obs):
            if oid in m.kfs:
                counter[oid] = counter.get(oid, 0) + 1
    return counter


def update_local_keyframes(m, frame, prev):
    """Tracking::UpdateLocalKeyFrames (Tracking.cc:1259-1366).  prev = mvpLocalKeyFrames before the call (ids).  Returns dict(kfs = mvpLocalKeyFrames after it,
    n_voted, ref = pKFmax's id or None (mpReferenceKF unchanged), counter_empty, n_cleared); frame.mp_ids loses its bad points (:1278)."""
    counter = {}
    n_cleared = 0
    for i, pid in enumerate(frame.mp_ids):                      # :1263
        if pid == NO_ID or pid not in m.mps:                    # :1265: getMapPoint() is NULL -- the id stays
            if pid != NO_ID:
                m.stats["unresolved_kept"] += 1
            continue
        mp = m.mps[pid]
        if not mp.bad:                                          # :1269
            for oid in sorted(mp.obs):                          # :1271-1274: GetObservations() holds the keyframes of the cache only (MapPoint.cc:219-231)
                if oid in m.kfs:
                    counter[oid] = counter.get(oid, 0) + 1
        else:
            frame.mp_ids[i] = NO_ID                             # :1278
            n_cleared += 1; m.stats["cleared"] += 1
    if not counter:                                             # :1282
        m.stats["counter_empty"] += 1
        return dict(kfs=list(prev), n_voted=0, ref=None, counter_empty=True, n_cleared=n_cleared)
    best, kfmax = 0, None
    local, mark = [], set()
    for oid in sorted(counter):                                 # :1292 (ascending id: the reading)
        if m.kfs[oid].bad:                                      # :1296
            continue
        if counter[oid] > best:                                 # :1299: of equals the smallest id
            best, kfmax = counter[oid], oid
        local.append(oid); mark.add(oid)                        # :1305-1306
    if sum(1 for o in counter if not m.kfs[o].bad and counter[o] == best) >= 2:
        m.stats["vote_tie"] += 1
    if any(m.kfs[o].bad and counter[o] > best for o in counter):
        m.stats["bad_top_voter"] += 1
    n_voted = len(local)
    for k in range(n_voted):                                    # :1310: itEndKF is taken before the pushes
        if len(local) > MAX_LOCAL:                              # :1313
            m.stats["stop_80"] += 1
            break
        kf = tree(m.kfs[local[k]])
        if any(i not in m.kfs for i, _ in kf.ordered[:10]):
            m.stats["neighbour_unheld"] += 1
        for oid in R.get_best_covisibles(m, kf.id, 10):         # :1318-1332
            if not m.kfs[oid].bad and oid not in mark:
                local.append(oid); mark.add(oid)
                break
        seen_earlier = False
        for cid in sorted(kf.children):                         # :1334-1347: GetChilds() drops what the cache does not hold (KeyFrame.cc:523-532)
            if cid not in m.kfs:
                continue
            if not m.kfs[cid].bad and cid not in mark:
                local.append(cid); mark.add(cid)
                m.stats["child_pick"] += 1
                if seen_earlier:
                    m.stats["child_pick_not_first"] += 1
                break
            seen_earlier = True
        if kf.parent is not None and kf.parent in m.kfs:        # :1349-1350: GetParent() is getKeyFrameInCache()
            if kf.parent not in mark:                           # :1352 -- isBad() is not asked
                local.append(kf.parent); mark.add(kf.parent)
                m.stats["parent_break"] += 1
                if k + 1 < n_voted:
                    m.stats["parent_break_before_the_end"] += 1
                break                                           # :1356: leaves the whole walk
    return dict(kfs=local, n_voted=n_voted, ref=kfmax, counter_empty=False, n_cleared=n_cleared)


def update_local_points(m, local_kfs):
    """Tracking::UpdateLocalPoints (Tracking.cc:1230-1256): ids of mvpLocalMapPoints.  pKF->isBad() is not asked."""
    out, mark = [], set()
    for kid in local_kfs:                                       # :1234
        for pid in m.kfs[kid].mp_ids:                           # :1239
            if pid == NO_ID or pid not in m.mps:                # :1243
                continue
            if pid in mark:                                     # :1245
                continue
            if not m.mps[pid].bad:                              # :1247
                out.append(pid); mark.add(pid)
    return out


def update_local_map(m, frame, prev):
    """Tracking::UpdateLocalMap (Tracking.cc:1218-1228): the dict of update_local_keyframes with mps = mvpLocalMapPoints"""
    r = update_local_keyframes(m, frame, prev)
    r["mps"] = update_local_points(m, r["kfs"])
    return r

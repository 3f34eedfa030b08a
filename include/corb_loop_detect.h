/* corb_loop_detect.h -- LoopClosing::DetectLoop on records (corbslam_client/src/LoopClosing.cc:100-231): the head of the loop-closing chain as one call per keyframe,
 * and as one call for a queue of keyframes (exported from libcorb_accel.so beside corb_accel.h).
 *
 * A CorbLoopDetector is created over a covisibility graph (and through it the keyframe store) and a keyframe database.  It holds on the device what LoopClosing
 * holds between calls -- mLastLoopKFid, mnCovisibilityConsistencyTh (3, LoopClosing.cc:42) and mvConsistentGroups -- and the two-way table that says which database
 * entry is the BowVector of which store slot.  A group is a bit set over the slots of the keyframe store, ceil(capacity / 64) 64-bit words, with its counter.
 * The object owns all of its device memory, its page-locked staging and its stream: no call of this header opens a workspace lane.
 * Locks: the detector, the database, the graph, the keyframe store (csrc/record_locks.h; the database before the stores as in corb_map_fusion.h).
 * SetNotErase / SetErase (LoopClosing.cc:107, :115, :149, :221) have no record field: they stay with the caller.
 * No existing struct changes: CORB_ABI_VERSION stays as corb_accel.h states it. */
#ifndef CORB_LOOP_DETECT_H
#define CORB_LOOP_DETECT_H
#include "corb_accel.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct CorbLoopDetector CorbLoopDetector;

#define CORB_LOOP_GAP         0    /* mnId < mLastLoopKFid + 10 (:111): added to the database, the groups untouched */
#define CORB_LOOP_NONE        1    /* no candidate (:144-151): the groups cleared, added */
#define CORB_LOOP_NOT_ENOUGH  2    /* candidates, none of them consistent enough (:219-223): the groups replaced, added */
#define CORB_LOOP_DETECTED    3    /* mvpEnoughConsistentCandidates is not empty (:224-227): the groups replaced, added */
#define CORB_LOOP_DETECT_MAX_QUEUE 64   /* keyframes one corb_loop_detect_queue call takes: the read-back block is sized at creation */

typedef struct CorbLoopDetectResult {   /* one keyframe's DetectLoop, 20 bytes */
    int32_t  outcome;                   /* CORB_LOOP_* */
    uint32_t min_score_bits;            /* minScore (:124-137) as the bits of the float; 0 for CORB_LOOP_GAP, which does not compute it */
    int32_t  n_candidates;              /* vpCandidateKFs.size(); on CORB_ERR_CAPACITY by max_candidates the number found */
    int32_t  n_enough;                  /* mvpEnoughConsistentCandidates.size() */
    int32_t  n_groups;                  /* mvConsistentGroups.size() after the keyframe */
} CorbLoopDetectResult;

/* max_candidates: room for vpCandidateKFs of one keyframe; max_groups: room for mvConsistentGroups.  Both >= 1.  The graph, its stores and the database must
 * outlive the object and live on one device.  A fresh detector has mLastLoopKFid = 0, no group and no slot bound. */
int  corb_loop_detector_create(CorbCovis* g, CorbKfDb* db, int max_candidates, int max_groups, CorbLoopDetector** out);
void corb_loop_detector_destroy(CorbLoopDetector* det);
/* entries[i] of the database is the BowVector of slots[i] of the keyframe store; entries[i] = -1 unbinds the slot.  A slot and an entry have at most one partner: a
 * new pair releases the earlier partners of both.  CORB_ERR_ARG with nothing changed: a slot or an entry out of range, one listed twice. */
int  corb_loop_detector_bind(CorbLoopDetector* det, const int32_t* slots, const int32_t* entries, int n);
/* mLastLoopKFid = id: what CorrectLoop does at LoopClosing.cc:591 */
int  corb_loop_detector_set_last_loop(CorbLoopDetector* det, uint64_t id);
int  corb_loop_detector_get_last_loop(CorbLoopDetector* det, uint64_t* id);
/* LoopClosing::ResetIfRequested (:647): mLastLoopKFid = 0; the groups stay, as in the reference (the queue is the caller's) */
int  corb_loop_detector_reset(CorbLoopDetector* det);
/* mvConsistentGroups.clear() */
int  corb_loop_detector_clear_groups(CorbLoopDetector* det);
/* clears the slot's bit in every stored group.  A caller uses it before it refills the slot with another keyframe: with the reference's pointers a keyframe that
 * left the map can never match again */
int  corb_loop_detector_drop_slot(CorbLoopDetector* det, int slot);
/* mvConsistentGroups in order: counters[g], and the member slots of group g ascending at members[offsets[g] .. offsets[g + 1]).  More groups than cap_groups or more
 * members than cap_members: CORB_ERR_CAPACITY with *n_groups and *n_members set and nothing written */
int  corb_loop_detector_get_groups(CorbLoopDetector* det, int32_t* counters, int32_t* offsets /* cap_groups + 1 */, int32_t* members, int cap_groups, int cap_members,
                                   int* n_groups, int* n_members);

/* DetectLoop for mpCurrentKF = the record in `slot`, all on the device; one synchronisation and one read-back.
 *   :111      mnId from the record header; mnId < mLastLoopKFid + 10: CORB_LOOP_GAP
 *   :122-137  minScore over GetVectorCovisibleKeyFrames() -- the row's ordered list, the ids the store holds, as corb_covis_query(N <= 0, min_weight <= 0) answers it --
 *             without the records that carry CORB_KF_BAD: score() against each one's bound entry by the in-order sum of corb_kfdb_score, rounded to float; the minimum
 *             of those floats from 1.0f
 *   :141      DetectLoopCandidates with that minScore, the connected set being the row's whole weight map (held ids with a bound entry).  Neither visits the host.
 *             The six fields of every entry end as corb_kfdb_detect(kind 0) leaves them; GetBestCovisibilityKeyFrames(10) of the entries is what
 *             corb_kfdb_set_neighbours last set
 *   :157-212  a candidate's group is the held ids of its row's weight map and itself (a candidate whose entry is bound to no slot has the empty group and slot -1).
 *             Consistent(i, iG): the two bit sets share a bit.  The serial loop in closed form: previous group iG gives one new group, that of the first candidate
 *             consistent with it, with counter previous + 1; a candidate consistent with no previous group gives its group with counter 0; the new vector is ordered
 *             by (candidate, iG ascending, the counter-0 entry last); a candidate is enough iff it is consistent with a group whose counter + 1 >= 3
 *   :217      the keyframe's entry is added to the database as corb_kfdb_add adds it
 * res: the outcome and counts.  cand_entries / cand_slots [max_candidates] (optional): vpCandidateKFs as database entries and store slots.  enough [max_candidates]
 * (optional): mvpEnoughConsistentCandidates as positions in the candidate list, ascending.
 * CORB_ERR_ARG with nothing changed: a slot outside the store, empty or without features; a slot without a bound entry, or whose entry has no BowVector or is in the
 * database already; a covisible keyframe (not bad) whose slot has no bound entry with a BowVector.
 * CORB_ERR_CAPACITY: more than max_candidates candidates (res->n_candidates says how many), or more than max_groups new groups (at most previous groups + candidates).
 * The keyframe is then NOT processed: the groups, mLastLoopKFid and the database's live set are as before the call; the six query fields may have moved, as on
 * corb_kfdb_detect's overflow. */
int  corb_loop_detect(CorbLoopDetector* det, int slot, CorbLoopDetectResult* res, int32_t* cand_entries, int32_t* cand_slots, int32_t* enough);
/* DetectLoop for mlpLoopKeyFrameQueue = slots[0 .. n) in order, n <= CORB_LOOP_DETECT_MAX_QUEUE, distinct: what corb_loop_detect gives called for one after the other,
 * stopping after the first keyframe whose outcome is CORB_LOOP_DETECTED -- where the reference goes on to ComputeSim3 / CorrectLoop, which move mLastLoopKFid and the
 * graph.  *n_consumed keyframes were processed; res[k] and row k of the arrays ([n][max_candidates], optional) are theirs.  The decisions between keyframes are taken on
 * the device and the kernels of later keyframes are gated on the stop flag: one synchronisation and one read-back for the whole queue.  The keyframes behind the
 * stopping one are not added to the database and leave no trace, and the database's add sequence ends where the single calls leave it.
 * An error of corb_loop_detect at keyframe k ends the queue there with *n_consumed = k and the earlier keyframes' effects kept; the CORB_ERR_ARG cases the host can
 * see (slots, bindings, BowVectors, a slot listed twice) are checked for the whole queue before anything runs. */
int  corb_loop_detect_queue(CorbLoopDetector* det, const int32_t* slots, int n, CorbLoopDetectResult* res, int32_t* cand_entries, int32_t* cand_slots, int32_t* enough,
                            int* n_consumed);

#ifdef __cplusplus
}
#endif
#endif

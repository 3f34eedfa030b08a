/* corb_trajectory.h -- the camera trajectory on records: the per-frame log of Tracking::Track, KeyFrame::mTcp and mTimeStamp, and the three dumps every main of the
 * reference ends with (exported from libcorb_accel.so beside corb_accel.h).
 *
 * Tracking::Track appends mlRelativeFramePoses, mlpReferences, mlFrameTimes and mlbLost at its end (C/src/Tracking.cc:485-504); KeyFrame::SetBadFlag writes
 * mTcp = Tcw * mpParent->GetPoseInverse() in the `if` that sets mbBad (KeyFrame.cc:666); System::SaveTrajectoryTUM / SaveKeyFrameTrajectoryTUM / SaveTrajectoryKITTI
 * (System.cc:254-403) resolve every logged frame against its reference keyframe as the poses stand at the end -- after local BA, loop correction, the essential
 * graph and the spread of a global BA have moved them -- and walk the spanning tree where that keyframe was culled.  A CorbTrajectory holds the log and the two
 * per-keyframe tables on the device, tied to a CorbCovis graph, which supplies the keyframe store and the parent fields.
 * The object owns all of its device memory and its stream: no call of this header opens a workspace lane.  Locks: the graph, then the keyframe stores by address.
 * Every pose product is cv::gemm on CV_32F as corb_track_frame.h states it (csrc/trackframe_math.h); the quaternion is Eigen::Quaterniond(Matrix3d) on the floats
 * widened to double, each component rounded to float once, not normalised (csrc/traj_math.h).  Every output is reproducible bit for bit.
 * No existing struct changes: CORB_ABI_VERSION stays as corb_accel.h states it. */
#ifndef CORB_TRAJECTORY_H
#define CORB_TRAJECTORY_H
#include <stddef.h>
#include "corb_accel.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct CorbTrajectory CorbTrajectory;

typedef struct CorbTrajEntry {     /* one frame of the log, 88 bytes */
    float    Tcr[16];              /* mlRelativeFramePoses: mCurrentFrame.mTcw * mpReferenceKF->GetPoseInverse() */
    uint64_t ref_id;               /* mlpReferences: the reference keyframe's mnId when the entry was made */
    double   timestamp;            /* mlFrameTimes */
    int32_t  ref_slot;             /* its slot of the graph's keyframe store */
    int32_t  lost;                 /* mlbLost */
} CorbTrajEntry;
typedef struct CorbTrajStats {
    int32_t n_entries;             /* the log's length */
    int32_t n_rows;                /* rows the export gives */
    int32_t n_lost_skipped;        /* TUM: entries with the lost flag (System.cc:283); KITTI: 0 */
    int32_t n_ref_gone;            /* entries whose slot no longer holds their reference's id */
    int32_t n_chain_broken;        /* entries whose walk met a bad keyframe without a held parent, or took more steps than the store has slots */
    int32_t max_chain;             /* the longest walk among the rows, in steps */
} CorbTrajStats;

/* The log has room for capacity_frames entries; the per-slot tables are sized to the graph's keyframe store: Tcp[slot][16], the identity in a fresh object (the
 * reference leaves mTcp uninitialised, KeyFrame.cc:63 -- as corb_covis_create treats mTcwBefGBA), and timestamp[slot], 0.  The graph must outlive the object. */
int  corb_traj_create(CorbCovis* g, int capacity_frames, CorbTrajectory** out);
void corb_traj_destroy(CorbTrajectory* t);
/* Tracking::Reset (Tracking.cc:1569-1572): the four lists clear; the per-slot tables stay. */
int  corb_traj_reset(CorbTrajectory* t);

/* The end of Tracking::Track (Tracking.cc:485-504).
 *   cur_slot >= 0  `if(!mCurrentFrame.mTcw.empty())`: the entry (Tcr, id and slot of the graph's keyframe record ref_slot, timestamp, lost).  Tcr given: the caller's
 *                  16 floats -- what corb_track_frame_finish(stage 1) returned; `frames` may then be NULL and cur_slot is not read further.  Tcr = NULL: computed on
 *                  the device from record cur_slot of `frames` and record ref_slot, with stage 1's arithmetic: tfm_gemm4(Tcw(cur), tfm_pose_inverse(Tcw(ref))).
 *                  Neither variant uploads or reads back; with `frames` the work is enqueued on that store's stream, after the log's earlier appends
 *   cur_slot == -1 the `else`: a copy of the last entry's pose, reference and time with the new lost flag; ref_slot, Tcr and timestamp are not read.  On an empty log
 *                  the reference calls back() on an empty list; here CORB_ERR_ARG
 * CORB_ERR_CAPACITY: the log is full, nothing appended.  CORB_ERR_ARG: an empty slot, a slot out of range, a store on another device; nothing written. */
int  corb_traj_append(CorbTrajectory* t, CorbKfStore* frames, int cur_slot, int ref_slot, const float* Tcr /* 16 or NULL */, double timestamp, int lost);

/* KeyFrame::mTimeStamp of a slot (the 256-byte record header has no room for it) */
int  corb_traj_set_keyframe_time(CorbTrajectory* t, int slot, double timestamp);
int  corb_traj_get_keyframe_time(CorbTrajectory* t, int slot, double* timestamp);
/* KeyFrame.cc:666: Tcp(slot) = Tcw(slot) * GetPoseInverse(parent), on the device from the records and the graph's parent field as they stand.  The caller makes it
 * when corb_covis_reparent_children answered reference_sets_bad = 1, before it sets CORB_KF_BAD, which stays the caller's to set.
 * CORB_ERR_ARG with nothing written: an empty slot, a parent of "none", a parent the store does not hold. */
int  corb_traj_set_bad_pose(CorbTrajectory* t, int slot);
/* Tcp of a slot as it stands: for archives, pushes and tests */
int  corb_traj_set_tcp(CorbTrajectory* t, int slot, const float* Tcp /* 16 */);
int  corb_traj_get_tcp(CorbTrajectory* t, int slot, float* Tcp /* 16 */);
/* the log -> host; more than cap entries: CORB_ERR_CAPACITY with *n set and nothing written */
int  corb_traj_get_entries(CorbTrajectory* t, CorbTrajEntry* entries, int cap, int* n);

/* The loop of System::SaveTrajectoryTUM (System.cc:281-306, format 1) or SaveTrajectoryKITTI (:376-400, format 0) over the whole log; one synchronisation and one
 * read-back.  Per entry, with pKF the reference keyframe:
 *   Trw = I; while pKF carries CORB_KF_BAD: Trw = Trw * Tcp(pKF), pKF = parent(pKF); Trw = (Trw * Tcw(pKF)) * Two; Tcw = Tcr * Trw; Rwc = Rcw^T; twc = -Rwc * tcw
 * Two = GetPoseInverse(origin_slot): the caller passes vpKFs[0]; origin_slot = -1: the held record of the smallest id without CORB_KF_BAD.
 *   format 0  a row is 12 floats r00 r01 r02 tx r10 r11 r12 ty r20 r21 r22 tz (of Rwc, twc); lost entries are NOT skipped: the reference does not test mlbLost there
 *   format 1  a row is 7 floats tx ty tz qx qy qz qw, q = Converter::toQuaternion(Rwc); lost entries are skipped (:283)
 * rows [cap][12 | 7], times [cap] (optional), entry_index [cap] (optional): in log order, entry_index[r] naming row r's entry.
 * Where the reference dereferences NULL or never returns, the entry gives no row and is counted: its slot no longer holds its id (n_ref_gone); a bad keyframe whose
 * parent is "none" or not held, or more walk steps than the store has slots -- a cyclic parent chain (n_chain_broken).
 * More rows than cap: CORB_ERR_CAPACITY with *n (and *stats) set and no array written.  CORB_ERR_ARG: format outside 0 / 1, an empty origin slot, no record to be the
 * origin while the log has entries. */
int  corb_traj_frames(CorbTrajectory* t, int origin_slot, int format, float* rows, double* times, int32_t* entry_index, int cap, int* n, CorbTrajStats* stats);
/* The loop of System::SaveKeyFrameTrajectoryTUM (System.cc:326-341): every held record without CORB_KF_BAD in ascending id (KeyFrame::lId); a row is 7 floats
 * tx ty tz qx qy qz qw with t = GetCameraCenter() and q = toQuaternion(Rcw^T), in the world frame as it stands (Two is commented out there, :320, :329); times from
 * the table; ids (optional) the records' ids.  More than cap: CORB_ERR_CAPACITY with *n set and nothing written. */
int  corb_traj_keyframes(CorbTrajectory* t, float* rows, double* times, uint64_t* ids, int cap, int* n);

/* The text the reference's streams write for n rows, byte for byte; host code, no device call.  `<< fixed << setprecision(p)` of a float is %.pf of the value
 * widened to double.  Every line ends in \n, without a trailing blank.
 *   kind 0  KITTI: the 12 values at precision 9, one blank between them (times unused, may be NULL)
 *   kind 1  TUM: the time at precision 6, then the 7 values at precision 9
 *   kind 2  keyframe TUM: the time at precision 6, then the 7 values at precision 7
 * *len = the text's length (no terminator is counted or written).  buf = NULL, or more than cap: CORB_ERR_CAPACITY with *len set and nothing written. */
int  corb_traj_format_rows(int kind, const float* rows, const double* times, int n, char* buf, size_t cap, size_t* len);
/* The matching export (kind 0: corb_traj_frames format 0, 1: format 1, 2: corb_traj_keyframes; origin_slot unused for kind 2), the text, the file.  The monocular
 * refusal of SaveTrajectory* (System.cc:256, :352) is the adapter's: this call does not know the sensor.  CORB_ERR_ARG: the file cannot be written. */
int  corb_traj_save(CorbTrajectory* t, int origin_slot, int kind, const char* path);

#ifdef __cplusplus
}
#endif
#endif

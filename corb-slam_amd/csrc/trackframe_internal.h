// trackframe_internal.h -- Tracking::TrackWithMotionModel / TrackReferenceKeyFrame on records and the end of Tracking::Track (corb_trackframe.cpp,
// trackframe_kernels.hip): what the chains add to the kernels of SearchByProjection(Frame, Frame) / PoseOptimization (track_internal.h, proj_internal.h) and of
// SearchByBoW (match_internal.h, match_device.h)
#pragma once
#include "track_internal.h"
#include "match_internal.h"
#include "corb_track_frame.h"

// the front of a chain's result block: what the kernels decide and leave for the one read-back
struct TrackFrameHead {
    int n_first, wide, n_matches, status;    // the first search's count; the wide search ran; the count that decides; CORB_ERR_OVERFLOW of a search that ran
    int skip[2];                             // TrackPoseDev::skip: [0] status != 0, [1] `return false` before the optimisation (:913, :787-788)
    int n_rejected, n_map;                   // the "Discard outliers" loop: nmatches -= n_rejected; nmatchesMap (zeroed by the host)
    float Tlw[16], Tcw_pred[16], Tcw_before[16];     // mLastFrame.mTcw; the pose the optimisation starts from; the current record's pose as the call found it
    CorbProjPose pose;                       // what SearchByProjection(Frame, Frame) projects with: Tcw_pred, the intrinsics, forward / backward
};

struct TrackFrameDev {
    char* cur; char* last; int F, n_cur, n_last;             // records of the current / last frame (one store)
    const char* ref; int F_ref, n_ref;                       // the reference keyframe's record
    char* map; size_t mp_bytes; int max_obs; CorbIdTable idt;
    TrackFrameHead* head;
    unsigned long long frame_id;
    int check_replaced, has_Tlr, mono, min_matches;          // min_matches: 20 (TrackWithMotionModel), 15 (TrackReferenceKeyFrame)
    float velocity[16], Tlr[16], fx, fy, cx, cy, bf, mb;
    const int* counts1; const int* counts2;                  // n_matches | status of the two searches (TrackWithMotionModel); of SearchByBoW: counts1[0]
    const int* match1; const int* match2;                    // [n_cur] the searches' results
    int* out_match; const unsigned char* rejected; unsigned char* out_outlier;       // [n_cur] into the block (optional)
    // TrackReferenceKeyFrame
    unsigned char* kf_valid;                                 // [n_ref] the keyframe's feature holds a non-bad point of the map
    int n_nodes_ref;                                         // launch bound of the node walk (the host mirror's count)
    CorbBowDev bow;
};

// CheckReplacedInLastFrame (when asked) and the fill of the current frame, one launch
void trackframe_launch_open(const TrackFrameDev& t, int fill, hipStream_t s);
// UpdateLastFrame's pose, SetPose(mVelocity * mLastFrame.mTcw), the matcher's pose block (one workgroup)
void trackframe_launch_motion_pose(const TrackFrameDev& t, hipStream_t s);
// which search counts, its matches into the record, the decision `nmatches < 20`
void trackframe_launch_select(const TrackFrameDev& t, hipStream_t s);
// SearchByBoW(pKF, F, vpMapPointMatches): validity of the keyframe's features, the walk over the common vocabulary nodes found on the device, the rotation filter
void trackframe_launch_bow(const TrackFrameDev& t, hipStream_t s);
// `nmatches < 15`, setMapPointMatches, SetPose(mLastFrame.mTcw)
void trackframe_launch_set_matches(const TrackFrameDev& t, hipStream_t s);
// the "Discard outliers" loop and the packing of the result block
void trackframe_launch_tail(const TrackFrameDev& t, hipStream_t s);
// the loops at the end of Tracking::Track; Tcr (16 floats on the device) is written in stage 1
void trackframe_launch_finish(const TrackFrameDev& t, int stage, float* Tcr, hipStream_t s);

// trackframe_kernels.hip -- Tracking::TrackWithMotionModel (C/src/Tracking.cc:886-949), Tracking::TrackReferenceKeyFrame (:775-817) and the two per-feature loops
// at the end of Tracking::Track (:438-447, :463-467, :491) on records, the parts the separate calls do not have: CheckReplacedInLastFrame, the poses computed from
// the records, the decisions on the matchers' counts, setMapPointMatches, the "Discard outliers" loop with its writes into the MapPoints.  Small kernels in stream
// order, no grid barrier.  Integer atomics and same-value stores only: no result depends on the order they land in.
#include "trackframe_internal.h"
#include "trackframe_math.h"
#include "track_device.h"
#include "match_device.h"

namespace {

__device__ __forceinline__ const CorbMapPointRecord* tf_find(const TrackFrameDev& t, unsigned long long id) { return track_find_mp(t.map, t.mp_bytes, t.idt, id); }
__device__ __forceinline__ CorbMapPointScratch* tf_scratch(const TrackFrameDev& t, const CorbMapPointRecord* r)
{
    return reinterpret_cast<CorbMapPointScratch*>(t.map + (reinterpret_cast<const char*>(r) - t.map) + MpLayout(t.max_obs).scratch);      // (the record, writable)
}
__device__ __forceinline__ float* tf_pose(char* rec) { return reinterpret_cast<KfHeader*>(rec)->m.Tcw; }

// CheckReplacedInLastFrame (:754-772) for i < n_last; fill(mvpMapPoints, NULL) of a fresh Frame (:896) for i < n_cur
__global__ __launch_bounds__(256) void trackframe_open_kernel(TrackFrameDev t, int fill)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const RecLayout L(t.F);
    if (t.check_replaced && i < t.n_last) {
        const CorbMapPointRecord* r = tf_find(t, track_held_id(t.last, L, i));
        if (r) {                                                                                             // MapPoint* pRep = pMP->GetReplaced(); if(pRep) ... = pRep
            const unsigned long long rep = reinterpret_cast<const CorbMapPointCounters*>(reinterpret_cast<const char*>(r) + sizeof(CorbMapPointRecord))->replaced_by;
            if (rep != 0) reinterpret_cast<unsigned long long*>(t.last + L.mp_id)[i] = rep - 1;
        }
    }
    if (fill && i < t.n_cur) {
        reinterpret_cast<unsigned long long*>(t.cur + L.mp_id)[i] = CORB_NO_MAP_POINT;
        reinterpret_cast<unsigned char*>(t.cur + L.flags)[i] &= (unsigned char)~(CORB_FEATURE_OUTLIER | CORB_FEATURE_DISCARDED);
    }
}

// mLastFrame.SetPose(Tlr*pRef->GetPose()) (:825); mCurrentFrame.SetPose(mVelocity*mLastFrame.mTcw) (:894): a lane per element, trackframe_math.h's sums
__global__ __launch_bounds__(64) void trackframe_motion_pose_kernel(TrackFrameDev t)
{
    __shared__ float Tlw[16], Tpred[16];
    const int e = threadIdx.x;
    if (e < 16) {
        t.head->Tcw_before[e] = tf_pose(t.cur)[e];
        Tlw[e] = t.has_Tlr ? tfm_gemm4_at(t.Tlr, tf_pose(const_cast<char*>(t.ref)), e >> 2, e & 3) : tf_pose(t.last)[e];
    }
    __syncthreads();
    if (e < 16) {
        if (t.has_Tlr) tf_pose(t.last)[e] = Tlw[e];
        Tpred[e] = tfm_gemm4_at(t.velocity, Tlw, e >> 2, e & 3);
        tf_pose(t.cur)[e] = Tpred[e];
        t.head->Tlw[e] = Tlw[e]; t.head->Tcw_pred[e] = Tpred[e]; t.head->pose.Tcw[e] = Tpred[e];
    }
    __syncthreads();
    if (e == 0) {
        CorbProjPose& P = t.head->pose;
        P.fx = t.fx; P.fy = t.fy; P.cx = t.cx; P.cy = t.cy; P.bf = t.bf;
        int fw, bw;
        tfm_motion_direction(Tpred, Tlw, t.mb, t.mono, &fw, &bw);
        P.forward = fw; P.backward = bw;
    }
}

// if(nmatches<20) { fill; nmatches = SearchByProjection(..., 2*th, ...) } if(nmatches<20) return false; (:907-914) and the matches of the search that counts
// (ORBmatcher.cc:1582 / 1597).  The frame is all NULL since the fill, so the other search leaves no trace
__global__ __launch_bounds__(256) void trackframe_select_kernel(TrackFrameDev t)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int n1 = t.counts1[0], wide = n1 < t.min_matches ? 1 : 0;
    if (f == 0) {
        const int n = wide ? t.counts2[0] : n1, st = t.counts1[1] | (wide ? t.counts2[1] : 0);
        t.head->n_first = n1; t.head->wide = wide; t.head->n_matches = n; t.head->status = st;
        t.head->skip[0] = st != 0; t.head->skip[1] = n < t.min_matches;
    }
    if (f >= t.n_cur) return;
    const int m = wide ? t.match2[f] : t.match1[f];
    if (t.out_match) t.out_match[f] = m;
    if (m < 0 || m >= t.n_last) return;
    const RecLayout L(t.F);
    reinterpret_cast<unsigned long long*>(t.cur + L.mp_id)[f] = reinterpret_cast<const unsigned long long*>(t.last + L.mp_id)[m];
}

// ---- SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) (ORBmatcher.cc:160-288) for the one pair ----
// if(!pMP) continue; if(pMP->isBad()) continue; (:195-200) from the keyframe record's ids and the map, not from the record's CORB_FEATURE_HAS_MP byte
__global__ __launch_bounds__(256) void trackframe_kf_valid_kernel(TrackFrameDev t)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= t.n_ref) return;
    const RecLayout L(t.F_ref);
    const CorbMapPointRecord* r = tf_find(t, reinterpret_cast<const unsigned long long*>(t.ref + L.mp_id)[i]);
    t.kf_valid[i] = (r && !(r->flags & CORB_MP_BAD)) ? 1 : 0;
}
// a wavefront per node of the keyframe's FeatureVector: its position in the frame's (both ascend in the node id: a binary search, the same for every lane), then
// the walk of match_device.h.  The frame's node count is read from its record, where ComputeBoW may have written it a kernel ago
__global__ __launch_bounds__(256) void trackframe_bow_match_kernel(TrackFrameDev t)
{
    const int lane = threadIdx.x & 63, na = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n_a = min(reinterpret_cast<const KfHeader*>(t.ref)->n_nodes, t.n_nodes_ref);
    if (na >= n_a) return;
    const RecLayout La(t.F_ref), Lb(t.F);
    const uint32_t node = reinterpret_cast<const uint32_t*>(t.ref + La.fv_node)[na];
    const uint32_t* nodes_b = reinterpret_cast<const uint32_t*>(t.cur + Lb.fv_node);
    int lo = 0, hi = min(max(reinterpret_cast<const KfHeader*>(t.cur)->n_nodes, 0), t.F);
    const int n_b = hi;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (nodes_b[mid] < node) lo = mid + 1; else hi = mid; }
    if (lo >= n_b || nodes_b[lo] != node) return;
    bow_match_node(t.bow, na, lo, lane);
}
__global__ __launch_bounds__(256) void trackframe_bow_rot_kernel(TrackFrameDev t)
{
    __shared__ int ind[3];
    rot_finalize(t.bow.match, t.bow.bin, t.n_cur, t.bow.hist, t.bow.n_matches, 1, ind);
}

// if(nmatches<15) return false; mCurrentFrame.setMapPointMatches(vpMapPointMatches); mCurrentFrame.SetPose(mLastFrame.mTcw); (:787-791)
__global__ __launch_bounds__(256) void trackframe_set_matches_kernel(TrackFrameDev t)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int n = t.counts1[0];
    const bool go = n >= t.min_matches;
    if (f == 0) {
        t.head->n_first = n; t.head->wide = 0; t.head->n_matches = n; t.head->status = 0;
        t.head->skip[0] = 0; t.head->skip[1] = go ? 0 : 1;
    }
    if (f < 16) {
        const float before = tf_pose(t.cur)[f], lw = tf_pose(t.last)[f];
        t.head->Tcw_before[f] = before; t.head->Tlw[f] = lw; t.head->Tcw_pred[f] = lw;
        if (go) tf_pose(t.cur)[f] = lw;
    }
    if (f >= t.n_cur) return;
    const int m = t.match1[f];
    if (t.out_match) t.out_match[f] = m;
    if (!go) return;
    const RecLayout L(t.F), LK(t.F_ref);
    reinterpret_cast<unsigned long long*>(t.cur + L.mp_id)[f] = (m >= 0 && m < t.n_ref) ? reinterpret_cast<const unsigned long long*>(t.ref + LK.mp_id)[m] : CORB_NO_MAP_POINT;
    reinterpret_cast<unsigned char*>(t.cur + L.flags)[f] &= (unsigned char)~(CORB_FEATURE_OUTLIER | CORB_FEATURE_DISCARDED);
}

// the "Discard outliers" loop (:919-940 = :796-814) on the record track_pose_finish_kernel(discard) left: a thread per feature
__global__ __launch_bounds__(256) void trackframe_tail_kernel(TrackFrameDev t)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= t.n_cur) return;
    const bool skipped = t.head->skip[0] | t.head->skip[1];
    bool rej = false, in_map = false;
    if (!skipped) {
        const RecLayout L(t.F);
        rej = t.rejected[i] != 0;
        if (rej) {                                                                   // the id stays in the record behind CORB_FEATURE_DISCARDED: it names pMP
            const CorbMapPointRecord* r = tf_find(t, reinterpret_cast<const unsigned long long*>(t.cur + L.mp_id)[i]);
            if (r) { CorbMapPointScratch* sc = tf_scratch(t, r); sc->track_in_view = 0; sc->last_frame_seen = t.frame_id; }      // (two features of one point store the same values)
        } else {
            const CorbMapPointRecord* r = tf_find(t, track_held_id(t.cur, L, i));
            in_map = r && r->n_obs > 0;                                              // else if(pMP->Observations()>0) nmatchesMap++;
        }
    }
    if (t.out_outlier) t.out_outlier[i] = rej ? 1 : 0;
    const unsigned long long mr = __ballot(rej), mm = __ballot(in_map);             // one add per wavefront and counter
    const int lane = threadIdx.x & 63;
    if (mr && lane == __ffsll((long long)mr) - 1) atomicAdd(&t.head->n_rejected, __popcll(mr));
    if (mm && lane == __ffsll((long long)mm) - 1) atomicAdd(&t.head->n_map, __popcll(mm));
}

// stage 0: "Clean VO matches" (:438-447); stage 1: the outliers' points leave the frame (:463-467) and Tcr = mTcw * mpReferenceKF->GetPoseInverse() (:491)
__global__ __launch_bounds__(256) void trackframe_finish_kernel(TrackFrameDev t, int stage, float* Tcr)
{
    __shared__ float Twc[16];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (stage == 1 && blockIdx.x == 0) {
        if (threadIdx.x == 0) tfm_pose_inverse(tf_pose(const_cast<char*>(t.ref)), Twc);
        __syncthreads();
        if (threadIdx.x < 16) Tcr[threadIdx.x] = tfm_gemm4_at(tf_pose(t.cur), Twc, threadIdx.x >> 2, threadIdx.x & 3);
    }
    if (i >= t.n_cur) return;
    const RecLayout L(t.F);
    const CorbMapPointRecord* r = tf_find(t, track_held_id(t.cur, L, i));
    if (!r) return;
    unsigned char* fl = reinterpret_cast<unsigned char*>(t.cur + L.flags) + i;
    unsigned long long* id = reinterpret_cast<unsigned long long*>(t.cur + L.mp_id) + i;
    if (stage == 0) { if (r->n_obs < 1) { *fl &= (unsigned char)~CORB_FEATURE_OUTLIER; *id = CORB_NO_MAP_POINT; } }
    else if (*fl & CORB_FEATURE_OUTLIER) *id = CORB_NO_MAP_POINT;
}

}  // namespace

void trackframe_launch_open(const TrackFrameDev& t, int fill, hipStream_t s)
{
    const int n = max(t.check_replaced ? t.n_last : 0, fill ? t.n_cur : 0);
    if (n > 0) hipLaunchKernelGGL(trackframe_open_kernel, dim3((n + 255) / 256), dim3(256), 0, s, t, fill);
}
void trackframe_launch_motion_pose(const TrackFrameDev& t, hipStream_t s) { hipLaunchKernelGGL(trackframe_motion_pose_kernel, dim3(1), dim3(64), 0, s, t); }
void trackframe_launch_select(const TrackFrameDev& t, hipStream_t s)
{
    hipLaunchKernelGGL(trackframe_select_kernel, dim3((max(t.n_cur, 1) + 255) / 256), dim3(256), 0, s, t);
}
void trackframe_launch_bow(const TrackFrameDev& t, hipStream_t s)
{
    if (t.n_ref > 0) hipLaunchKernelGGL(trackframe_kf_valid_kernel, dim3((t.n_ref + 255) / 256), dim3(256), 0, s, t);
    if (t.n_nodes_ref > 0 && t.n_ref > 0 && t.n_cur > 0) hipLaunchKernelGGL(trackframe_bow_match_kernel, dim3((t.n_nodes_ref + 3) / 4), dim3(256), 0, s, t);
    if (t.bow.check_ori && t.n_cur > 0) hipLaunchKernelGGL(trackframe_bow_rot_kernel, dim3(1), dim3(256), 0, s, t);
}
void trackframe_launch_set_matches(const TrackFrameDev& t, hipStream_t s)
{
    hipLaunchKernelGGL(trackframe_set_matches_kernel, dim3((max(t.n_cur, 16) + 255) / 256), dim3(256), 0, s, t);
}
void trackframe_launch_tail(const TrackFrameDev& t, hipStream_t s)
{
    if (t.n_cur > 0) hipLaunchKernelGGL(trackframe_tail_kernel, dim3((t.n_cur + 255) / 256), dim3(256), 0, s, t);
}
void trackframe_launch_finish(const TrackFrameDev& t, int stage, float* Tcr, hipStream_t s)
{
    hipLaunchKernelGGL(trackframe_finish_kernel, dim3((max(t.n_cur, 1) + 255) / 256), dim3(256), 0, s, t, stage, Tcr);
}

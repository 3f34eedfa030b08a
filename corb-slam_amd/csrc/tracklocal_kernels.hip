// tracklocal_kernels.hip -- Tracking::TrackLocalMap (C/src/Tracking.cc:951-992) on records, the parts the separate calls do not have: SearchLocalPoints over the
// local list where UpdateLocalMap left it (slots on the device) with the writes the reference makes into its MapPoints (IncreaseVisible, mnLastFrameSeen,
// isInFrustum's mTrack* fields), and the tail (IncreaseFound, mnMatchesInliers, the stereo outliers' points).  Integer atomics on distinct records and same-value
// stores only: no result depends on the order they land in.
#include "tracklocal_internal.h"
#include "track_device.h"

__device__ __forceinline__ bool tracklocal_failed(const LocalMapHead* head) { return head && (head->status | head->fail); }
__device__ __forceinline__ CorbMapPointCounters* tracklocal_counters(const TrackLocalMapDev& t, const CorbMapPointRecord* r)
{
    return reinterpret_cast<CorbMapPointCounters*>(t.map + (reinterpret_cast<const char*>(r) - t.v.mp_base) + sizeof(CorbMapPointRecord));
}
__device__ __forceinline__ CorbMapPointScratch* tracklocal_scratch(const TrackLocalMapDev& t, const CorbMapPointRecord* r)
{
    return reinterpret_cast<CorbMapPointScratch*>(t.map + (reinterpret_cast<const char*>(r) - t.v.mp_base) + MpLayout(t.max_obs).scratch);
}

// track_local_frame_kernel's decisions (the "seen in this frame" set, the claims) and, for a feature that holds a good point, :1182-1184
__global__ __launch_bounds__(256) void tracklocal_frame_kernel(TrackLocalMapDev t)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= t.v.n_cur) return;
    unsigned char cl = 0;
    if (!tracklocal_failed(t.head)) {
        const RecLayout L(t.v.F);
        unsigned long long* mid = reinterpret_cast<unsigned long long*>(t.v.cur + L.mp_id);
        const unsigned long long id = mid[i];
        const bool discarded = reinterpret_cast<const unsigned char*>(t.v.cur + L.flags)[i] & CORB_FEATURE_DISCARDED;
        const CorbMapPointRecord* r = track_find_mp(t.v.mp_base, t.v.mp_bytes, t.v.idt, id);
        if (r) {
            if (discarded) (void)corb_idtab_insert(t.v.inframe, id, i);        // pMP->mnLastFrameSeen = mCurrentFrame.mnId of a discarded outlier (:933)
            else if (r->flags & CORB_MP_BAD) mid[i] = CORB_NO_MAP_POINT;       // if(pMP->isBad()) *vit = NULL;  (:1176-1179)
            else {
                (void)corb_idtab_insert(t.v.inframe, id, i);
                cl = r->n_obs > 0 ? 1 : 0;
                atomicAdd(&tracklocal_counters(t, r)->n_visible, 1);           // pMP->IncreaseVisible(); once per feature
                CorbMapPointScratch* sc = tracklocal_scratch(t, r);
                sc->last_frame_seen = t.frame_id; sc->track_in_view = 0;       // (two features of one point store the same values)
            }
        }
    }
    t.v.claimed[i] = cl;
}

// track_local_points_kernel over the list by slot, with Frame::isInFrustum's writes; entries beyond the true count are no queries
__global__ __launch_bounds__(256) void tracklocal_list_kernel(TrackLocalMapDev t)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= t.v.n_local) return;
    CorbTrackedPoint o; o.proj_x = o.proj_y = o.proj_xr = o.view_cos = 0.f; o.level = 0; o.valid = 0; o.claims = 0; o.pad[0] = o.pad[1] = 0;
    unsigned long long dsc[4] = {0, 0, 0, 0};
    const int n_list = tracklocal_failed(t.head) ? 0 : min(t.head->n_mp, t.v.n_local);
    if (q < n_list) {
        const CorbMapPointRecord* r = reinterpret_cast<const CorbMapPointRecord*>(t.v.mp_base + (size_t)t.list[q] * t.v.mp_bytes);
        if (!(r->flags & CORB_MP_BAD) && corb_idtab_find(t.v.inframe, r->id) < 0) {
            CorbMapPointScratch* sc = tracklocal_scratch(t, r);
            if (track_in_frustum(t.v, r, o) == 0) {
                sc->track_in_view = 1; sc->track_proj_x = o.proj_x; sc->track_proj_y = o.proj_y; sc->track_proj_xr = o.proj_xr;
                sc->track_scale_level = o.level; sc->track_view_cos = o.view_cos;
                atomicAdd(&tracklocal_counters(t, r)->n_visible, 1);           // pMP->IncreaseVisible(); (:1201)
                o.valid = 1; o.claims = r->n_obs > 0 ? 1 : 0;
                const unsigned long long* dp = reinterpret_cast<const unsigned long long*>(r->descriptor);
                dsc[0] = dp[0]; dsc[1] = dp[1]; dsc[2] = dp[2]; dsc[3] = dp[3];
            } else sc->track_in_view = 0;                                      // pMP->mbTrackInView = false; (Frame.cc:272)
        }
    }
    t.v.tracked[q] = o;
#pragma unroll
    for (int k = 0; k < 4; k++) t.v.qdesc[4 * (size_t)q + k] = dsc[k];
    const unsigned long long m = __ballot(o.valid != 0);                       // nToMatch++: one add per wavefront
    if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(t.v.n_in_view, __popcll(m));
}
void tracklocal_launch_prepare(const TrackLocalMapDev& t, hipStream_t s)
{
    if (t.v.n_cur > 0) hipLaunchKernelGGL(tracklocal_frame_kernel, dim3((t.v.n_cur + 255) / 256), dim3(256), 0, s, t);
    if (t.v.n_local > 0) hipLaunchKernelGGL(tracklocal_list_kernel, dim3((t.v.n_local + 255) / 256), dim3(256), 0, s, t);
}

__global__ __launch_bounds__(256) void tracklocal_scatter_kernel(TrackLocalMapDev t)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= t.v.n_cur || tracklocal_failed(t.head)) return;
    const int m = t.v.match[f];
    if (m < 0 || m >= min(t.head->n_mp, t.v.n_local)) return;
    const RecLayout L(t.v.F);
    reinterpret_cast<unsigned long long*>(t.v.cur + L.mp_id)[f] = reinterpret_cast<const CorbMapPointRecord*>(t.v.mp_base + (size_t)t.list[m] * t.v.mp_bytes)->id;
    reinterpret_cast<unsigned char*>(t.v.cur + L.flags)[f] &= (unsigned char)~(CORB_FEATURE_DISCARDED | CORB_FEATURE_OUTLIER);
}
void tracklocal_launch_scatter(const TrackLocalMapDev& t, hipStream_t s)
{
    if (t.v.n_cur > 0) hipLaunchKernelGGL(tracklocal_scatter_kernel, dim3((t.v.n_cur + 255) / 256), dim3(256), 0, s, t);
}

// for(int i=0; i<mCurrentFrame.N; i++) if(mCurrentFrame.mvpMapPoints[i]) ... (:960-978): a thread per feature
__global__ __launch_bounds__(256) void tracklocal_tail_kernel(TrackLocalMapDev t)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 3 && t.out_counts) t.out_counts[i] = t.proj_counts[i];
    if (i >= t.v.n_cur) return;
    const bool failed = tracklocal_failed(t.head);
    if (t.out_match) t.out_match[i] = t.v.match[i];
    if (t.out_outlier) t.out_outlier[i] = failed ? 0 : t.rejected[i];          // (the pose's finish kernel has written `rejected` unless the chain failed)
    bool counts = false;
    if (!failed) {
        const RecLayout L(t.v.F);
        const CorbMapPointRecord* r = track_find_mp(t.v.mp_base, t.v.mp_bytes, t.v.idt, track_held_id(t.v.cur, L, i));
        if (r) {
            if (!(reinterpret_cast<const unsigned char*>(t.v.cur + L.flags)[i] & CORB_FEATURE_OUTLIER)) {
                atomicAdd(&tracklocal_counters(t, r)->n_found, 1);             // mvpMapPoints[i]->IncreaseFound();
                counts = t.only_tracking || r->n_obs > 0;                      // if(!mbOnlyTracking) { if(Observations()>0) mnMatchesInliers++; } else mnMatchesInliers++;
            } else if (t.sensor == 1)
                reinterpret_cast<unsigned long long*>(t.v.cur + L.mp_id)[i] = CORB_NO_MAP_POINT;       // else if(mSensor==System::STEREO) mvpMapPoints[i] = NULL;
        }
    }
    const unsigned long long m = __ballot(counts);                             // one add per wavefront
    if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(t.n_inliers, __popcll(m));
}
void tracklocal_launch_tail(const TrackLocalMapDev& t, hipStream_t s)
{
    const int n = t.v.n_cur > 3 ? t.v.n_cur : 3;
    hipLaunchKernelGGL(tracklocal_tail_kernel, dim3((n + 255) / 256), dim3(256), 0, s, t);
}

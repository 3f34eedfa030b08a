// normal_depth.h -- MapPoint::UpdateNormalAndDepth (C/src/MapPoint.cc:424-472) on a map-point record, shared by the kernels that move points (store_kernels.hip,
// loopfix_kernels.hip).  Which keyframes are at hand, and with which pose, is the caller's: a Lookup gives find(id) -> handle or < 0, pose(handle) -> 16 floats,
// record(handle) -> the keyframe's record.  Device code only.
#pragma once
#include "store_internal.h"
#include "kfinsert_math.h"             // bas_camera_center: stated once for the kernels and the host check

// the first `kept` observations of the record; mvScaleFactors rebuilt from scale_factor as ORBextractor.cc:418-424 does
template <class Lookup>
__device__ __forceinline__ void corb_update_normal_depth(const Lookup& L, CorbMapPointRecord* h, const unsigned long long* okf, const uint32_t* oidx, int kept, const RecLayout& KL, float scale_factor)
{
    const int pr = L.find(h->ref_kf_id);
    if (pr < 0) return;                                                       // pRefKF == nullptr (:438)
    int ref_f = -1;
    float nx = 0.f, ny = 0.f, nz = 0.f; int n = 0;
    const float px = h->world_pos[0], py = h->world_pos[1], pz = h->world_pos[2];
    for (int k = 0; k < kept; k++) {
        if (okf[k] == h->ref_kf_id) ref_f = (int)oidx[k];
        const int p = L.find(okf[k]);
        if (p < 0) continue;                                                  // if (pKF) (:452): a keyframe that is not at hand
        float Ow[3]; bas_camera_center(L.pose(p), Ow);
        const float vx = px - Ow[0], vy = py - Ow[1], vz = pz - Ow[2];
        const double inv = 1.0 / sqrt((double)vx * vx + (double)vy * vy + (double)vz * vz);     // cv::norm accumulates in double; Mat / double scales by its reciprocal
        nx += (float)(vx * inv); ny += (float)(vy * inv); nz += (float)(vz * inv); n++;
    }
    const char* rrec = L.record(pr);
    const KfHeader* rh = reinterpret_cast<const KfHeader*>(rrec);
    if (ref_f < 0 || ref_f >= rh->n || n == 0) return;                        // (:441-444)
    float Or[3]; bas_camera_center(L.pose(pr), Or);
    const float cx = px - Or[0], cy = py - Or[1], cz = pz - Or[2];
    const float dist = (float)sqrt((double)cx * cx + (double)cy * cy + (double)cz * cz);
    const int nl = min(max(rh->m.nlevels, 1), CORB_MAX_LEVELS);
    const int level = min(max(reinterpret_cast<const CorbKeyPoint*>(rrec + KL.kp)[ref_f].octave, 0), nl - 1);
    float sc = 1.f, sc_level = 1.f;                                           // mvScaleFactor[i] = mvScaleFactor[i-1] * scaleFactor (ORBextractor.cc:418-424)
    for (int l = 1; l < nl; l++) { sc *= scale_factor; if (l == level) sc_level = sc; }
    h->max_distance = dist * sc_level;
    h->min_distance = h->max_distance / sc;
    const double rn = 1.0 / (double)n;
    h->normal[0] = (float)(nx * rn); h->normal[1] = (float)(ny * rn); h->normal[2] = (float)(nz * rn);
}

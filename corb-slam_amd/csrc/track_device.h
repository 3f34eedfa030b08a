// track_device.h -- device code the tracking kernels share (track_kernels.hip, tracklocal_kernels.hip): how a feature's MapPoint id reaches a record, and
// Frame::isInFrustum's arithmetic, stated once.  Device code only.
#pragma once
#include "track_internal.h"

__device__ __forceinline__ const CorbMapPointRecord* track_find_mp(const char* mp_base, size_t mp_bytes, const CorbIdTable& idt, unsigned long long id)
{
    if (id == CORB_NO_MAP_POINT) return nullptr;
    const int slot = corb_idtab_find(idt, id);
    return slot < 0 ? nullptr : reinterpret_cast<const CorbMapPointRecord*>(mp_base + (size_t)slot * mp_bytes);
}

// the MapPoint id a feature HOLDS (discarded ones hold none)
__device__ __forceinline__ unsigned long long track_held_id(const char* rec, const RecLayout& L, int i)
{
    const unsigned char fl = reinterpret_cast<const unsigned char*>(rec + L.flags)[i];
    return (fl & CORB_FEATURE_DISCARDED) ? CORB_NO_MAP_POINT : reinterpret_cast<const unsigned long long*>(rec + L.mp_id)[i];
}

// bool Frame::isInFrustum(MapPoint* pMP, float viewingCosLimit) (Frame.cc:270-329) for a non-bad record: 0 = in the frustum, with o.proj_x / _y / _xr, o.view_cos and
// o.level written (:321-326); else the test that returned false, o untouched: 1 depth (:283), 2 image (:291-294), 3 distance (:303-304), 4 viewing cosine (:311-312).
// (3x3 products = cv::gemm on CV_32F: double accumulation, one rounding; cv::norm / Mat::dot = double sums; PredictScale's log as in proj_kernels.hip)
__device__ __forceinline__ int track_in_frustum(const TrackLocalDev& t, const CorbMapPointRecord* r, CorbTrackedPoint& o)
{
    const float* P = r->world_pos;
    float Pc[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double s = __fma_rn((double)t.Tcw[i * 4 + 2], (double)P[2], __fma_rn((double)t.Tcw[i * 4 + 1], (double)P[1], __dmul_rn((double)t.Tcw[i * 4], (double)P[0])));
        Pc[i] = (float)__dadd_rn(s, (double)t.Tcw[i * 4 + 3]);
    }
    if (!(Pc[2] > 0.0f)) return 1;
    const float invz = __fdiv_rn(1.0f, Pc[2]);
    const float u = __fadd_rn(__fmul_rn(__fmul_rn(t.fx, Pc[0]), invz), t.cx), v = __fadd_rn(__fmul_rn(__fmul_rn(t.fy, Pc[1]), invz), t.cy);
    if (u < t.min_x || u > t.max_x || v < t.min_y || v > t.max_y) return 2;
    const float maxD = __fmul_rn(1.2f, r->max_distance), minD = __fmul_rn(0.8f, r->min_distance);
    const float PO[3] = { __fsub_rn(P[0], t.Ow[0]), __fsub_rn(P[1], t.Ow[1]), __fsub_rn(P[2], t.Ow[2]) };
    const float dist = (float)sqrt(__fma_rn((double)PO[2], (double)PO[2], __fma_rn((double)PO[1], (double)PO[1], __dmul_rn((double)PO[0], (double)PO[0]))));
    if (dist < minD || dist > maxD) return 3;
    const double dot = __fma_rn((double)PO[2], (double)r->normal[2], __fma_rn((double)PO[1], (double)r->normal[1], __dmul_rn((double)PO[0], (double)r->normal[0])));
    const float viewCos = (float)__ddiv_rn(dot, (double)dist);
    if (viewCos < t.cos_limit) return 4;
    const float ratio = __fdiv_rn(r->max_distance, dist);
    const float lg = (float)log((double)ratio);
    int lvl = (int)ceilf(__fdiv_rn(lg, t.log_scale));
    if (lvl < 0) lvl = 0; else if (lvl >= t.nlevels) lvl = t.nlevels - 1;
    o.proj_x = u; o.proj_y = v; o.proj_xr = __fsub_rn(u, __fmul_rn(t.bf, invz)); o.view_cos = viewCos; o.level = lvl;
    return 0;
}

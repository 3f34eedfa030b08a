// kfinsert_math.h -- the arithmetic of keyframe insertion (include/corb_keyframe_insert.h), stated once for the kernels (kfinsert_kernels.hip, newpoints_kernels.hip)
// and for the host program that holds it byte-equal to tests/kfinsert_reference.py (tests/host/kfinsert_main.cpp).  Plain C++: no HIP type, no store layout.
// Float expressions are the reference's, as non-fused IEEE operations with the C++ types of the source (-ffp-contract=off); cv::Mat products = cv::gemm (double
// accumulation, one rounding), cv::norm = a double sum (numerics contract).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KFI_HD __host__ __device__ __forceinline__
#else
#define KFI_HD inline
#endif

// a camera as UnprojectStereo reads it: Tcw rows 0..2, Ow, intrinsics
struct NpCam { float T[12]; float Ow[3]; float fx, fy, cx, cy, invfx, invfy; };

// T and fx..cy are set: invfx = 1.0f / fx (Frame.cc), Ow = -Rcw^T * tcw -- exact negation of the transposed rotation, then cv::gemm (proj_host.h camera_centre)
KFI_HD void np_cam_finish(NpCam& c)
{
    c.invfx = 1.0f / c.fx; c.invfy = 1.0f / c.fy;
    for (int i = 0; i < 3; i++) { double s_ = 0; for (int k = 0; k < 3; k++) s_ += (double)(-c.T[k * 4 + i]) * (double)c.T[k * 4 + 3]; c.Ow[i] = (float)s_; }
}
// KeyFrame::UnprojectStereo (C/src/KeyFrame.cc:741-754) = Frame::UnprojectStereo (Frame.cc:670-684): Twc = [Rcw^T | Ow]
KFI_HD void np_unproject_uv(const NpCam& c, float u, float v, float z, float* X)
{
    const float x = (u - c.cx) * z * c.invfx, y = (v - c.cy) * z * c.invfy;
    for (int i = 0; i < 3; i++) X[i] = (float)((double)c.T[0 * 4 + i] * (double)x + (double)c.T[1 * 4 + i] * (double)y + (double)c.T[2 * 4 + i] * (double)z + (double)c.Ow[i]);
}

// ---- the visit rule of CreateNewKeyFrame / UpdateLastFrame (Tracking.cc:1114-1156, :843-883) in closed form ----
// a feature is a candidate when z > 0 (NaN fails); the candidates ascend in (z, i), and positive floats order as their bit patterns
KFI_HD bool kfi_is_candidate(float z) { return z > 0; }
KFI_HD bool kfi_is_far(float z, float th_depth) { return z > th_depth; }
// m candidates of which n_near are not far.  The loop breaks behind the first entry j with z_j > th_depth && j + 1 > 100: the far entries are a suffix of the
// sorted list, so that j is max(100, n_near), and every entry is visited when the list ends before it.  Mode 0 (StereoInitialization) visits every candidate.
KFI_HD int kfi_n_visited(int m, int n_near, int mode)
{
    if (mode == 0) return m;
    const int J = n_near > 100 ? n_near : 100;
    return J < m ? J + 1 : m;
}

// camera centre from a pose (KeyFrame::SetPose: Ow = -Rwc * tcw in float, KeyFrame.cc:120-135); normal_depth.h's UpdateNormalAndDepth reads it from here
KFI_HD void bas_camera_center(const float* T, float* Ow)
{
    for (int a = 0; a < 3; a++) Ow[a] = -(T[0 * 4 + a] * T[3] + T[1 * 4 + a] * T[7] + T[2 * 4 + a] * T[11]);
}

// ---- MapPoint::UpdateNormalAndDepth (MapPoint.cc:424-471) for the single observation of a new stereo point, in the arithmetic of normal_depth.h: the camera
// centre in float, the norm as a double sum, Mat / double as a product with the reciprocal, and n = 1 still divides ----
KFI_HD int kfi_level(int octave, int nlevels) { const int nl = nlevels < 1 ? 1 : (nlevels > 16 ? 16 : nlevels); return octave < 0 ? 0 : (octave > nl - 1 ? nl - 1 : octave); }
// out = normal[3], min_distance, max_distance
KFI_HD void kfi_single_observation(const float* Tcw, const float* X, int octave, int nlevels, const float* scale, float* out)
{
    float Ow[3]; bas_camera_center(Tcw, Ow);
    const float vx = X[0] - Ow[0], vy = X[1] - Ow[1], vz = X[2] - Ow[2];
    const double inv = 1.0 / sqrt((double)vx * vx + (double)vy * vy + (double)vz * vz);
    float nx = 0.f, ny = 0.f, nz = 0.f;
    nx += (float)(vx * inv); ny += (float)(vy * inv); nz += (float)(vz * inv);
    const float dist = (float)sqrt((double)vx * vx + (double)vy * vy + (double)vz * vz);
    const int nl = nlevels < 1 ? 1 : (nlevels > 16 ? 16 : nlevels);
    const double rn = 1.0 / (double)1;
    out[0] = (float)(nx * rn); out[1] = (float)(ny * rn); out[2] = (float)(nz * rn);
    out[4] = dist * scale[kfi_level(octave, nlevels)];
    out[3] = out[4] / scale[nl - 1];
}
// the temporal point of UpdateLastFrame, MapPoint(x3D, cacher, pFrame, idxF) (MapPoint.cc:61-95): Ow = the frame's mOw (the camera centre UnprojectStereo used),
// mNormalVector = (Pos - Ow) / cv::norm, dist = cv::norm(Pos - Ow) rounded to float
KFI_HD void kfi_temporal_point(const NpCam& c, const float* X, int octave, int nlevels, const float* scale, float* out)
{
    const float vx = X[0] - c.Ow[0], vy = X[1] - c.Ow[1], vz = X[2] - c.Ow[2];
    const double nrm = sqrt((double)vx * vx + (double)vy * vy + (double)vz * vz), inv = 1.0 / nrm;
    out[0] = (float)(vx * inv); out[1] = (float)(vy * inv); out[2] = (float)(vz * inv);
    const float dist = (float)nrm;
    const int nl = nlevels < 1 ? 1 : (nlevels > 16 ? 16 : nlevels);
    out[4] = dist * scale[kfi_level(octave, nlevels)];
    out[3] = out[4] / scale[nl - 1];
}

// ---- LocalMapping::MapPointCulling (LocalMapping.cc:161-188) ----
// MapPoint::GetFoundRatio: static_cast<float>(mnFound) / mnVisible -- both converted to float, one division; 0 / 0 is NaN and does not cull
KFI_HD bool kfi_found_ratio_culls(int n_found, int n_visible) { return (float)n_found / (float)n_visible < 0.25f; }
// one observation's share of nObs (MapPoint.cc:155-158): 2 when its keyframe is at hand and mvuRight[idx] >= 0, else 1
KFI_HD int kfi_obs_weight(bool at_hand, float u_right) { return (at_hand && u_right >= 0) ? 2 : 1; }
// the else-if chain, first applicable branch: 1 already bad, 2 found ratio, 3 too few observations two keyframes on, 4 old enough to leave the list, 0 stays
KFI_HD int kfi_cull_decision(bool bad, int n_found, int n_visible, unsigned long long cur_kf_id, long long first_kf_id, int n_obs_weighted, int th_obs)
{
    const int age = (int)cur_kf_id - (int)first_kf_id;
    if (bad) return 1;
    if (kfi_found_ratio_culls(n_found, n_visible)) return 2;
    if (age >= 2 && n_obs_weighted <= th_obs) return 3;
    if (age >= 3) return 4;
    return 0;
}

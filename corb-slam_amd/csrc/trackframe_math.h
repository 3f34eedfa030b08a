// trackframe_math.h -- the pose arithmetic of include/corb_track_frame.h, stated once for the host and the device: the 4x4 products of UpdateLastFrame, SetPose and
// mlRelativeFramePoses, GetPoseInverse, and the forward / backward test of SearchByProjection(Frame, Frame).  Plain C++ for a host compiler (no HIP, no library
// header: a stand-alone host program can include it; compile with -ffp-contract=off like the rest); in a kernel every operation is the explicit round-to-nearest
// intrinsic, so no contraction default can fuse one.
//
// The rule (proj_host.h): a product of CV_32F matrices is cv::gemm -- every element a double sum over k ascending, rounded to float once.  All sixteen elements
// come out of the product: the bottom row is not forced to 0 0 0 1.  (The factors are floats, so each double product is exact and only the additions round.)
#pragma once

#if defined(__HIP_DEVICE_COMPILE__)
#define TFM_HD __host__ __device__ inline
#define TFM_MUL(a, b) __dmul_rn((a), (b))
#define TFM_ADD(a, b) __dadd_rn((a), (b))
#elif defined(__HIPCC__)
#define TFM_HD __host__ __device__ inline
#define TFM_MUL(a, b) ((a) * (b))
#define TFM_ADD(a, b) ((a) + (b))
#else
#define TFM_HD inline
#define TFM_MUL(a, b) ((a) * (b))
#define TFM_ADD(a, b) ((a) + (b))
#endif

// element (i, j) of A * B (row-major 4x4)
TFM_HD float tfm_gemm4_at(const float* A, const float* B, int i, int j)
{
    double s = 0.0;
    for (int k = 0; k < 4; k++) s = TFM_ADD(s, TFM_MUL((double)A[i * 4 + k], (double)B[k * 4 + j]));
    return (float)s;
}
// C = A * B; C may not alias A or B
TFM_HD void tfm_gemm4(const float* A, const float* B, float* C)
{
    for (int e = 0; e < 16; e++) C[e] = tfm_gemm4_at(A, B, e >> 2, e & 3);
}
// Ow = -Rcw^T * tcw as proj_host::camera_centre: the transposed rotation negated exactly, then the double sum over k ascending, one rounding
TFM_HD void tfm_camera_centre(const float* Tcw, float* Ow)
{
    for (int i = 0; i < 3; i++) {
        double s = 0.0;
        for (int k = 0; k < 3; k++) s = TFM_ADD(s, TFM_MUL((double)(-Tcw[k * 4 + i]), (double)Tcw[k * 4 + 3]));
        Ow[i] = (float)s;
    }
}
// KeyFrame::GetPoseInverse (KeyFrame.cc:120-135): Twc = [Rcw^T | Ow ; 0 0 0 1]
TFM_HD void tfm_pose_inverse(const float* Tcw, float* Twc)
{
    float Ow[3];
    tfm_camera_centre(Tcw, Ow);
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) Twc[i * 4 + j] = Tcw[j * 4 + i]; Twc[i * 4 + 3] = Ow[i]; }
    Twc[12] = 0.f; Twc[13] = 0.f; Twc[14] = 0.f; Twc[15] = 1.f;
}
// proj_host::motion_direction: twc = -Rcw^T tcw ; tlc = Rlw twc + tlw ; forward = tlc.z > mb && !mono ; backward = -tlc.z > mb && !mono (ORBmatcher.cc:1480-1491)
TFM_HD void tfm_motion_direction(const float* Tcw, const float* Tlw, float mb, int mono, int* forward, int* backward)
{
    float twc[3];
    tfm_camera_centre(Tcw, twc);
    double s = 0.0;
    for (int k = 0; k < 3; k++) s = TFM_ADD(s, TFM_MUL((double)Tlw[8 + k], (double)twc[k]));
    const float z = (float)TFM_ADD(s, (double)Tlw[11]);
    *forward = (z > mb && !mono) ? 1 : 0;
    *backward = (-z > mb && !mono) ? 1 : 0;
}

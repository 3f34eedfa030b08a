// traj_math.h -- the arithmetic of include/corb_trajectory.h, stated once for the host and the device: the spanning-tree walk of System::SaveTrajectoryTUM / KITTI
// (C/src/System.cc:288-296 = :380-388), a frame's row in both formats, a keyframe's row, Converter::toQuaternion.  Plain C++ on trackframe_math.h's macros (no HIP, no
// library header: a stand-alone host program can include it; compile with -ffp-contract=off like the rest); in a kernel every double operation is the explicit
// round-to-nearest intrinsic.
//
// Every 4x4 product is tfm_gemm4 (cv::gemm on CV_32F: a double sum over k ascending, one rounding, all sixteen elements the product's), the product with the
// identity at the walk's start included.  GetPoseInverse and the camera centre are tfm_pose_inverse / tfm_camera_centre.
#pragma once
#include "trackframe_math.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define TJM_SUB(a, b) __dsub_rn((a), (b))
#define TJM_DIV(a, b) __ddiv_rn((a), (b))
#define TJM_SQRT(a) __dsqrt_rn((a))
#else
#include <cmath>
#define TJM_SUB(a, b) ((a) - (b))
#define TJM_DIV(a, b) ((a) / (b))
#define TJM_SQRT(a) std::sqrt((a))
#endif

#define TJM_KF_BAD 1u                        // CORB_KF_BAD (corb_accel.h)
#define TJM_CHAIN_BROKEN (-1)

// Converter::toQuaternion (Converter.cc:137-149): Eigen::Quaterniond(Matrix3d) of the 3x3 row-major floats M widened to double -- the rule of ba_math.h's quat_from_R --
// then each component rounded to float once: q = x y z w.  No normalisation.  The square root is correctly rounded on both sides.
TFM_HD void tjm_quaternion(const float* M, float* q)
{
    const double m[9] = { (double)M[0], (double)M[1], (double)M[2], (double)M[3], (double)M[4], (double)M[5], (double)M[6], (double)M[7], (double)M[8] };
    double t = TFM_ADD(TFM_ADD(m[0], m[4]), m[8]);
    if (t > 0) {
        t = TJM_SQRT(TFM_ADD(t, 1.0));
        q[3] = (float)TFM_MUL(0.5, t);
        t = TJM_DIV(0.5, t);
        q[0] = (float)TFM_MUL(TJM_SUB(m[7], m[5]), t); q[1] = (float)TFM_MUL(TJM_SUB(m[2], m[6]), t); q[2] = (float)TFM_MUL(TJM_SUB(m[3], m[1]), t);
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[i * 3 + i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = TJM_SQRT(TFM_ADD(TJM_SUB(TJM_SUB(m[i * 3 + i], m[j * 3 + j]), m[k * 3 + k]), 1.0));
        q[i] = (float)TFM_MUL(0.5, t);
        t = TJM_DIV(0.5, t);
        q[3] = (float)TFM_MUL(TJM_SUB(m[k * 3 + j], m[j * 3 + k]), t);
        q[j] = (float)TFM_MUL(TFM_ADD(m[j * 3 + i], m[i * 3 + j]), t);
        q[k] = (float)TFM_MUL(TFM_ADD(m[k * 3 + i], m[i * 3 + k]), t);
    }
}

// Rwc = Rcw^T (row-major 3x3) of a 4x4 pose
TFM_HD void tjm_rotation_transposed(const float* Tcw, float* Rwc)
{
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rwc[i * 3 + j] = Tcw[j * 4 + i];
}

// The walk for the reference keyframe in `slot` over plain per-slot arrays: flags (CORB_KF_BAD), parent_slot (-1: none, or not held), Tcp [n_slots][16],
// Tcw [n_slots][16]:
//   Trw = I; while(pKF->isBad()) { Trw = Trw*pKF->mTcp; pKF = pKF->GetParent(); } Trw = Trw*pKF->GetPose()*Two;
// as a for loop bounded by the slot count.  Returns the steps taken, or TJM_CHAIN_BROKEN where the reference dereferences NULL (a bad keyframe without a held parent)
// or never returns (more steps than the store has slots: the parent chain is cyclic); Trw is then unspecified.
TFM_HD int tjm_walk(int slot, const unsigned int* flags, const int* parent_slot, const float* Tcp, const float* Tcw, int n_slots, const float* Two, float* Trw)
{
    float A[16], B[16];
    for (int e = 0; e < 16; e++) A[e] = (e % 5 == 0) ? 1.f : 0.f;
    int s = slot, steps = 0;
    for (int it = 0; it <= n_slots; it++) {
        if (!(flags[s] & TJM_KF_BAD)) {
            tfm_gemm4(A, Tcw + (size_t)s * 16, B);
            tfm_gemm4(B, Two, Trw);
            return steps;
        }
        if (it == n_slots) break;
        tfm_gemm4(A, Tcp + (size_t)s * 16, B);
        for (int e = 0; e < 16; e++) A[e] = B[e];
        s = parent_slot[s]; steps++;
        if (s < 0 || s >= n_slots) return TJM_CHAIN_BROKEN;
    }
    return TJM_CHAIN_BROKEN;
}

// a frame's pose in the origin's frame: Tcw = Tcr * Trw (System.cc:298 = :390)
// KITTI (:391-399): Rwc = Rcw^T, twc = -Rwc*tcw: r00 r01 r02 tx r10 r11 r12 ty r20 r21 r22 tz.
// twc equals tfm_camera_centre(Tcw): cv::Mat's unary minus scales the product, negating a float is exact, and so it commutes with the one rounding of the sum --
// -(fl(sum of Rwc_ik tcw_k)) = fl(sum of (-Rwc_ik) tcw_k) term by term.
TFM_HD void tjm_row_kitti(const float* Tcr, const float* Trw, float* row)
{
    float Tcw[16], twc[3];
    tfm_gemm4(Tcr, Trw, Tcw);
    tfm_camera_centre(Tcw, twc);
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) row[i * 4 + j] = Tcw[j * 4 + i]; row[i * 4 + 3] = twc[i]; }
}
// TUM (:299-305): tx ty tz qx qy qz qw, q = toQuaternion(Rwc)
TFM_HD void tjm_row_tum(const float* Tcr, const float* Trw, float* row)
{
    float Tcw[16], Rwc[9];
    tfm_gemm4(Tcr, Trw, Tcw);
    tfm_camera_centre(Tcw, row);
    tjm_rotation_transposed(Tcw, Rwc);
    tjm_quaternion(Rwc, row + 3);
}
// SaveKeyFrameTrajectoryTUM (:334-339): R = GetRotation().t(), q = toQuaternion(R), t = GetCameraCenter(): tx ty tz qx qy qz qw
TFM_HD void tjm_row_keyframe(const float* Tcw, float* row)
{
    float Rwc[9];
    tfm_camera_centre(Tcw, row);
    tjm_rotation_transposed(Tcw, Rwc);
    tjm_quaternion(Rwc, row + 3);
}

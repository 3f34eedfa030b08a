/* corb_stereo_rectify.h -- stereo rectification in front of the stereo front-end: what the reference's two stereo mains for unrectified cameras do on the host
 * before every TrackStereo (C/Examples/Stereo/stereo_euroc.cc:64-98,136-137; C/Examples/ROS/ORB_SLAM2/src/ros_stereo.cc:82-107,161-162): read LEFT / RIGHT
 * {K, D, R, P, width, height} from the settings file, build four maps with cv::initUndistortRectifyMap(..., CV_32F, ...), and cv::remap(..., cv::INTER_LINEAR) both
 * images of every frame.  Exported from libcorb_accel.so beside the drop-in boundary of corb_accel.h.
 *
 * A CorbRect belongs to one CorbStereo (borrowed: destroy the rectifier first).  It holds the two eyes' maps in fixed-point form on the device (6 bytes per pixel)
 * and its own raw staging buffer for 2 * max_frames raw images, allocated at create and never replaced.  The maps are built once, on the host.  Per frame the raw
 * pair takes one host-to-device copy and one kernel, which writes the level-0 planes of the stereo handle's image slots 2f (left) and 2f + 1 (right) -- every byte
 * of width x height, zeros included.  The calls take nothing from a workspace lane (WORKSPACE_AUDIT.md).  Argument errors are a status with a message in
 * corb_last_error().  A handle serves one call at a time, as its stereo handle does.
 *
 * The definition of every map entry and every rectified byte is tests/rectify_reference.py (readings: DESIGN.md section 2): 8-bit, one channel, bilinear, constant
 * border 0; pinhole model with up to eight distortion coefficients.  The fisheye model, other interpolations, other borders and colour input are not provided. */
#ifndef CORB_STEREO_RECTIFY_H
#define CORB_STEREO_RECTIFY_H
#include "corb_accel.h"

#ifdef __cplusplus
extern "C" {
#endif

/* LEFT.* / RIGHT.* as in the settings file (stereo_euroc.cc:72-82), row-major: K 3x3, D = (k1, k2, p1, p2, k3, k4, k5, k6) with zeros where the file gives 4 or 5
 * coefficients, R 3x3, P 3x4 (its left 3x3 is used: P_l.rowRange(0,3).colRange(0,3), stereo_euroc.cc:97-98) */
typedef struct CorbRectifyEye { double K[9], D[8], R[9], P[12]; } CorbRectifyEye;
typedef struct CorbRectifyConfig { int32_t raw_width, raw_height; CorbRectifyEye left, right; } CorbRectifyConfig;

typedef struct CorbRect CorbRect;

/* stereo_euroc.cc:64-98 / ros_stereo.cc:82-107.  Maps of the stereo handle's width x height (LEFT.width x LEFT.height = the size the front-end was created
 * with); raw_width x raw_height is the size of the raw images, which may differ.  CORB_ERR_ARG and nothing allocated or launched: the reference's own refusals
 * (:88-93: a zero size, a missing matrix = an all-zero K, R or P of either eye); det(P3x3 R) zero or not finite; a map entry that is not finite or whose
 * magnitude is 2^26 or more; a raw or rectified dimension above 32767. */
int corb_rect_create(const CorbRectifyConfig* cfg, CorbStereo* stereo, CorbRect** out);
/* before the stereo handle's corb_stereo_destroy */
void corb_rect_destroy(CorbRect* h);
/* M1 / M2 of `eye` (0 left, 1 right) as built or as last set: host copies, height x width floats each (either may be NULL) */
int corb_rect_maps(CorbRect* h, int eye, float* map_x, float* map_y);
/* cv::remap with a caller's own maps (height x width floats each): the same checks and the same conversion as create; on CORB_ERR_ARG the eye keeps its maps */
int corb_rect_set_maps(CorbRect* h, int eye, const float* map_x, const float* map_y);
/* stereo_euroc.cc:136-137 for frames first .. first + n - 1 from ONE contiguous block: per frame the raw left image followed by the raw right image
 * (2 x raw_height x raw_width bytes).  One host-to-device copy and one kernel; afterwards corb_stereo_run, corb_stereo_sync and the fetch calls work unchanged. */
int corb_rect_upload_batch(CorbRect* h, int first_frame, int n_frames, const uint8_t* raw_left_right);
/* corb_stereo_frames for raw input: remap (:136-137), then Frame::Frame(stereo), in one call.  The same result layout (corb_stereo_frame_layout), the same status
 * and overflow rule and the same bookkeeping; one transfer each way around one captured kernel chain, one synchronisation. */
int corb_rect_frames(CorbRect* h, int n_frames, const uint8_t* raw_left_right, void* result, CorbStereoFrameTiming* timing);

#ifdef __cplusplus
}
#endif
#endif

// cam_internal.h -- the RGB-D / monocular front-end (corb_cam.cpp, cam_kernels.hip): camera model, input format and the undistortion that
// the host (image bounds) and the device (keypoints) share.  Compile with -ffp-contract=off: the expressions below are specified as the
// non-fused IEEE operations of the reference's OpenCV calls.
#pragma once
#include "corb_internal.h"

struct CorbCamParams {
    int w, h;                     // image size (== level 0 of the extractor)
    int channels;                 // 1, 3 or 4 bytes per input pixel
    int blue_idx;                 // cvtColor's blue index: 0 = BGR(A) order, 2 = RGB(A) order
    int rgbd;                     // 1: a depth plane follows the colour plane (Frame::ComputeStereoFromRGBD); 0: monocular (u_right = depth = -1)
    int depth_f32;                // depth plane format: 0 = uint16, 1 = float32
    int depth_convert;            // 1: depth = (float)raw * depth_f + 0.0f (Mat::convertTo), 0: the f32 plane as it is
    float depth_f;                // 1 / DepthMapFactor (Tracking.cc:141-145)
    float bf;                     // Frame::mbf
    int distorted;                // mDistCoef[0] != 0 (Frame::UndistortKeyPoints: otherwise mvKeysUn = mvKeys)
    double fx, fy, cx, cy;        // the camera matrix as cvUndistortPoints converts it (double of the float settings)
    double k[8];                  // {k1, k2, p1, p2, k3, 0, 0, 0}
    double RR[9];                 // P * R = K * I (double GEMM, row major)
    size_t in_frame_bytes;        // one frame of input: colour plane, then the depth plane (RGB-D)
    size_t color_bytes;           // w * h * channels
    int frame_base;               // first frame of this launch
    int cap;                      // entries per frame of the extractor's output arrays
    const uint8_t* stage;         // [max_frames][in_frame_bytes] device staging of the input
    CorbKeyPoint* keys_un;        // [max_frames][cap]
    float* u_right;               // [max_frames][cap]
    float* depth;                 // [max_frames][cap]
};

// cv::undistortPoints(pts, K, D, noArray(), K) of OpenCV 2.4.8 (cvUndistortPoints, undistort.cpp) for one point, restated literally: every term in double,
// five fixed-point iterations, the zero terms of k and RR included, the result cast to float.
#ifdef __HIPCC__
__host__ __device__
#endif
inline void corb_undistort_point(const CorbCamParams& c, float px, float py, float* ox, float* oy)
{
    const double* k = c.k;
    const double* RR = c.RR;
    const double ifx = 1. / c.fx, ify = 1. / c.fy;
    double x = px, y = py, x0, y0;
    x0 = x = (x - c.cx) * ifx;
    y0 = y = (y - c.cy) * ify;
    for (int j = 0; j < 5; j++) {
        double r2 = x * x + y * y;
        double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x);
        double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    double xx = RR[0] * x + RR[1] * y + RR[2];
    double yy = RR[3] * x + RR[4] * y + RR[5];
    double ww = 1. / (RR[6] * x + RR[7] * y + RR[8]);
    *ox = (float)(xx * ww);
    *oy = (float)(yy * ww);
}

// kernel launchers (cam_kernels.hip); all asynchronous on `stream`
// colour / grey input of frames [0, n) of `c` (stage slots frame_base ..) -> level 0 of extractor images frame_base .. at the pyramid's pitch
void corb_launch_cam_ingest(const CorbCamParams& c, int frame_base, int n_frames, const CorbOrbParams& p, hipStream_t stream, CorbProfiler* prof);
// after the describe kernel: keys_un, u_right, depth of every keypoint of frames frame_base .. frame_base + n - 1
void corb_launch_cam_finish(const CorbCamParams& c, int frame_base, int n_frames, const CorbOrbParams& p, hipStream_t stream, CorbProfiler* prof);
// frames [frame_base, frame_base + n) -> n result blocks of corb_rgbd_frames at `out`
void corb_launch_cam_pack(const CorbCamParams& c, int frame_base, int n_frames, const CorbOrbParams& p, uint8_t* out, const CorbRgbdFrameLayout& lay, hipStream_t stream, CorbProfiler* prof);

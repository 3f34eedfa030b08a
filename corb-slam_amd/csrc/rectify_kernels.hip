// rectify_kernels.hip -- cv::remap(raw, rectified, M1, M2, cv::INTER_LINEAR) of both images of every frame (C/Examples/Stereo/stereo_euroc.cc:136-137,
// C/Examples/ROS/ORB_SLAM2/src/ros_stereo.cc:161-162) straight into the level-0 planes of the extractor's image slots.  gfx950 only.
// The definition of every byte is tests/rectify_reference.py (remap): integer arithmetic only.
#include "rectify_internal.h"

// One destination pixel.  xy = ix | iy << 16 (int16 each), fr = ay * 32 + ax.  The taps (ix, iy) (ix+1, iy) (ix, iy+1) (ix+1, iy+1) are the source byte inside
// W x H and 0 outside (constant border 0); weights 32 (32-ax)(32-ay), 32 ax (32-ay), 32 (32-ax) ay, 32 ax ay sum to 32768; the pixel is (sum + 16384) >> 15.
__device__ __forceinline__ uint32_t rect_pixel(const uint8_t* __restrict__ src, int W, int H, int xy, int fr)
{
    const int ix = (short)(xy & 0xffff), iy = xy >> 16;
    int t00, t01, t10, t11;
    if ((unsigned)ix < (unsigned)(W - 1) && (unsigned)iy < (unsigned)(H - 1)) {      // all four taps inside: no per-tap tests
        const uint8_t* p = src + iy * W + ix;
        t00 = p[0]; t01 = p[1]; t10 = p[W]; t11 = p[W + 1];
    } else {
        if (ix >= W || ix + 1 < 0 || iy >= H || iy + 1 < 0) return 0;
        const bool x0 = (unsigned)ix < (unsigned)W, x1 = (unsigned)(ix + 1) < (unsigned)W, y0 = (unsigned)iy < (unsigned)H, y1 = (unsigned)(iy + 1) < (unsigned)H;
        t00 = x0 && y0 ? src[iy * W + ix] : 0;
        t01 = x1 && y0 ? src[iy * W + ix + 1] : 0;
        t10 = x0 && y1 ? src[(iy + 1) * W + ix] : 0;
        t11 = x1 && y1 ? src[(iy + 1) * W + ix + 1] : 0;
    }
    const int ax = fr & 31, ay = fr >> 5, bx = 32 - ax, by = 32 - ay;
    return (uint32_t)(32 * (bx * by * t00 + ax * by * t01 + bx * ay * t10 + ax * ay * t11) + 16384) >> 15;
}

// One launch for all 2n images (grid.y = image, eye = image & 1).  A lane produces four adjacent bytes of one row from one 16-byte and one 8-byte map load and
// stores them as one aligned dword; the group that holds a row's end stores its bytes one by one.  The source reads are byte gathers: a rectifying warp is close
// to the identity, so neighbouring lanes read neighbouring bytes and the raw image (361 KB at 752 x 480) is served from the L2.
__global__ __launch_bounds__(256) void rect_remap_kernel(CorbRectParams P, const uint8_t* __restrict__ raw, uint8_t* __restrict__ plane, int pitch, size_t image_stride)
{
    const int g = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y, eye = img & 1;
    if (g >= P.groups * P.h) return;
    const int y = g / P.groups, x4 = (g - y * P.groups) * 4;
    const int4 xy = reinterpret_cast<const int4*>(P.xy[eye])[g];
    const uint2 fr = reinterpret_cast<const uint2*>(P.frac[eye])[g];
    const uint8_t* src = raw + (size_t)img * P.raw_w * P.raw_h;
    const uint32_t v0 = rect_pixel(src, P.raw_w, P.raw_h, xy.x, fr.x & 0xffff), v1 = rect_pixel(src, P.raw_w, P.raw_h, xy.y, fr.x >> 16);
    const uint32_t v2 = rect_pixel(src, P.raw_w, P.raw_h, xy.z, fr.y & 0xffff), v3 = rect_pixel(src, P.raw_w, P.raw_h, xy.w, fr.y >> 16);
    uint8_t* d = plane + (size_t)img * image_stride + (size_t)y * pitch + x4;
    if (x4 + 4 <= P.w) *reinterpret_cast<uint32_t*>(d) = v0 | v1 << 8 | v2 << 16 | v3 << 24;
    else {                                                   // one to three bytes are left of the row (x4 < w always)
        d[0] = (uint8_t)v0;
        if (x4 + 1 < P.w) d[1] = (uint8_t)v1;
        if (x4 + 2 < P.w) d[2] = (uint8_t)v2;
    }
}

void corb_launch_rect_remap(const CorbRectParams& P, const uint8_t* raw, int n_images, uint8_t* plane, int pitch, size_t image_stride, hipStream_t stream, CorbProfiler* prof)
{
    CORB_LAUNCH(prof, "rect_remap", rect_remap_kernel, dim3((P.groups * P.h + 255) / 256, n_images), dim3(256), 0, stream, P, raw, plane, pitch, image_stride);
}

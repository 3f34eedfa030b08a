// cam_kernels.hip -- the RGB-D / monocular front-end's kernels (gfx950): colour ingest, keypoint finish (undistortion + depth), result pack.
// The ORB chain between ingest and finish is the extractor's own (orb_kernels.hip).
#include "cam_internal.h"

// ------------------------------------------------------------------------------------------------
// Tracking::GrabImageRGBD / GrabImageMonocular's cvtColor (OpenCV 2.4.8 RGB2Gray<uchar>): gray = (4899 R + 9617 G + 1868 B + 8192) >> 14, alpha ignored; exact
// integer arithmetic.  Replaces orb_ingest_kernel for this front-end: the staged input goes to level 0 of the pyramid at its pitch in one pass, 4 pixels a lane.
template <int CH>
__device__ __forceinline__ uint32_t cam_grey4(const uint8_t* s, int c0, int c2)
{
    uint32_t w[CH];                                       // 4 pixels = CH dwords
    __builtin_memcpy(w, s, 4 * CH);                       // (unaligned load: a row of 3-byte pixels starts anywhere)
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int b0 = CH * i, b1 = b0 + 1, b2 = b0 + 2;
        const int v0 = (w[b0 >> 2] >> (8 * (b0 & 3))) & 255, v1 = (w[b1 >> 2] >> (8 * (b1 & 3))) & 255, v2 = (w[b2 >> 2] >> (8 * (b2 & 3))) & 255;
        out |= (uint32_t)((c0 * v0 + 9617 * v1 + c2 * v2 + 8192) >> 14) << (8 * i);
    }
    return out;
}
template <int CH>
__device__ __forceinline__ uint8_t cam_grey1(const uint8_t* s, int c0, int c2)
{
    if (CH == 1) return s[0];
    return (uint8_t)((c0 * s[0] + 9617 * s[1] + c2 * s[2] + 8192) >> 14);
}

template <int CH>
__global__ __launch_bounds__(256) void cam_ingest_kernel(const CorbCamParams c, const uint8_t* __restrict__ stage, uint8_t* __restrict__ dst, int pitch, size_t dst_image_stride)
{
    const int x4 = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y, img = blockIdx.z;
    if (x4 >= c.w) return;
    const int c0 = c.blue_idx == 0 ? 1868 : 4899, c2 = c.blue_idx == 0 ? 4899 : 1868;      // src[0] * coeffs[bidx ^ 2], src[2] * coeffs[bidx]
    const uint8_t* s = stage + (size_t)img * c.in_frame_bytes + ((size_t)y * c.w + x4) * CH;
    uint8_t* d = dst + (size_t)img * dst_image_stride + (size_t)y * pitch + x4;
    if (x4 + 4 <= c.w) {
        uint32_t v;
        if (CH == 1) __builtin_memcpy(&v, s, 4);
        else v = cam_grey4<CH>(s, c0, c2);
        *reinterpret_cast<uint32_t*>(d) = v;                                  // aligned store (pitch and x4 are multiples of 4)
    } else
        for (int k = 0; x4 + k < c.w; k++) d[k] = cam_grey1<CH>(s + CH * k, c0, c2);
}

void corb_launch_cam_ingest(const CorbCamParams& c0, int frame_base, int n_frames, const CorbOrbParams& p, hipStream_t stream, CorbProfiler* prof)
{
    CorbCamParams c = c0; c.frame_base = frame_base;
    const uint8_t* stage = c.stage + (size_t)frame_base * c.in_frame_bytes;
    uint8_t* dst = p.pyr + (size_t)frame_base * p.arena_per_image + p.lv[0].plane_off;
    const dim3 grid((c.w + 1023) / 1024, c.h, n_frames);
    if (c.channels == 1) CORB_LAUNCH(prof, "cam_ingest_kernel", cam_ingest_kernel<1>, grid, dim3(256), 0, stream, c, stage, dst, p.lv[0].pitch, p.arena_per_image);
    else if (c.channels == 3) CORB_LAUNCH(prof, "cam_ingest_kernel", cam_ingest_kernel<3>, grid, dim3(256), 0, stream, c, stage, dst, p.lv[0].pitch, p.arena_per_image);
    else CORB_LAUNCH(prof, "cam_ingest_kernel", cam_ingest_kernel<4>, grid, dim3(256), 0, stream, c, stage, dst, p.lv[0].pitch, p.arena_per_image);
}

// ------------------------------------------------------------------------------------------------
// Frame::UndistortKeyPoints (Frame.cc:408-438) and Frame::ComputeStereoFromRGBD (:647-668), one lane per keypoint.  The depth is looked up at the DISTORTED
// keypoint (int conversion truncates), read raw from the staged input and scaled as Mat::convertTo does per pixel: (float)raw * f + 0.0f.
__global__ __launch_bounds__(256) void cam_finish_kernel(const CorbCamParams c, const CorbOrbParams p)
{
    const int frame = c.frame_base + blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(p.out_count[frame], c.cap);
    if (i >= n) return;
    const size_t e = (size_t)frame * c.cap + i;
    const CorbKeyPoint kp = p.out_kp[e];
    CorbKeyPoint ku = kp;
    if (c.distorted) corb_undistort_point(c, kp.x, kp.y, &ku.x, &ku.y);
    c.keys_un[e] = ku;
    float ur = -1.0f, dd = -1.0f;
    if (c.rgbd) {
        const int u = (int)kp.x, v = (int)kp.y;
        if (u >= 0 && u < c.w && v >= 0 && v < c.h) {               // (always true for an extractor keypoint; no read outside the plane in any case)
            const uint8_t* dp = c.stage + (size_t)frame * c.in_frame_bytes + c.color_bytes;
            const size_t px = (size_t)v * c.w + u;
            float d;
            if (c.depth_f32) {
                __builtin_memcpy(&d, dp + 4 * px, 4);
                if (c.depth_convert) d = __fadd_rn(__fmul_rn(d, c.depth_f), 0.0f);
            } else {
                uint16_t r; __builtin_memcpy(&r, dp + 2 * px, 2);
                d = __fadd_rn(__fmul_rn((float)r, c.depth_f), 0.0f);
            }
            if (d > 0) { dd = d; ur = __fsub_rn(ku.x, __fdiv_rn(c.bf, d)); }
        }
    }
    c.u_right[e] = ur;
    c.depth[e] = dd;
}

void corb_launch_cam_finish(const CorbCamParams& c0, int frame_base, int n_frames, const CorbOrbParams& p, hipStream_t stream, CorbProfiler* prof)
{
    CorbCamParams c = c0; c.frame_base = frame_base;
    CORB_LAUNCH(prof, "cam_finish_kernel", cam_finish_kernel, dim3((c.cap + 255) / 256, n_frames), dim3(256), 0, stream, c, p);
}

// ------------------------------------------------------------------------------------------------
// corb_rgbd_frames' result blocks: header {n, status}, mvKeys, mvKeysUn, descriptors, mvuRight, mvDepth (dword copies; the sections are 64-byte aligned)
__global__ __launch_bounds__(256) void cam_pack_kernel(const CorbCamParams c, const CorbOrbParams p, uint8_t* out, CorbRgbdFrameLayout lay)
{
    const int f = blockIdx.y, frame = c.frame_base + f;
    uint32_t* o = reinterpret_cast<uint32_t*>(out + (size_t)f * lay.frame_bytes);
    const int n = min(p.out_count[frame], lay.capacity);
    if (blockIdx.x == 0 && threadIdx.x == 0) { o[0] = (uint32_t)n; o[1] = (uint32_t)p.status[frame]; }
    const size_t cap = (size_t)c.cap, e0 = (size_t)frame * cap;
    const uint32_t* src[5] = { reinterpret_cast<const uint32_t*>(p.out_kp + e0), reinterpret_cast<const uint32_t*>(c.keys_un + e0),
                               reinterpret_cast<const uint32_t*>(p.out_desc + e0 * 32), reinterpret_cast<const uint32_t*>(c.u_right + e0),
                               reinterpret_cast<const uint32_t*>(c.depth + e0) };
    const int off[5] = { lay.off_keys, lay.off_keys_un, lay.off_desc, lay.off_u_right, lay.off_depth };
    const int nd[5] = { n * 7, n * 7, n * 8, n, n };
    const int t = blockIdx.x * 256 + threadIdx.x, T = gridDim.x * 256;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        uint32_t* dst = o + off[k] / 4;
        for (int i = t; i < nd[k]; i += T) dst[i] = src[k][i];
    }
}

void corb_launch_cam_pack(const CorbCamParams& c0, int frame_base, int n_frames, const CorbOrbParams& p, uint8_t* out, const CorbRgbdFrameLayout& lay, hipStream_t stream, CorbProfiler* prof)
{
    CorbCamParams c = c0; c.frame_base = frame_base;
    CORB_LAUNCH(prof, "cam_pack_kernel", cam_pack_kernel, dim3(8, n_frames), dim3(256), 0, stream, c, p, out, lay);
}

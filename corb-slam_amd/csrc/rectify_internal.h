// rectify_internal.h -- shared between rectify_kernels.hip and corb_rectify.cpp (include/corb_stereo_rectify.h).
#pragma once
#include "corb_internal.h"

// The maps as the remap kernel reads them, 6 bytes per pixel in two planes per eye, rows of `groups` 4-pixel groups (the width rounded up to 4; the entries past
// the width point outside the image):
//   xy   [height][4 * groups]  int16 pairs {ix, iy}: the source pixel of tap (0, 0), saturated to int16       -- one 16-byte load per lane
//   frac [height][4 * groups]  uint16 ay * 32 + ax: the two 5-bit fractions                                    -- one 8-byte load per lane
struct CorbRectParams {
    const short2* xy[2];          // [eye]
    const uint16_t* frac[2];
    int w, h, groups;             // rectified size; 4-pixel groups per row
    int raw_w, raw_h;
};

// raw: 2 n raw images, eye = image & 1 (the first image is a left one); plane: the level-0 plane of the first image's slot
void corb_launch_rect_remap(const CorbRectParams& P, const uint8_t* raw, int n_images, uint8_t* plane, int pitch, size_t image_stride, hipStream_t stream, CorbProfiler* prof);

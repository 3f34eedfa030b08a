// rectify_math.h -- the host arithmetic of the stereo rectifier (include/corb_stereo_rectify.h): cv::initUndistortRectifyMap(K, D, R, P, size, CV_32F, M1, M2) of
// Examples/Stereo/stereo_euroc.cc:97-98 and the fixed-point form cv::remap(INTER_LINEAR) converts such maps to.  Plain C++ (no HIP, no library header): a
// stand-alone host program can include it (tests/host/rectify_math_main.cpp).  Compile with -ffp-contract=off like the rest.
//
// The reading (tests/rectify_reference.py states the same expressions).  All arithmetic is double, one IEEE operation at a time:
//   A  = P3x3 R            A[r][c] = ((P[r][0] R[0][c] + P[r][1] R[1][c]) + P[r][2] R[2][c]),  P3x3 = the left 3x3 of the 3x4 P
//   iR = adj(A) (1 / det)  det = (a0 (a4 a8 - a5 a7) - a1 (a3 a8 - a5 a6)) + a2 (a3 a7 - a4 a6), the nine adjugate entries as written in rect_inverse3
//   row i starts at _x = i iR[1] + iR[2], _y = i iR[4] + iR[5], _w = i iR[7] + iR[8]; after every pixel _x += iR[0], _y += iR[3], _w += iR[6] -- the running sums
//   are part of the definition
//   pixel: w_ = 1 / _w, x = _x w_, y = _y w_, x2 = x x, y2 = y y, r2 = x2 + y2, _2xy = (2 x) y,
//          kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2),
//          u = fx ((x kr + p1 _2xy) + p2 (r2 + 2 x2)) + cx,   v = fy ((y kr + p1 (r2 + 2 y2)) + p2 _2xy) + cy,   stored as (float)u, (float)v
//   D = (k1, k2, p1, p2, k3, k4, k5, k6)
// Fixed point: sx = rint(map_x * 32) (the float product is exact; round half to even), ix = sat_int16(sx >> 5), ax = sx & 31, and the same for y.
#pragma once
#include <cmath>
#include <cstdint>

// A <- P3x3 * R (row-major 3x3; P is the 3x4 projection, row stride 4)
inline void rect_p3_times_r(const double* P, const double* R, double* A)
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) A[r * 3 + c] = (P[r * 4 + 0] * R[0 * 3 + c] + P[r * 4 + 1] * R[1 * 3 + c]) + P[r * 4 + 2] * R[2 * 3 + c];
}
// iR <- A^-1; false if the determinant is zero or not finite (iR is then untouched)
inline bool rect_inverse3(const double* a, double* iR)
{
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[3] * a[8] - a[5] * a[6], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = (a[0] * c00 - a[1] * c01) + a[2] * c02;
    if (!(det != 0.0) || !std::isfinite(det)) return false;
    const double id = 1.0 / det;
    iR[0] = c00 * id;
    iR[1] = (a[2] * a[7] - a[1] * a[8]) * id;
    iR[2] = (a[1] * a[5] - a[2] * a[4]) * id;
    iR[3] = (a[5] * a[6] - a[3] * a[8]) * id;
    iR[4] = (a[0] * a[8] - a[2] * a[6]) * id;
    iR[5] = (a[2] * a[3] - a[0] * a[5]) * id;
    iR[6] = c02 * id;
    iR[7] = (a[1] * a[6] - a[0] * a[7]) * id;
    iR[8] = (a[0] * a[4] - a[1] * a[3]) * id;
    return true;
}
// map_x / map_y [h][w] of one eye; false if P3x3 R has no inverse
inline bool rect_build_maps(const double* K, const double* D, const double* R, const double* P, int w, int h, float* map_x, float* map_y)
{
    double A[9], iR[9];
    rect_p3_times_r(P, R, A);
    if (!rect_inverse3(A, iR)) return false;
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const double k1 = D[0], k2 = D[1], p1 = D[2], p2 = D[3], k3 = D[4], k4 = D[5], k5 = D[6], k6 = D[7];
    for (int i = 0; i < h; i++) {
        double _x = i * iR[1] + iR[2], _y = i * iR[4] + iR[5], _w = i * iR[7] + iR[8];
        for (int j = 0; j < w; j++, _x += iR[0], _y += iR[3], _w += iR[6]) {
            const double w_ = 1.0 / _w, x = _x * w_, y = _y * w_;
            const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2 * x * y;
            const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
            const double u = fx * ((x * kr + p1 * _2xy) + p2 * (r2 + 2 * x2)) + cx;
            const double v = fy * ((y * kr + p1 * (r2 + 2 * y2)) + p2 * _2xy) + cy;
            map_x[(size_t)i * w + j] = (float)u; map_y[(size_t)i * w + j] = (float)v;
        }
    }
    return true;
}

// what the remap kernel reads per pixel: the integer source pixel and the two 5-bit fractions as ay * 32 + ax
struct RectFixed { int16_t ix, iy; uint16_t frac; };
#define RECT_MAP_LIMIT 67108864.0f      // 2^26: below it rint(v * 32) fits an int32
inline int16_t rect_sat16(int v) { return (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v); }
// false for an entry that is not finite or whose magnitude is 2^26 or more (out is then untouched)
inline bool rect_fix(float mx, float my, RectFixed* out)
{
    if (!std::isfinite(mx) || !std::isfinite(my) || !(std::fabs(mx) < RECT_MAP_LIMIT) || !(std::fabs(my) < RECT_MAP_LIMIT)) return false;
    const int sx = (int)std::lrint(mx * 32.0f), sy = (int)std::lrint(my * 32.0f);          // (default rounding mode: half to even)
    out->ix = rect_sat16(sx >> 5); out->iy = rect_sat16(sy >> 5);
    out->frac = (uint16_t)((sy & 31) * 32 + (sx & 31));
    return true;
}

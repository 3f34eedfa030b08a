// publish_math.h -- the host arithmetic of the map publish (include/corb_map_publish.h): Ttrans.inv() of Cache.cc:479 / :576.  Plain C++ (no HIP, no library
// header): a stand-alone host program can include it (tests/host/publish_math_main.cpp).  Compile with -ffp-contract=off like the rest.
//
// The reading: cv::Mat::inv on a float 4x4 = the cofactor inverse of the FULL 4x4, evaluated in double from the float entries -- the
// general inverse, not the rigid one, because a monocular To2n carries a scale -- times 1 / det, each entry rounded to float once.  The order of operations is
// part of the definition (tests/publish_reference.py inverse4 states the same expressions):
//   det3(a..i)  = a (e i - f h) - b (d i - f g) + c (d h - e g)
//   minor(r, c) = det3 of the rows and columns other than r and c, in ascending order;   cof(r, c) = minor(r, c), negated if r + c is odd
//   det         = ((a00 cof(0,0) + a01 cof(0,1)) + a02 cof(0,2)) + a03 cof(0,3)
//   inv[r][c]   = (float)(cof(c, r) * (1.0 / det))
#pragma once
#include <cmath>

inline double pub_det3(double a, double b, double c, double d, double e, double f, double g, double h, double i)
{
    return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
}
inline double pub_cofactor(const double* A, int r, int c)
{
    int rr[3], cc[3];
    for (int k = 0, j = 0; k < 4; k++) if (k != r) rr[j++] = k;
    for (int k = 0, j = 0; k < 4; k++) if (k != c) cc[j++] = k;
    const double m = pub_det3(A[rr[0] * 4 + cc[0]], A[rr[0] * 4 + cc[1]], A[rr[0] * 4 + cc[2]], A[rr[1] * 4 + cc[0]], A[rr[1] * 4 + cc[1]], A[rr[1] * 4 + cc[2]],
                              A[rr[2] * 4 + cc[0]], A[rr[2] * 4 + cc[1]], A[rr[2] * 4 + cc[2]]);
    return ((r + c) & 1) ? -m : m;
}
// Tinv <- T^-1 (row-major 4x4); false if the determinant is zero or not finite (Tinv is then untouched)
inline bool pub_inverse4(const float* T, float* Tinv)
{
    double A[16], C[16];
    for (int k = 0; k < 16; k++) A[k] = (double)T[k];
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) C[r * 4 + c] = pub_cofactor(A, r, c);
    const double det = ((A[0] * C[0] + A[1] * C[1]) + A[2] * C[2]) + A[3] * C[3];
    if (!(det != 0.0) || !std::isfinite(det)) return false;
    const double inv = 1.0 / det;
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) Tinv[r * 4 + c] = (float)(C[c * 4 + r] * inv);
    return true;
}

// rectify_math_main.cpp -- csrc/rectify_math.h on the host, alone: for every request line `w h` followed by the 38 doubles K[9] D[8] R[9] P[12] as 16-digit hex
// bit patterns, the program appends to the output file one int32 status (1: maps follow, 0: P3x3 R has no inverse, -1: an entry the fixed-point form refuses)
// and, for status 1, map_x[h][w], map_y[h][w] (float32), then ix[h][w], iy[h][w] (int16) and frac[h][w] (uint16).  tests/test_rectify_math_host.py compares
// them with tests/rectify_reference.py bit for bit.
#include "rectify_math.h"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s requests.txt out.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "r"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    int w, h;
    while (fscanf(in, "%d %d", &w, &h) == 2) {
        double v[38];
        for (int k = 0; k < 38; k++) {
            uint64_t bits;
            if (fscanf(in, "%" SCNx64, &bits) != 1) { fprintf(stderr, "short request\n"); return 2; }
            memcpy(&v[k], &bits, 8);
        }
        const size_t n = (size_t)w * h;
        std::vector<float> mx(n), my(n);
        std::vector<int16_t> ix(n), iy(n); std::vector<uint16_t> frac(n);
        int32_t status = rect_build_maps(v, v + 9, v + 17, v + 26, w, h, mx.data(), my.data()) ? 1 : 0;
        for (size_t k = 0; k < n && status == 1; k++) {
            RectFixed f;
            if (!rect_fix(mx[k], my[k], &f)) { status = -1; break; }
            ix[k] = f.ix; iy[k] = f.iy; frac[k] = f.frac;
        }
        fwrite(&status, 4, 1, out);
        if (status != 1) continue;
        fwrite(mx.data(), 4, n, out); fwrite(my.data(), 4, n, out);
        fwrite(ix.data(), 2, n, out); fwrite(iy.data(), 2, n, out); fwrite(frac.data(), 2, n, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}

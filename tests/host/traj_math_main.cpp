// traj_math_main.cpp -- csrc/traj_math.h and csrc/trackframe_math.h as plain host code against a case file that tests/test_traj_math_host.py writes from the definition
// (tests/traj_reference.py): every product, inverse, quaternion, row and walk result must have the definition's bytes, the cyclic parent chain included.
// File (little endian): int32 n_products, n_quaternions, n_rows, n_walks, then
//   product:    A[16] B[16] | A*B [16], GetPoseInverse(B) [16]
//   quaternion: M[9] | q[4]
//   row:        Tcr[16] Trw[16] | KITTI [12], TUM [7], the keyframe row of Tcr [7]
//   walk:       int32 n_slots, slot; uint32 flags[n]; int32 parent_slot[n]; Tcp[n][16]; Tcw[n][16]; Two[16] | int32 steps; Trw[16] (read only when steps >= 0)
// Prints "ok <products> <quaternions> <rows> <walks> broken=<walks that answered TJM_CHAIN_BROKEN>"; exit status 1 with the first difference otherwise.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "trackframe_math.h"
#include "traj_math.h"

namespace {
FILE* f;
template <class T> std::vector<T> get(size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return v;
}
bool same(const char* what, int k, const float* got, const float* want, int n)
{
    if (memcmp(got, want, (size_t)n * 4) == 0) return true;
    for (int i = 0; i < n; i++) if (memcmp(got + i, want + i, 4)) { fprintf(stderr, "%s %d: element %d is %a, the definition has %a\n", what, k, i, got[i], want[i]); break; }
    return false;
}
}

int main(int argc, char** argv)
{
    if (argc != 2 || !(f = fopen(argv[1], "rb"))) { fprintf(stderr, "usage: traj_math_main <case file>\n"); return 2; }
    const std::vector<int32_t> head = get<int32_t>(4);
    for (int k = 0; k < head[0]; k++) {
        const std::vector<float> in = get<float>(32), want = get<float>(32);
        float C[16], D[16];
        tfm_gemm4(in.data(), in.data() + 16, C); tfm_pose_inverse(in.data() + 16, D);
        if (!same("product", k, C, want.data(), 16) || !same("inverse", k, D, want.data() + 16, 16)) return 1;
    }
    for (int k = 0; k < head[1]; k++) {
        const std::vector<float> M = get<float>(9), want = get<float>(4);
        float q[4];
        tjm_quaternion(M.data(), q);
        if (!same("quaternion", k, q, want.data(), 4)) return 1;
    }
    for (int k = 0; k < head[2]; k++) {
        const std::vector<float> in = get<float>(32), want = get<float>(26);
        float a[12], b[7], c[7];
        tjm_row_kitti(in.data(), in.data() + 16, a); tjm_row_tum(in.data(), in.data() + 16, b); tjm_row_keyframe(in.data(), c);
        if (!same("KITTI row", k, a, want.data(), 12) || !same("TUM row", k, b, want.data() + 12, 7) || !same("keyframe row", k, c, want.data() + 19, 7)) return 1;
    }
    int broken = 0;
    for (int k = 0; k < head[3]; k++) {
        const std::vector<int32_t> ns = get<int32_t>(2);
        const size_t n = (size_t)ns[0];
        const std::vector<uint32_t> flags = get<uint32_t>(n);
        const std::vector<int32_t> parent = get<int32_t>(n);
        const std::vector<float> Tcp = get<float>(n * 16), Tcw = get<float>(n * 16), Two = get<float>(16);
        const int32_t steps = get<int32_t>(1)[0];
        const std::vector<float> want = get<float>(16);
        float Trw[16];
        const int got = tjm_walk(ns[1], flags.data(), parent.data(), Tcp.data(), Tcw.data(), ns[0], Two.data(), Trw);
        if (got != steps) { fprintf(stderr, "walk %d: %d steps, the definition has %d\n", k, got, steps); return 1; }
        if (got == TJM_CHAIN_BROKEN) broken++;
        else if (!same("walk", k, Trw, want.data(), 16)) return 1;
    }
    fclose(f);
    printf("ok %d %d %d %d broken=%d\n", head[0], head[1], head[2], head[3], broken);
    return 0;
}

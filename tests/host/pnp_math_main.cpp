// pnp_math_main.cpp -- csrc/pnp_math.h on the host, without the library or a GPU: compute_pose on given sets of correspondences and CheckInliers over the whole problem.
// Built by tests/test_pnp_math_host.py with the host compiler and -ffp-contract=off and compared bit for bit with tests/pnpsolver_reference.py.
//   usage: pnp_math_main <in> <out> [repeat]
//   in : int32 n_problems; per problem: int32 n, int32 n_sets, float K[4] (fx, fy, cx, cy), n x (float X[3], u[2], max_err), per set: int32 len, int32 idx[len]
//   out: per set: double R[9], t[3], rep_errors[3], chosen N; int32 count; n flag bytes
// With repeat > 0 every set is evaluated that many times more and the best wall time of one pass over the file is printed: the serial CPU figure of DESIGN.md section 4.
#include "pnp_math.h"
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Problem { int n; double K[4]; std::vector<PnpCorr> corr; std::vector<std::vector<int>> sets; };

static bool read_all(const char* path, std::vector<Problem>& out)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    int32_t np = 0;
    if (fread(&np, 4, 1, f) != 1 || np < 0) { fclose(f); return false; }
    out.resize((size_t)np);
    for (Problem& p : out) {
        int32_t hdr[2]; float K[4];
        if (fread(hdr, 4, 2, f) != 2 || fread(K, 4, 4, f) != 4 || hdr[0] < 0 || hdr[1] < 0) { fclose(f); return false; }
        p.n = hdr[0];
        for (int k = 0; k < 4; k++) p.K[k] = (double)K[k];
        p.corr.resize((size_t)p.n);
        if (p.n && fread(p.corr.data(), sizeof(PnpCorr), (size_t)p.n, f) != (size_t)p.n) { fclose(f); return false; }
        p.sets.resize((size_t)hdr[1]);
        for (std::vector<int>& s : p.sets) {
            int32_t len = 0;
            if (fread(&len, 4, 1, f) != 1 || len < 0) { fclose(f); return false; }
            s.resize((size_t)len);
            if (len && fread(s.data(), 4, (size_t)len, f) != (size_t)len) { fclose(f); return false; }
            for (int i : s) if (i < 0 || i >= p.n) { fclose(f); return false; }
        }
    }
    fclose(f);
    return true;
}

static double pass(const std::vector<Problem>& problems, FILE* out)
{
    static PnpWork W;
    std::vector<uint8_t> flags;
    const auto t0 = std::chrono::steady_clock::now();
    for (const Problem& p : problems) {
        flags.assign((size_t)p.n, 0);
        for (const std::vector<int>& s : p.sets) {
            PnpPose pose; memset(&pose, 0, sizeof(pose));
            const PnpIndexSet S{p.corr.data(), s.data(), (int)s.size()};
            pnp_compute_pose(S, p.K, W, pose);
            int32_t count = 0;
            for (int i = 0; i < p.n; i++) { flags[i] = pnp_check_inlier(pose.R, pose.t, p.corr[i], p.K) ? 1 : 0; count += flags[i]; }
            if (out) { fwrite(&pose, sizeof(pose), 1, out); fwrite(&count, 4, 1, out); fwrite(flags.data(), 1, flags.size(), out); }
        }
    }
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s <in> <out> [repeat]\n", argv[0]); return 2; }
    std::vector<Problem> problems;
    if (!read_all(argv[1], problems)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    FILE* out = fopen(argv[2], "wb");
    if (!out) { fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    pass(problems, out);
    fclose(out);
    const int repeat = argc > 3 ? atoi(argv[3]) : 0;
    if (repeat > 0) {
        double best = 1e300;
        for (int r = 0; r < repeat; r++) { const double t = pass(problems, nullptr); if (t < best) best = t; }
        printf("seconds_per_pass %.9f\n", best);
    }
    return 0;
}

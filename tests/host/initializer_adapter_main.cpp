// initializer_adapter_main.cpp -- drives corb::Initializer<Frame> (corb-slam_amd/host/corb_adapter_orbslam.hpp) on test doubles of its own that carry the members
// Initializer.cc reads.  TEST INFRASTRUCTURE, not product code.
//   initializer_adapter_main <in.bin> : int32 n_pairs, iterations; float K[4]; per pair: int32 n1, n2; n1 x float pt[2]; n2 x float pt[2]; n1 x int32 vMatches12;
//                                       int32 rand[iterations * 8]
// Pair 0 goes through Initialize on its own, then all pairs through one Initializer::RunBatch.  Prints one line per result (pair 0 twice):
// pair ok status | R21 and t21 as 12 hex floats | per key of frame 1: vbTriangulated and vP3D as hex floats
#include <cstddef>
#include <cstdint>
#include <vector>
#include "corb_adapter_orbslam.hpp"
#include <cstdio>
#include <memory>

namespace mock {
struct Mat {
    int rows = 0, cols = 0; std::vector<float> f;
    template <class T> const T& at(int r, int c) const { return reinterpret_cast<const T&>(f[(size_t)r * cols + c]); }
    template <class T> const T& at(int i) const { return reinterpret_cast<const T&>(f[(size_t)i]); }
    bool empty() const { return f.empty(); }
};
struct Point2f { float x = 0, y = 0; };
struct Point3f { float x = 0, y = 0, z = 0; };
struct KeyPoint { Point2f pt; };
}
namespace corb { namespace adapt {
template <> struct MatFactory<mock::Mat> { static mock::Mat from_floats(int rows, int cols, const float* p) { mock::Mat m; m.rows = rows; m.cols = cols; m.f.assign(p, p + (size_t)rows * cols); return m; } };
} }
struct Frame { std::vector<mock::KeyPoint> mvKeysUn; mock::Mat mK; };
using Init = corb::Initializer<Frame>;

static void print(int pair, bool ok, const Init& ini, const mock::Mat& R21, const mock::Mat& t21, const std::vector<mock::Point3f>& vP3D, const std::vector<bool>& vb)
{
    printf("%d %d %d |", pair, ok ? 1 : 0, ini.result.status);
    for (float v : R21.f) printf(" %a", (double)v);
    for (float v : t21.f) printf(" %a", (double)v);
    printf(" |");
    for (size_t i = 0; i < vb.size(); i++) printf(" %d %a %a %a", vb[i] ? 1 : 0, (double)vP3D[i].x, (double)vP3D[i].y, (double)vP3D[i].z);
    printf("\n");
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    auto rd = [&](void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } };
    int32_t hdr[2]; rd(hdr, sizeof(hdr));
    const int n_pairs = hdr[0], its = hdr[1];
    float K[4]; rd(K, sizeof(K));
    const float Kf[9] = {K[0], 0.f, K[2], 0.f, K[1], K[3], 0.f, 0.f, 1.f};
    std::vector<Frame> ref((size_t)n_pairs), cur((size_t)n_pairs); std::vector<std::vector<int>> m12((size_t)n_pairs); std::vector<std::vector<int32_t>> rv((size_t)n_pairs);
    std::vector<size_t> next((size_t)n_pairs, 0);
    for (int c = 0; c < n_pairs; c++) {
        int32_t n[2]; rd(n, sizeof(n));
        ref[c].mK = corb::adapt::MatFactory<mock::Mat>::from_floats(3, 3, Kf); cur[c].mK = ref[c].mK;
        ref[c].mvKeysUn.resize(n[0]); cur[c].mvKeysUn.resize(n[1]);
        for (auto& k : ref[c].mvKeysUn) rd(&k.pt, 8);
        for (auto& k : cur[c].mvKeysUn) rd(&k.pt, 8);
        std::vector<int32_t> m(n[0]); rd(m.data(), m.size() * 4); m12[c].assign(m.begin(), m.end());
        rv[c].resize((size_t)its * 8); rd(rv[c].data(), rv[c].size() * 4);
    }
    fclose(f);
    std::vector<std::unique_ptr<Init>> inits; std::vector<Init::Job> jobs;
    for (int c = 0; c < n_pairs; c++) {
        auto src = [&rv, &next, c] { return (int)rv[c][next[c]++ % rv[c].size()]; };
        inits.emplace_back(new Init(ref[c], 1.0f, its, src));
        jobs.push_back({inits.back().get(), &cur[c], &m12[c]});
    }
    mock::Mat R21, t21; std::vector<mock::Point3f> vP3D; std::vector<bool> vb;
    const bool ok0 = inits[0]->Initialize(cur[0], m12[0], R21, t21, vP3D, vb);
    print(0, ok0, *inits[0], R21, t21, vP3D, vb);
    Init::RunBatch(jobs);                                             // (pair 0 draws the same values again: its source wraps around)
    for (int c = 0; c < n_pairs; c++) {
        mock::Mat R, t; std::vector<mock::Point3f> P; std::vector<bool> b;
        const bool ok = inits[c]->Result(R, t, P, b);
        print(c, ok, *inits[c], R, t, P, b);
    }
    return 0;
}

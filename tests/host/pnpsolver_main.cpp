// pnpsolver_main.cpp -- drives corb::PnPsolver<Frame, KeyFrame, MapPoint> (corb-slam_amd/host/corb_adapter_orbslam.hpp) on test doubles of its own that carry the members
// PnPsolver.cc reads.  TEST INFRASTRUCTURE, not product code.
//   pnpsolver_main <in.bin> : int32 n_cand, n, chunk, tail, n_calls; float K[4], sigma2[8]; per feature: float pt[2], int32 octave;
//                             per candidate: per feature (float pos[3], int32 state: 0 = NULL, 1 = good, 2 = bad), then int32 rand[(300 + tail) * 4]
// Candidate 0 is built over a Frame, the others over a KeyFrame; all run in one PnPsolver::RunBatch.  Prints one line per (candidate, iterate(chunk) call):
// cand found bNoMore nInliers <indices of vbInliers> | Tcw as 16 hex floats
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
struct KeyPoint { Point2f pt; int octave = 0; };
}
namespace corb { namespace adapt {
template <> struct MatFactory<mock::Mat> { static mock::Mat from_floats(int rows, int cols, const float* p) { mock::Mat m; m.rows = rows; m.cols = cols; m.f.assign(p, p + (size_t)rows * cols); return m; } };
} }
struct Frame { std::vector<mock::KeyPoint> mvKeysUn; std::vector<float> mvLevelSigma2; float fx = 0, fy = 0, cx = 0, cy = 0; };
struct KeyFrame { std::vector<mock::KeyPoint> mvKeysUn; std::vector<float> mvLevelSigma2; float fx = 0, fy = 0, cx = 0, cy = 0; };
struct MP {
    bool bad = false; mock::Mat pos;
    bool isBad() { return bad; }
    mock::Mat GetWorldPos() { return pos; }
};
using Solver = corb::PnPsolver<Frame, KeyFrame, MP>;

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    auto rd = [&](void* p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } };
    int32_t hdr[5]; rd(hdr, sizeof(hdr));
    const int n_cand = hdr[0], n = hdr[1], chunk = hdr[2], tail = hdr[3], n_calls = hdr[4];
    float K[4], sigma2[8]; rd(K, sizeof(K)); rd(sigma2, sizeof(sigma2));
    Frame fr; KeyFrame kf;
    fr.mvKeysUn.resize(n); fr.mvLevelSigma2.assign(sigma2, sigma2 + 8); fr.fx = K[0]; fr.fy = K[1]; fr.cx = K[2]; fr.cy = K[3];
    for (int i = 0; i < n; i++) { float pt[2]; int32_t o; rd(pt, 8); rd(&o, 4); fr.mvKeysUn[i].pt.x = pt[0]; fr.mvKeysUn[i].pt.y = pt[1]; fr.mvKeysUn[i].octave = o; }
    kf.mvKeysUn = fr.mvKeysUn; kf.mvLevelSigma2 = fr.mvLevelSigma2; kf.fx = fr.fx; kf.fy = fr.fy; kf.cx = fr.cx; kf.cy = fr.cy;
    std::vector<std::unique_ptr<MP>> own; std::vector<std::vector<int32_t>> rv((size_t)n_cand); std::vector<size_t> next((size_t)n_cand, 0);
    std::vector<std::unique_ptr<Solver>> solvers; std::vector<Solver*> all;
    for (int c = 0; c < n_cand; c++) {
        std::vector<MP*> matches(n, nullptr);
        for (int i = 0; i < n; i++) {
            float pos[3]; int32_t st; rd(pos, 12); rd(&st, 4);
            if (st == 0) continue;
            own.emplace_back(new MP()); MP* p = own.back().get(); p->pos.rows = 3; p->pos.cols = 1; p->pos.f.assign(pos, pos + 3); p->bad = st == 2; matches[i] = p;
        }
        rv[c].resize((size_t)(300 + tail) * 4); rd(rv[c].data(), rv[c].size() * 4);
        auto src = [&rv, &next, c] { return (int)rv[c][next[c]++ % rv[c].size()]; };
        if (c == 0) solvers.emplace_back(new Solver(fr, matches, src, tail)); else solvers.emplace_back(new Solver(kf, matches, src, tail));
        solvers.back()->SetRansacParameters(0.99, 10, 300, 4, 0.5f, 5.991f);
        all.push_back(solvers.back().get());
    }
    fclose(f);
    Solver::RunBatch(all);
    for (int c = 0; c < n_cand; c++)
        for (int call = 0; call < n_calls; call++) {
            bool bNoMore; std::vector<bool> vb; int nInliers;
            const mock::Mat T = all[c]->iterate(chunk, bNoMore, vb, nInliers);
            printf("%d %d %d %d", c, T.empty() ? 0 : 1, bNoMore ? 1 : 0, nInliers);
            for (size_t i = 0; i < vb.size(); i++) if (vb[i]) printf(" %zu", i);
            printf(" |");
            for (float v : T.f) printf(" %a", (double)v);
            printf("\n");
        }
    return 0;
}

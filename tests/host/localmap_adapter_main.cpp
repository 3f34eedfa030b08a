// localmap_adapter_main.cpp -- drives the spanning-tree methods and UpdateLocalMap of corb::Covisibility<KeyFrame, Db> (corb-slam_amd/host/corb_adapter_orbslam.hpp) on
// test doubles.  TEST INFRASTRUCTURE, not product code.
//   localmap_adapter_main <in.bin> : int32 K, F, n_mp, O, max_connections, n_ops; the keyframes and map points as tests/host/covis_adapter_main.cpp reads them (the
//       LAST keyframe slot is the current frame's record); per op int32 code, k, a, b:
//       0 UpdateConnections(k)   1 EraseConnections(k) + ReparentChildren(k), then CORB_KF_BAD on the record   2 the tree of k (GetParent, GetChilds, hasChild(k, a))
//       3 AddChild(k, a)   4 EraseChild(k, a)   5 ChangeParent(k, a)   6 UpdateLocalMap of the frame (the local keyframes carry over from the last one)
//       7 the same through FrameStoreT::UpdateLocalMap (slots in, slots out), its ids handed to FrameStoreT::SearchLocalPoints' id form
// Keyframes are printed as slots (-1 = NULL).
#include <cstddef>
#include <cstdint>
#include <vector>
#include "corb_adapter_orbslam.hpp"
#include "mock_orbslam.hpp"
#include <cmath>
#include <cstdio>

namespace mock {
struct Db { void UpdateConnections(KeyFrame*) {} };
}
namespace corb { namespace adapt {
template <> struct MatFactory<mock::Mat> { static mock::Mat from_floats(int rows, int cols, const float* p) { mock::Mat m; m.rows = rows; m.cols = cols; m.f.assign(p, p + (size_t)rows * cols); return m; } };
} }

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    auto rd = [&](void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } };
    int32_t hdr[6]; rd(hdr, sizeof(hdr));
    const int K = hdr[0], F = hdr[1], n_mp = hdr[2], O = hdr[3], M = hdr[4], n_ops = hdr[5];
    std::vector<uint64_t> kid((size_t)K); std::vector<uint32_t> kfl((size_t)K); std::vector<int32_t> off((size_t)K + 1);
    rd(kid.data(), (size_t)K * 8); rd(kfl.data(), (size_t)K * 4); rd(off.data(), ((size_t)K + 1) * 4);
    const size_t T = (size_t)off[K];
    std::vector<int32_t> oct(T); std::vector<float> ur(T), dp(T); std::vector<uint64_t> mpid(T);
    rd(oct.data(), T * 4); rd(ur.data(), T * 4); rd(dp.data(), T * 4); rd(mpid.data(), T * 8);
    std::vector<uint64_t> pid((size_t)n_mp); std::vector<uint32_t> pfl((size_t)n_mp); std::vector<int32_t> ooff((size_t)n_mp + 1);
    rd(pid.data(), (size_t)n_mp * 8); rd(pfl.data(), (size_t)n_mp * 4); rd(ooff.data(), ((size_t)n_mp + 1) * 4);
    std::vector<uint64_t> okf((size_t)ooff[n_mp]); std::vector<uint32_t> oidx((size_t)ooff[n_mp]);
    rd(okf.data(), okf.size() * 8); rd(oidx.data(), oidx.size() * 4);

    corb::check_abi();
    CorbKfStore* kfs = nullptr; CorbMpStore* mps = nullptr;
    corb::check(corb_kf_store_create(0, K, F, &kfs), "corb_kf_store_create"); corb::check(corb_mp_store_create(0, n_mp, O, &mps), "corb_mp_store_create");
    std::vector<CorbKeyFrameMeta> meta((size_t)K); std::memset(meta.data(), 0, meta.size() * sizeof(CorbKeyFrameMeta));
    for (int k = 0; k < K; k++) { meta[k].id = kid[k]; meta[k].flags = kfl[k]; meta[k].nlevels = 8; }
    std::vector<CorbKeyPoint> kp(T); std::memset(kp.data(), 0, T * sizeof(CorbKeyPoint));
    for (size_t i = 0; i < T; i++) kp[i].octave = oct[i];
    corb::check(corb_kf_store_put_batch(kfs, 0, K, meta.data(), off.data(), kp.data(), nullptr, ur.data(), dp.data(), mpid.data()), "corb_kf_store_put_batch");
    std::vector<CorbMapPointRecord> rec((size_t)n_mp); std::memset(rec.data(), 0, rec.size() * sizeof(CorbMapPointRecord));
    for (int j = 0; j < n_mp; j++) { rec[j].id = pid[j]; rec[j].flags = pfl[j]; rec[j].n_obs = ooff[j + 1] - ooff[j]; }
    corb::check(corb_mp_store_put_host(mps, 0, n_mp, rec.data(), ooff.data(), okf.data(), oidx.data()), "corb_mp_store_put_host");
    corb::check(corb_mp_store_build_index(mps, 0, n_mp), "corb_mp_store_build_index");

    std::vector<mock::KeyFrame> kf((size_t)K);
    {
        corb::Covisibility<mock::KeyFrame, mock::Db> g(kfs, mps, M, nullptr);
        for (int k = 0; k < K - 1; k++) { kf[k].mnId = (unsigned long)kid[k]; g.Bind(&kf[k], k); }
        auto slot = [&](mock::KeyFrame* p) { return p ? (int)(p - kf.data()) : -1; };
        std::vector<mock::KeyFrame*> local; mock::KeyFrame* ref = nullptr;
        for (int o = 0; o < n_ops; o++) {
            int32_t op[4]; rd(op, sizeof(op));
            mock::KeyFrame* p = &kf[op[1]]; mock::KeyFrame* q = &kf[op[2]];
            if (op[0] == 0) printf("U %d\n", slot(g.UpdateConnections(p)));
            else if (op[0] == 1) {
                g.EraseConnections(p);
                int n = 0; const bool bad = g.ReparentChildren(p, &n);
                meta[op[1]].flags |= CORB_KF_BAD; corb::check(corb_kf_store_set_meta(kfs, op[1], &meta[op[1]]), "corb_kf_store_set_meta");
                printf("R %d %d\n", n, bad ? 1 : 0);
            } else if (op[0] == 2) {
                const auto c = g.GetChilds(p);
                printf("T %d %d %zu", slot(g.GetParent(p)), g.hasChild(p, q) ? 1 : 0, c.size());
                for (auto* x : c) printf(" %d", slot(x));
                printf("\n");
            } else if (op[0] == 3) g.AddChild(p, q);
            else if (op[0] == 4) g.EraseChild(p, q);
            else if (op[0] == 5) g.ChangeParent(p, q);
            else if (op[0] == 6) {
                const auto r = g.UpdateLocalMap(kfs, K - 1, local, &ref, n_mp);
                printf("M %zu %zu %d %d %d %d", local.size(), r.mpSlots.size(), r.nVoted, slot(ref), r.counterEmpty ? 1 : 0, r.nCleared);
                for (auto* x : local) printf(" %d", slot(x));
                for (int v : r.mpSlots) printf(" %d", v);
                printf("\n");
            } else if (op[0] == 7) {
                // the frame store's forms: the map of this session carries no geometry (positions and distance ranges are zero), so no point is in view --
                // the call is made for its arguments, the lists are compared
                using FS = corb::adapt::FrameStoreT<mock::Frame, mock::MapPoint, mock::Mat>;
                std::vector<int32_t> prev; for (auto* x : local) prev.push_back(slot(x));
                const auto r = FS::UpdateLocalMap(g.handle(), kfs, K - 1, prev, 1024, n_mp);
                mock::Frame Fr; Fr.N = off[K] - off[K - 1];
                const float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 5, 0, 0, 0, 1};
                Fr.mTcw = corb::adapt::MatFactory<mock::Mat>::from_floats(4, 4, T);
                Fr.fx = Fr.fy = 500.f; Fr.cx = 320.f; Fr.cy = 240.f; Fr.mbf = 40.f; Fr.mb = 0.08f; Fr.mfLogScaleFactor = std::log(1.2f); Fr.mnScaleLevels = 8;
                for (int l = 0; l < 8; l++) Fr.mvScaleFactors.push_back(std::pow(1.2f, (float)l));
                mock::Frame::mnMinX = 0; mock::Frame::mnMaxX = 640; mock::Frame::mnMinY = 0; mock::Frame::mnMaxY = 480;
                int nToMatch = -1;
                const int n = FS::SearchLocalPoints(kfs, K - 1, mps, Fr, r.mpIds, 1.0f, 0.8f, &nToMatch);
                printf("F %zu %zu %d %d %d %d %d", r.kfSlots.size(), r.mpSlots.size(), r.nVoted, r.refSlot, r.counterEmpty ? 1 : 0, n, nToMatch);
                for (int v : r.kfSlots) printf(" %d", v);
                for (int v : r.mpSlots) printf(" %d", v);
                printf("\n");
            }
        }
    }
    corb_kf_store_destroy(kfs); corb_mp_store_destroy(mps);
    fclose(f);
    return 0;
}

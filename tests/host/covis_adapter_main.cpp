// covis_adapter_main.cpp -- drives corb::Covisibility<KeyFrame, Db> (corb-slam_amd/host/corb_adapter_orbslam.hpp) on test doubles.  TEST INFRASTRUCTURE, not product code.
//   covis_adapter_main <in.bin> : int32 K, F, n_mp, O, max_connections, n_ops; the keyframes (ids u64[K], flags u32[K], feat_off i32[K + 1], octave i32[], u_right f32[],
//       depth f32[], mp_id u64[]); the map points (ids u64[n_mp], flags u32[n_mp], obs_off i32[n_mp + 1], obs_kf u64[], obs_idx u32[]); per op int32 code, k, a, b:
//       0 UpdateConnections(k)   1 EraseConnections(k)   2 the queries of k (a = w of GetCovisiblesByWeight, b = the other keyframe of GetWeight)
//       3 KeyFrameCulling(k, monocular = a, thDepth = b)   4 LocalWindow(k)
// Keyframes are printed as slots (-1 = NULL).  Db is a stand-in that records which keyframes the adapter reports to the place-recognition database.
#include <cstddef>
#include <cstdint>
#include <vector>
#include "corb_adapter_orbslam.hpp"
#include <cstdio>

namespace mock {
struct KeyFrame { unsigned long mnId = 0; };
struct Db { std::vector<KeyFrame*> calls; void UpdateConnections(KeyFrame* p) { calls.push_back(p); } };
}

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
    mock::Db db;
    {
        corb::Covisibility<mock::KeyFrame, mock::Db> g(kfs, mps, M, &db);
        for (int k = 0; k < K; k++) { kf[k].mnId = (unsigned long)kid[k]; g.Bind(&kf[k], k); }
        auto slot = [&](mock::KeyFrame* p) { return p ? (int)(p - kf.data()) : -1; };
        auto list = [&](const char* tag, const std::vector<mock::KeyFrame*>& v) { printf("%s %zu", tag, v.size()); for (auto* p : v) printf(" %d", slot(p)); printf("\n"); };
        for (int o = 0; o < n_ops; o++) {
            int32_t op[4]; rd(op, sizeof(op));
            mock::KeyFrame* p = &kf[op[1]];
            if (op[0] == 0) { db.calls.clear(); mock::KeyFrame* parent = g.UpdateConnections(p); printf("U %d\n", slot(parent)); list("db", db.calls); }
            else if (op[0] == 1) g.EraseConnections(p);
            else if (op[0] == 2) {
                list("V", g.GetVectorCovisibleKeyFrames(p)); list("B1", g.GetBestCovisibilityKeyFrames(p, 1)); list("B10", g.GetBestCovisibilityKeyFrames(p, 10));
                list("W", g.GetCovisiblesByWeight(p, op[2])); printf("w %d\n", g.GetWeight(p, &kf[op[3]]));
            } else if (op[0] == 3) {
                const auto c = g.KeyFrameCulling(p, op[2] != 0, (float)op[3]);
                printf("C %zu", c.size()); for (const auto& e : c) printf(" %d:%d:%d:%d", slot(e.pKF), e.nMPs, e.nRedundantObservations, e.bCull ? 1 : 0); printf("\n");
            } else if (op[0] == 4) {
                std::vector<int32_t> l, x, m; g.LocalWindow(p, l, x, m, K, n_mp);
                printf("L %zu %zu %zu", l.size(), x.size(), m.size()); for (int v : l) printf(" %d", v); for (int v : x) printf(" %d", v); for (int v : m) printf(" %d", v); printf("\n");
            }
        }
    }
    corb_kf_store_destroy(kfs); corb_mp_store_destroy(mps);
    fclose(f);
    return 0;
}

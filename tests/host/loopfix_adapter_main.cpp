// loopfix_adapter_main.cpp -- drives CorrectLoop and PropagateGlobalBA of corb::Covisibility<KeyFrame, Db> (corb-slam_amd/host/corb_adapter_orbslam.hpp) on test
// doubles.  TEST INFRASTRUCTURE, not product code.
//   loopfix_adapter_main <in.bin> : int32 K, F, n_mp, O, max_connections, n_ops; the keyframes and map points as tests/host/covis_adapter_main.cpp reads them, then
//       float Tcw[K][16], TcwGBA[K][16], TcwBef[K][16]; uint64 kf_ba_global[K]; per keyframe uint64 parent, int32 n_children, uint64 children[]; float pos[n_mp][3],
//       pos_gba[n_mp][3]; uint64 mp_ba_global[n_mp], ref_kf[n_mp], corrected_by[n_mp]; per op int32 code, a, n, pad and double v[8], float scale, int32 slots[n]:
//       0 UpdateConnections of the slots   1 CorrectLoop(current = a, Scw = v, scale)   2 PropagateGlobalBA(origins = slots, nLoopKF = a)
// After the ops every object is printed: poses and positions as the bits of their floats.
#include <cstddef>
#include <cstdint>
#include <vector>
#include "corb_adapter_orbslam.hpp"
#include "mock_loopfix.hpp"
#include <array>
#include <cstdio>

namespace mock {
struct Db { void UpdateConnections(LoopKeyFrame*) {} };
}
namespace corb { namespace adapt {
template <> struct MatFactory<mock::Mat> { static mock::Mat from_floats(int rows, int cols, const float* p) { mock::Mat m; m.rows = rows; m.cols = cols; m.f.assign(p, p + (size_t)rows * cols); return m; } };
} }
typedef std::array<double, 8> Sim3;

static void print_floats(const char* tag, const std::vector<float>& f, size_t n)
{
    printf("%s", tag);
    for (size_t i = 0; i < n; i++) { uint32_t u = 0; if (i < f.size()) std::memcpy(&u, &f[i], 4); printf(" %08x", u); }
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
    std::vector<float> Tcw((size_t)K * 16), Tgba((size_t)K * 16), Tbef((size_t)K * 16); std::vector<uint64_t> kba((size_t)K);
    rd(Tcw.data(), Tcw.size() * 4); rd(Tgba.data(), Tgba.size() * 4); rd(Tbef.data(), Tbef.size() * 4); rd(kba.data(), (size_t)K * 8);
    std::vector<uint64_t> parent((size_t)K); std::vector<std::vector<uint64_t>> children((size_t)K);
    for (int k = 0; k < K; k++) { int32_t n = 0; rd(&parent[k], 8); rd(&n, 4); children[k].resize((size_t)n); rd(children[k].data(), (size_t)n * 8); }
    std::vector<float> pos((size_t)n_mp * 3), pgba((size_t)n_mp * 3); std::vector<uint64_t> pba((size_t)n_mp), pref((size_t)n_mp), pcor((size_t)n_mp);
    rd(pos.data(), pos.size() * 4); rd(pgba.data(), pgba.size() * 4); rd(pba.data(), (size_t)n_mp * 8); rd(pref.data(), (size_t)n_mp * 8); rd(pcor.data(), (size_t)n_mp * 8);

    corb::check_abi();
    CorbKfStore* kfs = nullptr; CorbMpStore* mps = nullptr;
    corb::check(corb_kf_store_create(0, K, F, &kfs), "corb_kf_store_create"); corb::check(corb_mp_store_create(0, n_mp, O, &mps), "corb_mp_store_create");
    std::vector<CorbKeyFrameMeta> meta((size_t)K); std::memset(meta.data(), 0, meta.size() * sizeof(CorbKeyFrameMeta));
    for (int k = 0; k < K; k++) {
        meta[k].id = kid[k]; meta[k].flags = kfl[k]; meta[k].nlevels = 8; meta[k].ba_global_for_kf = kba[k];
        std::memcpy(meta[k].Tcw, &Tcw[(size_t)k * 16], 64); std::memcpy(meta[k].TcwGBA, &Tgba[(size_t)k * 16], 64);
    }
    std::vector<CorbKeyPoint> kp(T); std::memset(kp.data(), 0, T * sizeof(CorbKeyPoint));
    for (size_t i = 0; i < T; i++) kp[i].octave = oct[i];
    corb::check(corb_kf_store_put_batch(kfs, 0, K, meta.data(), off.data(), kp.data(), nullptr, ur.data(), dp.data(), mpid.data()), "corb_kf_store_put_batch");
    std::vector<CorbMapPointRecord> rec((size_t)n_mp); std::memset(rec.data(), 0, rec.size() * sizeof(CorbMapPointRecord));
    std::vector<CorbMapPointScratch> sc((size_t)n_mp); std::memset(sc.data(), 0, sc.size() * sizeof(CorbMapPointScratch));
    for (int j = 0; j < n_mp; j++) {
        rec[j].id = pid[j]; rec[j].flags = pfl[j]; rec[j].n_obs = ooff[j + 1] - ooff[j]; rec[j].ref_kf_id = pref[j]; rec[j].ba_global_for_kf = pba[j];
        std::memcpy(rec[j].world_pos, &pos[(size_t)j * 3], 12); std::memcpy(rec[j].pos_gba, &pgba[(size_t)j * 3], 12);
        sc[j].corrected_by_kf = pcor[j];
    }
    corb::check(corb_mp_store_put_host(mps, 0, n_mp, rec.data(), ooff.data(), okf.data(), oidx.data()), "corb_mp_store_put_host");
    corb::check(corb_mp_store_set_scratch(mps, 0, n_mp, sc.data()), "corb_mp_store_set_scratch");
    corb::check(corb_mp_store_build_index(mps, 0, n_mp), "corb_mp_store_build_index");

    typedef corb::adapt::MatFactory<mock::Mat> MF;
    std::vector<mock::LoopKeyFrame> kf((size_t)K); std::vector<mock::LoopMapPoint> mp((size_t)n_mp); std::vector<mock::LoopMapPoint*> vpMP;
    mock::Cache cache;
    {
        corb::Covisibility<mock::LoopKeyFrame, mock::Db> g(kfs, mps, M, nullptr);
        for (int k = 0; k < K; k++) {
            kf[k].mnId = (unsigned long)kid[k]; kf[k].mnBAGlobalForKF = (unsigned long)kba[k]; kf[k].Tcw = MF::from_floats(4, 4, &Tcw[(size_t)k * 16]);
            kf[k].mTcwGBA = MF::from_floats(4, 4, &Tgba[(size_t)k * 16]); kf[k].mTcwBefGBA = MF::from_floats(4, 4, &Tbef[(size_t)k * 16]);
            g.Bind(&kf[k], k);
            g.SetTree(&kf[k], parent[k], false, children[k]);
            corb::check(corb_covis_set_pose_before_gba(g.handle(), k, &Tbef[(size_t)k * 16]), "corb_covis_set_pose_before_gba");
        }
        for (int j = 0; j < n_mp; j++) {
            mp[j].mnId = (unsigned long)pid[j]; mp[j].bad = (pfl[j] & CORB_MP_BAD) != 0; mp[j].pos = MF::from_floats(3, 1, &pos[(size_t)j * 3]);
            mp[j].mnBAGlobalForKF = (unsigned long)pba[j]; mp[j].mnCorrectedByKF = (unsigned long)pcor[j];
            for (int k = 0; k < K; k++) if (kid[k] == pref[j]) mp[j].loopRef = &kf[k];
            vpMP.push_back(&mp[j]);
        }
        for (int o = 0; o < n_ops; o++) {
            int32_t op[4]; double v[8]; float scale; rd(op, sizeof(op)); rd(v, sizeof(v)); rd(&scale, 4);
            std::vector<int32_t> slots((size_t)op[2]); rd(slots.data(), slots.size() * 4);
            if (op[0] == 0) { for (int32_t s : slots) g.UpdateConnections(&kf[s], op[1]); }
            else if (op[0] == 1) {
                std::map<mock::LoopKeyFrame*, Sim3> corrected, non; int np = 0;
                const auto members = g.CorrectLoop<mock::LoopMapPoint, mock::Mat>(&kf[op[1]], v, scale, kfs, mps, 0, vpMP, &cache, corrected, non,
                                                                                 [](const double* p) { Sim3 s; for (int i = 0; i < 8; i++) s[i] = p[i]; return s; }, &np);
                printf("C %zu %d %d %d", members.size(), np, cache.nUpdKF, cache.nUpdMP);
                for (auto* p : members) printf(" %d", (int)(p - kf.data()));
                printf("\n");
                for (auto* p : members) { printf("S"); for (double x : corrected[p]) printf(" %.17g", x); for (double x : non[p]) printf(" %.17g", x); printf("\n"); }
            } else if (op[0] == 2) {
                std::vector<mock::LoopKeyFrame*> origins; for (int32_t s : slots) origins.push_back(&kf[s]);
                const CorbGbaPropagation r = g.PropagateGlobalBA<mock::LoopMapPoint, mock::Mat>(origins, (unsigned long)op[1], kfs, mps, 0, vpMP, &cache);
                printf("G %d %d %d %d %d %d %d %d %d\n", r.n_popped, r.n_reached, r.n_propagated, r.n_revisited, r.n_points_set, r.n_points_moved, r.n_points_skipped, cache.nUpdKF, cache.nUpdMP);
            }
            cache.nUpdKF = cache.nUpdMP = 0;
        }
    }
    for (int k = 0; k < K; k++) {
        printf("K %d %lu", k, kf[k].mnBAGlobalForKF);
        print_floats("", kf[k].Tcw.f, 16); print_floats("", kf[k].mTcwGBA.f, 16); print_floats("", kf[k].mTcwBefGBA.f, 16);
        printf("\n");
    }
    for (int j = 0; j < n_mp; j++) {
        printf("P %d %lu %lu", j, mp[j].mnCorrectedByKF, mp[j].mnCorrectedReference);
        print_floats("", mp[j].pos.f, 3); print_floats("", mp[j].normal.f, 3);
        uint32_t a, b; std::memcpy(&a, &mp[j].minDistance, 4); std::memcpy(&b, &mp[j].maxDistance, 4);
        printf(" %08x %08x\n", a, b);
    }
    corb_kf_store_destroy(kfs); corb_mp_store_destroy(mps);
    fclose(f);
    return 0;
}

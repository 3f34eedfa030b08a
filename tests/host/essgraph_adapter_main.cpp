// essgraph_adapter_main.cpp -- drives AddLoopEdge / GetLoopEdges / OptimizeEssentialGraph of corb::Covisibility<KeyFrame, Db> (corb-slam_amd/host/
// corb_adapter_orbslam.hpp) on test doubles.  TEST INFRASTRUCTURE, not product code.
//   essgraph_adapter_main <in.bin> : int32 K, F, n_mp, O, max_connections, th; the keyframes and map points as tests/host/covis_adapter_main.cpp reads them (the
//       keyframe flags are set AFTER the connections: bit 0 bad, bit 1 fixed); float Tcw[K][16]; per keyframe uint64 parent, int32 n_children, uint64 children[],
//       int32 n_loop, int32 loop_slots[]; float pos[n_mp][3], normal[n_mp][3], min_max[n_mp][2]; uint64 ref_kf[n_mp], corrected_by[n_mp], corrected_ref[n_mp];
//       int32 n_update, slots[] (UpdateConnections in this order); int32 loop_slot, cur_slot, fix_scale, min_weight; float scale_factor; int32 n_corr, slots[],
//       double corrected[n_corr][8], non_corrected[n_corr][8]; int32 n_lc, per entry int32 key slot, n, member slots[]
// Prints the result, the loop edges GetLoopEdges answers, then every object: poses and positions as the bits of their floats.
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

static void print_floats(const std::vector<float>& f, size_t n)
{
    for (size_t i = 0; i < n; i++) { uint32_t u = 0; if (i < f.size()) std::memcpy(&u, &f[i], 4); printf(" %08x", u); }
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    auto rd = [&](void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } };
    auto rd_i = [&]() { int32_t v = 0; rd(&v, 4); return v; };
    int32_t hdr[6]; rd(hdr, sizeof(hdr));
    const int K = hdr[0], F = hdr[1], n_mp = hdr[2], O = hdr[3], M = hdr[4], th = hdr[5];
    std::vector<uint64_t> kid((size_t)K); std::vector<uint32_t> kfl((size_t)K); std::vector<int32_t> off((size_t)K + 1);
    rd(kid.data(), (size_t)K * 8); rd(kfl.data(), (size_t)K * 4); rd(off.data(), ((size_t)K + 1) * 4);
    const size_t T = (size_t)off[K];
    std::vector<int32_t> oct(T); std::vector<float> ur(T), dp(T); std::vector<uint64_t> mpid(T);
    rd(oct.data(), T * 4); rd(ur.data(), T * 4); rd(dp.data(), T * 4); rd(mpid.data(), T * 8);
    std::vector<uint64_t> pid((size_t)n_mp); std::vector<uint32_t> pfl((size_t)n_mp); std::vector<int32_t> ooff((size_t)n_mp + 1);
    rd(pid.data(), (size_t)n_mp * 8); rd(pfl.data(), (size_t)n_mp * 4); rd(ooff.data(), ((size_t)n_mp + 1) * 4);
    std::vector<uint64_t> okf((size_t)ooff[n_mp]); std::vector<uint32_t> oidx((size_t)ooff[n_mp]);
    rd(okf.data(), okf.size() * 8); rd(oidx.data(), oidx.size() * 4);
    std::vector<float> Tcw((size_t)K * 16); rd(Tcw.data(), Tcw.size() * 4);
    std::vector<uint64_t> parent((size_t)K); std::vector<std::vector<uint64_t>> children((size_t)K); std::vector<std::vector<int32_t>> loops((size_t)K);
    for (int k = 0; k < K; k++) {
        rd(&parent[k], 8);
        children[k].resize((size_t)rd_i()); rd(children[k].data(), children[k].size() * 8);
        loops[k].resize((size_t)rd_i()); rd(loops[k].data(), loops[k].size() * 4);
    }
    std::vector<float> pos((size_t)n_mp * 3), nrm((size_t)n_mp * 3), mm((size_t)n_mp * 2); std::vector<uint64_t> pref((size_t)n_mp), pcor((size_t)n_mp), pcref((size_t)n_mp);
    rd(pos.data(), pos.size() * 4); rd(nrm.data(), nrm.size() * 4); rd(mm.data(), mm.size() * 4);
    rd(pref.data(), (size_t)n_mp * 8); rd(pcor.data(), (size_t)n_mp * 8); rd(pcref.data(), (size_t)n_mp * 8);

    corb::check_abi();
    CorbKfStore* kfs = nullptr; CorbMpStore* mps = nullptr;
    corb::check(corb_kf_store_create(0, K, F, &kfs), "corb_kf_store_create"); corb::check(corb_mp_store_create(0, n_mp, O, &mps), "corb_mp_store_create");
    std::vector<CorbKeyFrameMeta> meta((size_t)K); std::memset(meta.data(), 0, meta.size() * sizeof(CorbKeyFrameMeta));
    for (int k = 0; k < K; k++) { meta[k].id = kid[k]; meta[k].nlevels = 8; std::memcpy(meta[k].Tcw, &Tcw[(size_t)k * 16], 64); meta[k].TcwGBA[0] = meta[k].TcwGBA[5] = meta[k].TcwGBA[10] = meta[k].TcwGBA[15] = 1.f; }
    std::vector<CorbKeyPoint> kp(T); std::memset(kp.data(), 0, T * sizeof(CorbKeyPoint));
    for (size_t i = 0; i < T; i++) kp[i].octave = oct[i];
    corb::check(corb_kf_store_put_batch(kfs, 0, K, meta.data(), off.data(), kp.data(), nullptr, ur.data(), dp.data(), mpid.data()), "corb_kf_store_put_batch");
    std::vector<CorbMapPointRecord> rec((size_t)n_mp); std::memset(rec.data(), 0, rec.size() * sizeof(CorbMapPointRecord));
    std::vector<CorbMapPointScratch> sc((size_t)n_mp); std::memset(sc.data(), 0, sc.size() * sizeof(CorbMapPointScratch));
    for (int j = 0; j < n_mp; j++) {
        rec[j].id = pid[j]; rec[j].flags = pfl[j]; rec[j].n_obs = ooff[j + 1] - ooff[j]; rec[j].ref_kf_id = pref[j];
        std::memcpy(rec[j].world_pos, &pos[(size_t)j * 3], 12); std::memcpy(rec[j].normal, &nrm[(size_t)j * 3], 12);
        rec[j].min_distance = mm[(size_t)j * 2]; rec[j].max_distance = mm[(size_t)j * 2 + 1];
        sc[j].corrected_by_kf = pcor[j]; sc[j].corrected_reference = pcref[j];
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
            kf[k].mnId = (unsigned long)kid[k]; kf[k].Tcw = MF::from_floats(4, 4, &Tcw[(size_t)k * 16]);
            kf[k].bad = (kfl[k] & CORB_KF_BAD) != 0; kf[k].fixed = (kfl[k] & CORB_KF_FIXED) != 0;
            g.Bind(&kf[k], k);
        }
        for (int32_t n = rd_i(); n > 0; n--) g.UpdateConnections(&kf[rd_i()], th);
        for (int k = 0; k < K; k++) {
            g.SetTree(&kf[k], parent[k], false, children[k]);
            for (int32_t l : loops[k]) g.AddLoopEdge(&kf[k], &kf[l]);
            if (kfl[k]) { meta[k].flags = kfl[k]; corb::check(corb_kf_store_set_meta(kfs, k, &meta[k]), "corb_kf_store_set_meta"); }
        }
        for (int j = 0; j < n_mp; j++) {
            mp[j].mnId = (unsigned long)pid[j]; mp[j].bad = (pfl[j] & CORB_MP_BAD) != 0; mp[j].fixed = (pfl[j] & CORB_MP_FIXED) != 0;
            mp[j].pos = MF::from_floats(3, 1, &pos[(size_t)j * 3]); mp[j].normal = MF::from_floats(3, 1, &nrm[(size_t)j * 3]);
            mp[j].minDistance = mm[(size_t)j * 2]; mp[j].maxDistance = mm[(size_t)j * 2 + 1];
            mp[j].mnCorrectedByKF = (unsigned long)pcor[j]; mp[j].mnCorrectedReference = (unsigned long)pcref[j];
            for (int k = 0; k < K; k++) if (kid[k] == pref[j]) mp[j].loopRef = &kf[k];
            vpMP.push_back(&mp[j]);
        }
        const int loop_slot = rd_i(), cur_slot = rd_i(), fix_scale = rd_i(), min_weight = rd_i(); float scale = 0; rd(&scale, 4);
        std::map<mock::LoopKeyFrame*, Sim3> corrected, non;
        {
            const int n = rd_i(); std::vector<int32_t> s((size_t)n); rd(s.data(), s.size() * 4);
            std::vector<double> co((size_t)n * 8), nc((size_t)n * 8); rd(co.data(), co.size() * 8); rd(nc.data(), nc.size() * 8);
            for (int i = 0; i < n; i++) for (int c = 0; c < 8; c++) { corrected[&kf[s[i]]][c] = co[(size_t)i * 8 + c]; non[&kf[s[i]]][c] = nc[(size_t)i * 8 + c]; }
        }
        std::map<mock::LoopKeyFrame*, std::set<mock::LoopKeyFrame*>> lc;
        for (int32_t n = rd_i(); n > 0; n--) { const int key = rd_i(); for (int32_t c = rd_i(); c > 0; c--) lc[&kf[key]].insert(&kf[rd_i()]); }
        const CorbEssentialGraphResult r = g.OptimizeEssentialGraph<mock::LoopMapPoint, mock::Mat>(&kf[loop_slot], &kf[cur_slot], non, corrected, lc, fix_scale != 0, scale, kfs, mps, 0, vpMP,
                                                                                                  &cache, [](const Sim3& s, double* v) { for (int i = 0; i < 8; i++) v[i] = s[i]; }, min_weight);
        printf("R %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", r.graph.n_vertices, r.graph.n_edges, r.graph.n_kind[0], r.graph.n_kind[1], r.graph.n_kind[2], r.graph.n_kind[3],
               r.graph.n_dropped, r.iters_done, r.n_poses_set, r.n_points_moved, r.n_points_kept, r.n_points_skipped, r.n_points_fixed_ref, cache.nUpdKF, cache.nUpdMP);
        for (int k = 0; k < K; k++) { printf("L %d", k); for (auto* p : g.GetLoopEdges(&kf[k])) printf(" %lu", p->mnId); printf("\n"); }
    }
    for (int k = 0; k < K; k++) { printf("K %d", k); print_floats(kf[k].Tcw.f, 16); printf("\n"); }
    for (int j = 0; j < n_mp; j++) {
        printf("P %d", j); print_floats(mp[j].pos.f, 3); print_floats(mp[j].normal.f, 3);
        uint32_t a, b; std::memcpy(&a, &mp[j].minDistance, 4); std::memcpy(&b, &mp[j].maxDistance, 4);
        printf(" %08x %08x\n", a, b);
    }
    corb_kf_store_destroy(kfs); corb_mp_store_destroy(mps);
    fclose(f);
    return 0;
}

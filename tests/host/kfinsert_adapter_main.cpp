// kfinsert_adapter_main.cpp -- drives corb::adapt::KeyFrameInsertT (corb-slam_amd/host/corb_adapter_orbslam.hpp) on the test doubles of tests/host/mock_orbslam.hpp:
// a map is filed with MapStoreT::PutKeyFrame / PutMapPoints, then one keyframe goes through CreateStereoPoints, the index, ProcessNewKeyFrame and MapPointCulling.
// TEST INFRASTRUCTURE, not product code.
//   kfinsert_adapter_main <in.bin> : int32 n_kf, n_mp, F, O, slot, mode, kf_first, kf_n, n_extra_recent | float th_depth, scale_factor | u64 first_mp_id, cur_kf_id |
//     float fx, fy, cx, cy, bf, mb, scale[8] | per keyframe: u64 id, int32 n, float Tcw[16], x[n], y[n], int32 octave[n], float ur[n], depth[n], u64 mp_id[n], u8 desc[n][32] |
//     per map point: u64 id, ref_kf_id, int32 bad, n_obs, found, visible, i64 first_kf, float pos[3], then n_obs x (u64 keyframe id, u32 feature) | int32 extra_recent[..]
// Prints one line per stage: the outputs of the calls as integers and IEEE bit patterns.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <map>
#include <memory>
#include <vector>
#include "mock_orbslam.hpp"
#include "corb_adapter_orbslam.hpp"

namespace corb { namespace adapt {
template <> struct MatFactory<mock::Mat> { static mock::Mat from_floats(int rows, int cols, const float* p) { mock::Mat m; m.rows = rows; m.cols = cols; m.f.assign(p, p + rows * cols); return m; } };
} }
using Store = corb::adapt::MapStoreT<mock::KeyFrame, mock::MapPoint, mock::Mat>;
using Insert = corb::adapt::KeyFrameInsertT<mock::KeyFrame, mock::MapPoint>;

static FILE* g_in;
template <class T> static T rd() { T v; if (fread(&v, sizeof(T), 1, g_in) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
template <class T> static std::vector<T> rdv(size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, g_in) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

int main(int argc, char** argv)
{
    if (argc < 2 || !(g_in = fopen(argv[1], "rb"))) return 2;
    const int n_kf = rd<int32_t>(), n_mp = rd<int32_t>(), F = rd<int32_t>(), O = rd<int32_t>(), slot = rd<int32_t>(), mode = rd<int32_t>(), kf_first = rd<int32_t>(), kf_n = rd<int32_t>(),
              n_extra = rd<int32_t>();
    const float th_depth = rd<float>(), scale_factor = rd<float>();
    const uint64_t first_mp_id = rd<uint64_t>(), cur_kf_id = rd<uint64_t>();
    CorbTrackCamera cam; memset(&cam, 0, sizeof(cam));
    cam.fx = rd<float>(); cam.fy = rd<float>(); cam.cx = rd<float>(); cam.cy = rd<float>(); cam.bf = rd<float>(); cam.mb = rd<float>();
    cam.min_x = 0; cam.max_x = 1241; cam.min_y = 0; cam.max_y = 376; cam.nlevels = 8;
    for (int l = 0; l < 8; l++) cam.scale[l] = rd<float>();

    CorbKfStore* kfs = nullptr; CorbMpStore* mps = nullptr;
    corb::check(corb_kf_store_create(0, n_kf, F, &kfs), "corb_kf_store_create");
    corb::check(corb_mp_store_create(0, n_mp + F, O, &mps), "corb_mp_store_create");
    std::vector<std::unique_ptr<mock::KeyFrame>> K; std::map<uint64_t, mock::KeyFrame*> by_id;
    for (int s = 0; s < n_kf; s++) {
        auto k = std::make_unique<mock::KeyFrame>();
        k->mnId = (unsigned long)rd<uint64_t>(); const int n = rd<int32_t>(); k->N = n;
        k->Tcw.rows = k->Tcw.cols = 4; k->Tcw.f = rdv<float>(16);
        const auto x = rdv<float>(n), y = rdv<float>(n); const auto oct = rdv<int32_t>(n);
        k->mvuRight = rdv<float>(n); k->mvDepth = rdv<float>(n);
        const auto ids = rdv<uint64_t>(n);
        k->mDescriptors.rows = n; k->mDescriptors.cols = 32; k->mDescriptors.b = rdv<uint8_t>((size_t)n * 32);
        k->mvKeysUn.resize(n);
        for (int i = 0; i < n; i++) k->mvKeysUn[i] = mock::KeyPoint{{x[i], y[i]}, 31.f, 0.f, 0.f, oct[i], -1};
        k->mvKeys = k->mvKeysUn; k->mps.assign(n, nullptr);
        k->fx = cam.fx; k->fy = cam.fy; k->cx = cam.cx; k->cy = cam.cy; k->mbf = cam.bf;
        for (int l = 0; l < 8; l++) k->mvInvLevelSigma2.push_back(1.0f / (cam.scale[l] * cam.scale[l]));
        Store::PutKeyFrame(kfs, s, k.get(), 1);
        if (n) corb::check(corb_kf_store_set_map_points(kfs, s, ids.data()), "corb_kf_store_set_map_points");      // (ids of points the doubles do not hold as objects among them)
        by_id[k->mnId] = k.get(); K.push_back(std::move(k));
    }
    std::vector<std::unique_ptr<mock::MapPoint>> P; std::vector<mock::MapPoint*> vp; std::vector<CorbMapPointCounters> cnt;
    for (int s = 0; s < n_mp; s++) {
        auto p = std::make_unique<mock::MapPoint>();
        p->mnId = (unsigned long)rd<uint64_t>(); const uint64_t ref = rd<uint64_t>(); p->bad = rd<int32_t>() != 0; const int n_obs = rd<int32_t>();
        CorbMapPointCounters c; c.n_found = rd<int32_t>(); c.n_visible = rd<int32_t>(); c.replaced_by = 0; cnt.push_back(c);
        p->mnFirstKFid = (long)rd<int64_t>();
        p->pos.rows = 3; p->pos.cols = 1; p->pos.f = rdv<float>(3);
        for (int q = 0; q < n_obs; q++) {
            const uint64_t kid = rd<uint64_t>(); const uint32_t idx = rd<uint32_t>();
            if (!by_id.count(kid)) { auto k = std::make_unique<mock::KeyFrame>(); k->mnId = (unsigned long)kid; by_id[kid] = k.get(); K.push_back(std::move(k)); }      // a keyframe the cache does not hold
            p->obs[by_id[kid]] = idx;
        }
        p->refKF = by_id.count(ref) ? by_id[ref] : nullptr;
        vp.push_back(p.get()); P.push_back(std::move(p));
    }
    const auto extra = rdv<int32_t>((size_t)n_extra);
    fclose(g_in);
    Store::PutMapPoints(mps, 0, vp, 1);
    if (n_mp) corb::check(corb_mp_store_set_counters(mps, 0, n_mp, cnt.data()), "corb_mp_store_set_counters");
    corb::check(corb_mp_store_build_index(mps, 0, n_mp), "corb_mp_store_build_index");

    Insert ins(F, n_mp + F);
    mock::KeyFrame* pKF = K[(size_t)slot].get();
    // Tracking::CreateNewKeyFrame
    const auto sp = ins.CreateStereoPoints(*pKF, kfs, slot, mps, cam, th_depth, mode, true, n_mp, first_mp_id, 1, 77);
    printf("points %zu %d", sp.vOrder.size(), sp.nCreated);
    for (size_t j = 0; j < sp.vOrder.size(); j++) printf(" %d:%d", sp.vOrder[j], (int)sp.vKind[j]);
    for (float v : sp.vX3D) printf(" %08x", bits(v));
    printf("\n");
    std::map<mock::MapPoint*, int> slot_of;
    for (int s = 0; s < n_mp; s++) slot_of[vp[(size_t)s]] = s;
    for (int k = 0; k < sp.nCreated; k++) {                                      // the objects of the new points: what `new MapPoint(x3D, pKF, mpCacher)` leaves on the host
        auto p = std::make_unique<mock::MapPoint>(); p->mnId = (unsigned long)(first_mp_id + (uint64_t)k); p->mnFirstKFid = (long)pKF->mnId;
        slot_of[p.get()] = n_mp + k; vp.push_back(p.get()); P.push_back(std::move(p));
    }
    corb::check(corb_mp_store_build_index(mps, 0, n_mp + sp.nCreated), "corb_mp_store_build_index");
    // LocalMapping::ProcessNewKeyFrame
    const auto as = ins.ProcessNewKeyFrame(pKF, kfs, slot, mps, kf_first, kf_n, scale_factor, true);
    printf("assoc %d %zu", as.nAdded, as.vRecentSlots.size());
    for (uint8_t k : as.vKind) printf(" %d", (int)k);
    for (int32_t s : as.vRecentSlots) printf(" %d", s);
    printf("\n");
    // LocalMapping::MapPointCulling, some keyframes later
    std::list<mock::MapPoint*> recent;
    for (int32_t s : extra) recent.push_back(vp[(size_t)s]);
    for (int32_t s : as.vRecentSlots) recent.push_back(vp[(size_t)s]);
    const auto dec = ins.MapPointCulling(recent, [&](mock::MapPoint* p) { return slot_of[p]; }, mps, (unsigned long)cur_kf_id, false, kfs, kf_first, kf_n, true);
    printf("cull %zu %zu", dec.size(), recent.size());
    for (uint8_t d : dec) printf(" %d", (int)d);
    for (mock::MapPoint* p : recent) printf(" %d", slot_of[p]);
    printf("\n");
    const auto c = ins.NeedNewKeyFrameCounts(kfs, slot, mps, th_depth, kfs, slot, 3, kf_first, kf_n);
    printf("counts %d %d %d\n", c.nTrackedClose, c.nNonTrackedClose, c.nRefMatches);
    corb_kf_store_destroy(kfs); corb_mp_store_destroy(mps);
    return 0;
}

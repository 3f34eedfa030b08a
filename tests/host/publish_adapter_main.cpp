// publish_adapter_main.cpp -- drives corb::adapt::MapPublishT (corb-slam_amd/host/corb_adapter_orbslam.hpp) on the test doubles of tests/host/mock_orbslam.hpp: a
// server map and a client map are filed with MapStoreT::PutKeyFrame / PutMapPoints, the server packs its four sets of light handles and transMs, the client applies.
// TEST INFRASTRUCTURE, not product code.
//   publish_adapter_main <in.bin> : int32 F, O, client_id, n_skf, n_smp, n_ckf, n_cmp, kf_n, kf_room, mp_n, mp_room, nA, nB, nC, nD, n_trans |
//     per keyframe (server's, then client's): u64 id, int32 client, fixed, n, float Tcw[16] | per map point (server's, then client's): u64 id, int32 client, fixed,
//     float pos[3] | u64 ids of the sets newKFs[nA], newMPs[nB], updKFs[nC], updMPs[nD] | per table entry: int32 client, float T[16]
// Prints the outputs of the apply and, per client record, id, flags and the pose / position as IEEE bit patterns.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <set>
#include <vector>
#include "mock_orbslam.hpp"
#include "corb_adapter_orbslam.hpp"

namespace corb { namespace adapt {
template <> struct MatFactory<mock::Mat> { static mock::Mat from_floats(int rows, int cols, const float* p) { mock::Mat m; m.rows = rows; m.cols = cols; m.f.assign(p, p + rows * cols); return m; } };
} }
using Store = corb::adapt::MapStoreT<mock::KeyFrame, mock::MapPoint, mock::Mat>;
using Publish = corb::adapt::MapPublishT<mock::Mat>;
struct Light { unsigned long mnId; bool operator<(const Light& o) const { return mnId < o.mnId; } };      // LightKeyFrame / LightMapPoint: ordered by mnId

static FILE* g_in;
template <class T> static T rd() { T v; if (fread(&v, sizeof(T), 1, g_in) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
template <class T> static std::vector<T> rdv(size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, g_in) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static std::vector<std::unique_ptr<mock::KeyFrame>> g_kf; static std::vector<std::unique_ptr<mock::MapPoint>> g_mp;
static void file_keyframes(CorbKfStore* s, int n, std::map<unsigned long, int>* slot_of)
{
    for (int k = 0; k < n; k++) {
        auto kf = std::make_unique<mock::KeyFrame>();
        kf->mnId = (unsigned long)rd<uint64_t>(); const int client = rd<int32_t>(); kf->fixed = rd<int32_t>() != 0; kf->N = rd<int32_t>();
        kf->Tcw.rows = kf->Tcw.cols = 4; kf->Tcw.f = rdv<float>(16);
        kf->mvKeysUn.assign((size_t)kf->N, mock::KeyPoint{{1.f, 2.f}, 31.f, 0.f, 0.f, 0, -1}); kf->mvKeys = kf->mvKeysUn; kf->mvuRight.assign((size_t)kf->N, -1.f); kf->mps.assign((size_t)kf->N, nullptr);
        Store::PutKeyFrame(s, k, kf.get(), client);
        if (slot_of && !slot_of->count(kf->mnId)) (*slot_of)[kf->mnId] = k;
        g_kf.push_back(std::move(kf));
    }
}
static void file_map_points(CorbMpStore* s, int n, std::map<unsigned long, int>* slot_of)
{
    for (int k = 0; k < n; k++) {
        auto p = std::make_unique<mock::MapPoint>();
        p->mnId = (unsigned long)rd<uint64_t>(); const int client = rd<int32_t>(); p->fixed = rd<int32_t>() != 0;
        p->pos.rows = 3; p->pos.cols = 1; p->pos.f = rdv<float>(3);
        Store::PutMapPoints(s, k, std::vector<mock::MapPoint*>{p.get()}, client);
        if (slot_of && !slot_of->count(p->mnId)) (*slot_of)[p->mnId] = k;
        g_mp.push_back(std::move(p));
    }
}

int main(int argc, char** argv)
{
    if (argc < 2 || !(g_in = fopen(argv[1], "rb"))) return 2;
    const int F = rd<int32_t>(), O = rd<int32_t>(), client_id = rd<int32_t>(), n_skf = rd<int32_t>(), n_smp = rd<int32_t>(), n_ckf = rd<int32_t>(), n_cmp = rd<int32_t>(),
              kf_n = rd<int32_t>(), kf_room = rd<int32_t>(), mp_n = rd<int32_t>(), mp_room = rd<int32_t>(), nA = rd<int32_t>(), nB = rd<int32_t>(), nC = rd<int32_t>(), nD = rd<int32_t>(),
              n_trans = rd<int32_t>();
    CorbKfStore *skf = nullptr, *ckf = nullptr; CorbMpStore *smp = nullptr, *cmp = nullptr;
    corb::check(corb_kf_store_create(0, n_skf, F, &skf), "corb_kf_store_create"); corb::check(corb_kf_store_create(0, n_ckf, F, &ckf), "corb_kf_store_create");
    corb::check(corb_mp_store_create(0, n_smp, O, &smp), "corb_mp_store_create"); corb::check(corb_mp_store_create(0, n_cmp, O, &cmp), "corb_mp_store_create");
    std::map<unsigned long, int> kf_slot, mp_slot;
    file_keyframes(skf, n_skf, &kf_slot); file_keyframes(ckf, n_ckf, nullptr);
    file_map_points(smp, n_smp, &mp_slot); file_map_points(cmp, n_cmp, nullptr);
    corb::check(corb_mp_store_build_index(cmp, 0, mp_n), "corb_mp_store_build_index");
    std::set<Light> newKFs, newMPs, updKFs, updMPs;
    for (uint64_t id : rdv<uint64_t>((size_t)nA)) newKFs.insert(Light{(unsigned long)id});
    for (uint64_t id : rdv<uint64_t>((size_t)nB)) newMPs.insert(Light{(unsigned long)id});
    for (uint64_t id : rdv<uint64_t>((size_t)nC)) updKFs.insert(Light{(unsigned long)id});
    for (uint64_t id : rdv<uint64_t>((size_t)nD)) updMPs.insert(Light{(unsigned long)id});
    std::map<int, mock::Mat> transMs;
    for (int k = 0; k < n_trans; k++) { const int c = rd<int32_t>(); mock::Mat T; T.rows = T.cols = 4; T.f = rdv<float>(16); transMs[c] = T; }
    fclose(g_in);

    Publish server, client;
    // a handle the server's cache does not resolve is skipped, as `if( tKF )` skips it
    server.Pack(skf, smp, newKFs, newMPs, updKFs, updMPs, [&](unsigned long id) { return kf_slot.count(id) ? kf_slot[id] : -1; }, [&](unsigned long id) { return mp_slot.count(id) ? mp_slot[id] : -1; }, transMs);
    const Publish::Message m = server.GetMessage();
    printf("counts %d %d %d %d %d\n", m.counts[0], m.counts[1], m.counts[2], m.counts[3], m.counts[4]);
    const Publish::Applied a = client.Apply(m, client_id, ckf, 0, kf_n, kf_n, kf_room, cmp, 0, mp_n, mp_n, mp_room, true);
    printf("applied %d %d %d %d", a.nUpdatedKF, a.nUpdatedMP, a.bNoTransform ? 1 : 0, a.bFull ? 1 : 0);
    for (const auto* v : {&a.vKindNewKF, &a.vKindNewMP, &a.vKindUpdKF, &a.vKindUpdMP}) { printf(" |"); for (uint8_t k : *v) printf(" %d", (int)k); }
    printf(" |"); for (int32_t s : a.vNewKFSlots) printf(" %d", s);
    printf(" |"); for (int32_t s : a.vNewMPSlots) printf(" %d", s);
    printf("\n");
    for (int s = 0; s < n_ckf; s++) {
        CorbKeyFrameMeta meta; corb::check(corb_kf_store_get_meta(ckf, s, &meta), "corb_kf_store_get_meta");
        printf("kf %d %llu %d %u", s, (unsigned long long)meta.id, meta.client_id, meta.flags);
        for (int k = 0; k < 16; k++) printf(" %08x", bits(meta.Tcw[k]));
        printf("\n");
    }
    std::vector<CorbMapPointRecord> rec((size_t)n_cmp);
    corb::check(corb_mp_store_get(cmp, 0, n_cmp, rec.data(), nullptr, nullptr), "corb_mp_store_get");
    for (int s = 0; s < n_cmp; s++) printf("mp %d %llu %d %u %08x %08x %08x\n", s, (unsigned long long)rec[(size_t)s].id, rec[(size_t)s].client_id, rec[(size_t)s].flags, bits(rec[(size_t)s].world_pos[0]),
                                           bits(rec[(size_t)s].world_pos[1]), bits(rec[(size_t)s].world_pos[2]));
    corb_kf_store_destroy(skf); corb_kf_store_destroy(ckf); corb_mp_store_destroy(smp); corb_mp_store_destroy(cmp);
    return 0;
}

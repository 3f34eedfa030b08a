// fusion_adapter_main.cpp -- drives corb::adapt::MapFusionDetectT (corb-slam_amd/host/corb_adapter_orbslam.hpp) and the mirror functions of corb_host.hpp for
// include/corb_map_fusion.h on test doubles that carry the members the server's detection loop reads of a KeyFrame.  TEST INFRASTRUCTURE, not product code.
//   fusion_adapter_main <voc.txt> <in.bin>
//     int32 n_global, n_sub, F, max_words, n_map_points, n_draws
//     per global keyframe (in entry order), then per sub keyframe: int32 slot (-1: no record), bad, n, u64 id; if slot >= 0 and n > 0: kp[n] (28 B), desc[n][32],
//       mp_id[n] (u64), int32 n_nodes, node_id[n_nodes], offset[n_nodes + 1], idx[offset[n_nodes]]; then the BowVector int32 n_words, word[u32], value[f64]; int32 nb[10]
//     float cam5[5] (fx fy cx cy bf of every record), CorbMapPointRecord[n_map_points], CorbTrackCamera, int32 draws[n_draws]
// Prints the definition's text (tests/fusion_reference.rows_text): `offsets ...`, one `row query entry slot n_matches kept ids_offset` per row, `ids ...` in hex;
// then `detect n0 n1 ...` = the candidates per sub keyframe of KeyFrameDatabase::DetectMapFusionCandidatesFromDB(vector) on a twin database; then
// `pose iKeyFrame row nTried nInliers kind` (refined: Refine()'s pose; best: the running best returned with bNoMore; none) and the pose's twelve floats as bit patterns.
#include <cstddef>
#include <cstdint>
#include <vector>
#include "corb_adapter_orbslam.hpp"
#include <cstdio>

namespace mock {
struct KeyFrame {
    unsigned long mnId = 0;
    std::map<unsigned, double> mBowVec;
    std::vector<KeyFrame*> best; int slot = -1;
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(int n) { return std::vector<KeyFrame*>(best.begin(), best.begin() + std::min((size_t)n, best.size())); }
    std::set<KeyFrame*> GetConnectedKeyFrames() { return {}; }
};
}
typedef corb::KeyFrameDatabase<mock::KeyFrame> Db;
static unsigned bits(float v) { unsigned b; std::memcpy(&b, &v, 4); return b; }

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* f = fopen(argv[2], "rb"); if (!f) return 2;
    auto rd = [&](void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } };
    corb::ORBVocabulary voc(argv[1]);
    int32_t hdr[6]; rd(hdr, sizeof(hdr));
    const int n_glob = hdr[0], n_sub = hdr[1], F = hdr[2], max_words = hdr[3], n_mp = hdr[4], n_draws = hdr[5];
    CorbKfStore *glob = nullptr, *sub = nullptr; CorbMpStore* map = nullptr;
    corb::check(corb_kf_store_create(0, n_glob, F, &glob), "corb_kf_store_create"); corb::check(corb_kf_store_create(0, n_sub, F, &sub), "corb_kf_store_create");
    std::vector<mock::KeyFrame> kf((size_t)n_glob + n_sub);
    std::vector<std::vector<int32_t>> nb(kf.size(), std::vector<int32_t>(10));
    struct Rec { int32_t slot, bad, n; uint64_t id; std::vector<CorbKeyPoint> kp; std::vector<uint8_t> desc; std::vector<uint64_t> mp; std::vector<uint32_t> node, idx; std::vector<int32_t> off; };
    std::vector<Rec> rec(kf.size());
    for (size_t k = 0; k < kf.size(); k++) {
        Rec& r = rec[k]; rd(&r.slot, 4); rd(&r.bad, 4); rd(&r.n, 4); rd(&r.id, 8);
        if (r.slot >= 0 && r.n > 0) {
            int32_t nn; r.kp.resize(r.n); r.desc.resize((size_t)r.n * 32); r.mp.resize(r.n);
            rd(r.kp.data(), (size_t)r.n * sizeof(CorbKeyPoint)); rd(r.desc.data(), r.desc.size()); rd(r.mp.data(), (size_t)r.n * 8);
            rd(&nn, 4); r.node.resize(nn); r.off.resize((size_t)nn + 1); rd(r.node.data(), (size_t)nn * 4); rd(r.off.data(), ((size_t)nn + 1) * 4);
            r.idx.resize(r.off[nn]); rd(r.idx.data(), r.idx.size() * 4);
        }
        int32_t nw; rd(&nw, 4); std::vector<uint32_t> w(nw); std::vector<double> v(nw); rd(w.data(), (size_t)nw * 4); rd(v.data(), (size_t)nw * 8);
        for (int i = 0; i < nw; i++) kf[k].mBowVec[w[i]] = v[i];
        rd(nb[k].data(), 40);
        kf[k].mnId = (unsigned long)r.id; kf[k].slot = r.slot;
    }
    float cam5[5]; rd(cam5, sizeof(cam5));
    for (size_t k = 0; k < kf.size(); k++) {                      // the records, as MapStoreT::PutKeyFrame files a keyframe: features, header, BoW groups, map-point ids
        const Rec& r = rec[k];
        if (r.slot < 0 || r.n <= 0) continue;
        CorbKfStore* s = k < (size_t)n_glob ? glob : sub;
        CorbKeyFrameMeta m; std::memset(&m, 0, sizeof(m));
        m.id = r.id; m.client_id = 1; m.flags = r.bad ? CORB_KF_BAD : 0; m.fx = cam5[0]; m.fy = cam5[1]; m.cx = cam5[2]; m.cy = cam5[3]; m.bf = cam5[4]; m.nlevels = 8;
        corb::check(corb_kf_store_put_frame(s, r.slot, r.kp.data(), r.desc.data(), nullptr, nullptr, r.n, &m), "corb_kf_store_put_frame");
        const CorbFeatVec fv = {(int32_t)r.node.size(), r.node.data(), r.off.data(), r.idx.data()};
        corb::check(corb_kf_store_set_bow(s, r.slot, &fv), "corb_kf_store_set_bow");
        corb::check(corb_kf_store_set_map_points(s, r.slot, r.mp.data()), "corb_kf_store_set_map_points");
        std::vector<uint8_t> fl(r.n); for (int i = 0; i < r.n; i++) fl[i] = r.mp[i] != CORB_NO_MAP_POINT;
        corb::check(corb_kf_store_set_flags(s, r.slot, fl.data()), "corb_kf_store_set_flags");
    }
    std::vector<CorbMapPointRecord> mps((size_t)std::max(n_mp, 1)); rd(mps.data(), (size_t)n_mp * sizeof(CorbMapPointRecord));
    CorbTrackCamera cam; rd(&cam, sizeof(cam));
    std::vector<int32_t> draws((size_t)n_draws); rd(draws.data(), draws.size() * 4);
    fclose(f);
    corb::check(corb_mp_store_create(0, n_mp + 4, 4, &map), "corb_mp_store_create");
    std::vector<int32_t> zero_off((size_t)n_mp + 1, 0);
    const uint64_t no_kf = 0; const uint32_t no_idx = 0;        // (no observations: the PnP RANSAC reads positions and flags only)
    corb::check(corb_mp_store_put_host(map, 0, n_mp, mps.data(), zero_off.data(), &no_kf, &no_idx), "corb_mp_store_put_host");
    corb::check(corb_mp_store_build_index(map, 0, n_mp), "corb_mp_store_build_index");

    // two databases filled alike: entries in keyframe order (a keyframe's entry is given at first sight), every global keyframe added, then the neighbours
    Db db(voc, (int)kf.size(), max_words), twin(voc, (int)kf.size(), max_words);
    for (Db* d : {&db, &twin}) {
        for (int g = 0; g < n_glob; g++) if (d->Entry(&kf[g]) != g) return 3;
        for (int g = 0; g < n_glob; g++) d->add(&kf[g]);
        for (int g = 0; g < n_glob; g++) { kf[g].best.clear(); for (int j : nb[g]) if (j >= 0) kf[g].best.push_back(&kf[j]); d->UpdateConnections(&kf[g]); }
    }
    std::vector<int32_t> entry_slot((size_t)db.Capacity(), -1);
    for (int g = 0; g < n_glob; g++) entry_slot[g] = rec[g].slot;
    std::vector<mock::KeyFrame*> submap; for (int s = 0; s < n_sub; s++) submap.push_back(&kf[n_glob + s]);

    corb::adapt::MapFusionDetectT<mock::KeyFrame, Db> detect;
    const auto d = detect.Detect(submap, [](mock::KeyFrame* p) { return p->slot; }, db, sub, glob, entry_slot, map, cam, [&](size_t k) { return draws[k % draws.size()]; },
                                 n_sub * db.Capacity(), (int64_t)n_sub * 16 * F);
    printf("offsets"); for (int o : d.cand.rowOffset) printf(" %d", o); printf("\n");
    for (const CorbFusionRow& r : d.cand.rows) printf("row %d %d %d %d %d %lld\n", r.query, r.entry, r.slot, r.n_matches, r.kept, (long long)r.ids_offset);
    printf("ids"); for (uint64_t i : d.cand.ids) printf(" %llx", (unsigned long long)i); printf("\n");
    printf("detect"); for (auto& l : twin.DetectMapFusionCandidatesFromDB(submap)) printf(" %zu", l.size()); printf("\n");
    int inl = 0; for (uint8_t b : d.vbInliers) inl += b;
    printf("pose %d %d %d %d %s", d.iKeyFrame, d.row, d.nTried, inl, d.iKeyFrame < 0 ? "none" : d.bRefined ? "refined" : "best"); for (int j = 0; j < 12; j++) printf(" %08x", bits(d.Tcw[j])); printf("\n");
    // the mirror of the matcher's batch form on the first two rows that have a record, against the rows' counts
    std::vector<int32_t> sa, sb, want;
    for (const CorbFusionRow& r : d.cand.rows) if (r.slot >= 0 && sa.size() < 2) { sa.push_back(r.slot); sb.push_back(submap[r.query]->slot); want.push_back(r.n_matches); }
    const corb::BowMatches bm = corb::SearchByBoWSlotsBatch(0, glob, sa, sub, sb, 0.75f, true, F);
    printf("bow %d\n", (int)(bm.count == want));
    corb_kf_store_destroy(glob); corb_kf_store_destroy(sub); corb_mp_store_destroy(map);
    return 0;
}

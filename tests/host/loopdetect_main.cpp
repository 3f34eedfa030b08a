// loopdetect_main.cpp -- drives corb::adapt::LoopDetectT<KeyFrame, KeyFrameDatabase> (corb-slam_amd/host/corb_adapter_orbslam.hpp) and through it corb::LoopDetector
// (corb_host.hpp) on test doubles: keyframes filed in a store with their map points, the covisibility rows by corb_covis_update, BowVectors handed over as data.
// TEST INFRASTRUCTURE, not product code.
//   loopdetect_main <voc.txt> <in.bin> : int32 n_slots, F, n_kf, n_mp, n_obs, M, th, max_queue, n_ops; per keyframe (ascending id) int32 slot, n_feat, n_words, n_best;
//       CorbKeyFrameMeta; u64 mp_id[n_feat]; u32 word[n_words]; f64 value[n_words]; int32 best[n_best] (keyframe indices: GetBestCovisibilityKeyFrames(10));
//       then CorbMapPointRecord[n_mp], int32 obs_off[n_mp + 1], u64 obs_kf[n_obs], u32 obs_idx[n_obs]; per op int32 code, arg:
//       0 add keyframe arg to the database (an old keyframe)   1 InsertKeyFrame(arg)   2 DetectLoop() until the queue is empty or a loop is detected
//       3 mLastLoopKFid = id of keyframe arg (CorrectLoop)     4 Bind(arg) without queueing
// Prints per consumed keyframe `D outcome minScore-bits | candidates' slots | enough candidates' slots`, per DetectLoop() call `R ret mpCurrentKF's-id queue-size |
// mvpEnoughConsistentCandidates' ids`, and the groups `G counter members' slots` after it.
#include <cstddef>
#include <cstdint>
#include <vector>
#include "corb_adapter_orbslam.hpp"
#include <cstdio>

namespace mock {
struct KeyFrame {
    unsigned long mnId = 0; int slot = -1;
    std::map<unsigned, double> mBowVec;
    std::vector<KeyFrame*> best;
    std::set<KeyFrame*> GetConnectedKeyFrames() { return std::set<KeyFrame*>(); }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(int n) { return std::vector<KeyFrame*>(best.begin(), best.begin() + std::min((size_t)n, best.size())); }
};
struct Frame { unsigned long mnId = 0; std::map<unsigned, double> mBowVec; };
}
typedef corb::KeyFrameDatabase<mock::KeyFrame, mock::Frame> Db;

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* f = fopen(argv[2], "rb"); if (!f) return 2;
    auto rd = [&](void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } };
    corb::ORBVocabulary voc(argv[1]);
    int32_t hdr[9]; rd(hdr, sizeof(hdr));
    const int S = hdr[0], F = hdr[1], n_kf = hdr[2], n_mp = hdr[3], n_obs = hdr[4], M = hdr[5], th = hdr[6], max_queue = hdr[7], n_ops = hdr[8];
    CorbKfStore* kfs = nullptr; CorbMpStore* mps = nullptr; CorbCovis* g = nullptr;
    corb::check(corb_kf_store_create(0, S, F, &kfs), "corb_kf_store_create");
    corb::check(corb_mp_store_create(0, n_mp, 4, &mps), "corb_mp_store_create");
    std::vector<mock::KeyFrame> kf((size_t)n_kf);
    std::vector<int32_t> slots;
    for (int k = 0; k < n_kf; k++) {
        int32_t h[4]; CorbKeyFrameMeta meta; rd(h, sizeof(h)); rd(&meta, sizeof(meta));
        std::vector<uint64_t> mp((size_t)h[1]); rd(mp.data(), mp.size() * 8);
        std::vector<uint32_t> w((size_t)h[2]); std::vector<double> v((size_t)h[2]); rd(w.data(), w.size() * 4); rd(v.data(), v.size() * 8);
        std::vector<int32_t> best((size_t)h[3]); rd(best.data(), best.size() * 4);
        kf[k].mnId = (unsigned long)meta.id; kf[k].slot = h[0];
        for (size_t i = 0; i < w.size(); i++) kf[k].mBowVec[w[i]] = v[i];
        for (int32_t b : best) kf[k].best.push_back(&kf[(size_t)b]);
        const int32_t off[2] = {0, h[1]}; std::vector<CorbKeyPoint> kp((size_t)h[1]); std::memset(kp.data(), 0, kp.size() * sizeof(CorbKeyPoint));
        corb::check(corb_kf_store_put_batch(kfs, h[0], 1, &meta, off, kp.data(), nullptr, nullptr, nullptr, mp.data()), "corb_kf_store_put_batch");
        slots.push_back(h[0]);
    }
    {
        std::vector<CorbMapPointRecord> rec((size_t)n_mp); std::vector<int32_t> off((size_t)n_mp + 1); std::vector<uint64_t> okf((size_t)n_obs); std::vector<uint32_t> oidx((size_t)n_obs);
        rd(rec.data(), rec.size() * sizeof(CorbMapPointRecord)); rd(off.data(), off.size() * 4); rd(okf.data(), okf.size() * 8); rd(oidx.data(), oidx.size() * 4);
        corb::check(corb_mp_store_put_host(mps, 0, n_mp, rec.data(), off.data(), okf.data(), oidx.data()), "corb_mp_store_put_host");
        corb::check(corb_mp_store_build_index(mps, 0, n_mp), "corb_mp_store_build_index");
    }
    corb::check(corb_covis_create(kfs, mps, M, &g), "corb_covis_create");
    corb::check(corb_covis_update(g, slots.data(), n_kf, th, nullptr), "corb_covis_update");
    int rc = 0;
    {
        Db db(voc, n_kf + 2, 512);
        corb::adapt::LoopDetectT<mock::KeyFrame, Db> lc(g, db, [](mock::KeyFrame* p) { return p->slot; }, S, 8, 16, max_queue);
        for (int o = 0; o < n_ops; o++) {
            int32_t op[2]; rd(op, sizeof(op));
            mock::KeyFrame* p = &kf[(size_t)op[1]];
            if (op[0] == 0) { lc.Bind(p); db.add(p); }
            else if (op[0] == 1) lc.InsertKeyFrame(p);
            else if (op[0] == 3) lc.SetLastLoop(p);
            else if (op[0] == 4) lc.Bind(p);
            else if (op[0] == 2) {
                bool ret = false;
                while (lc.CheckNewKeyFrames() && !ret) {
                    ret = lc.DetectLoop();
                    for (const corb::LoopDetection& d : lc.consumed) {
                        printf("D %d %08x |", d.result.outcome, d.result.min_score_bits);
                        for (int32_t s : d.candSlots) printf(" %d", s);
                        printf(" |");
                        for (int32_t i : d.enough) printf(" %d", d.candSlots[(size_t)i]);
                        printf("\n");
                    }
                    printf("R %d %lu %zu |", ret ? 1 : 0, lc.mpCurrentKF ? lc.mpCurrentKF->mnId : 0ul, lc.QueueSize());
                    for (mock::KeyFrame* q : lc.mvpEnoughConsistentCandidates) printf(" %lu", q->mnId);
                    printf("\n");
                    const corb::ConsistentGroups G = lc.detector().Groups(S);
                    for (int i = 0; i < G.n(); i++) { printf("G %d", G.counters[(size_t)i]); for (int j = G.offsets[(size_t)i]; j < G.offsets[(size_t)i + 1]; j++) printf(" %d", G.members[(size_t)j]); printf("\n"); }
                }
            }
        }
    }
    fclose(f);
    corb_covis_destroy(g); corb_kf_store_destroy(kfs); corb_mp_store_destroy(mps);
    return rc;
}

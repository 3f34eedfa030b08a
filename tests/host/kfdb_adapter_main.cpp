// kfdb_adapter_main.cpp -- drives corb::ORBVocabulary and corb::KeyFrameDatabase<KeyFrame, Frame> (corb-slam_amd/host/corb_adapter_orbslam.hpp) on test doubles that carry
// the members KeyFrameDatabase.cc reads.  TEST INFRASTRUCTURE, not product code.
//   kfdb_adapter_main <voc.txt> <in.bin> : int32 n_keyframes, levelsup, n_ops; per op int32 code ...
//       0 bow e n desc[n][32] (ComputeBoW of keyframe e)   1 add e   2 erase e   3 clear   4 nb e nb[10]   5 query kind e id(u64) min_score(f32) nc conn[nc]
// Prints per query `Q n candidates...` and one `st` line per keyframe with its six fields (floats as bit patterns), and per bow op the score of the vector with itself.
#include <cstddef>
#include <cstdint>
#include <vector>
#include "corb_adapter_orbslam.hpp"
#include <cstdio>

namespace mock {
struct Desc { uint8_t b[32]; template <class T> const T* ptr(int) const { return reinterpret_cast<const T*>(b); } };
struct KeyFrame {
    unsigned long mnId = 0;
    std::map<unsigned, double> mBowVec; std::map<unsigned, std::vector<unsigned>> mFeatVec;
    std::set<KeyFrame*> conn; std::vector<KeyFrame*> best;
    std::set<KeyFrame*> GetConnectedKeyFrames() { return conn; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(int n) { return std::vector<KeyFrame*>(best.begin(), best.begin() + std::min((size_t)n, best.size())); }
};
struct Frame { unsigned long mnId = 0; std::map<unsigned, double> mBowVec; };
}
static unsigned bits(float v) { unsigned b; std::memcpy(&b, &v, 4); return b; }
static unsigned long long bits(double v) { unsigned long long b; std::memcpy(&b, &v, 8); return b; }

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* f = fopen(argv[2], "rb"); if (!f) return 2;
    auto rd = [&](void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } };
    corb::ORBVocabulary voc(argv[1]);
    int32_t hdr[3]; rd(hdr, sizeof(hdr));
    const int n_kf = hdr[0], levelsup = hdr[1], n_ops = hdr[2];
    std::vector<mock::KeyFrame> kf((size_t)n_kf);
    corb::KeyFrameDatabase<mock::KeyFrame, mock::Frame> db(voc, n_kf, 128);
    for (int o = 0; o < n_ops; o++) {
        int32_t code, e = 0; rd(&code, 4); if (code != 3) rd(&e, 4);
        if (code == 0) {
            int32_t n; rd(&n, 4); std::vector<mock::Desc> d((size_t)n); for (auto& x : d) rd(x.b, 32);
            voc.transform(d, kf[e].mBowVec, kf[e].mFeatVec, levelsup);
            size_t n_idx = 0; for (auto& g : kf[e].mFeatVec) n_idx += g.second.size();
            printf("B %zu %zu %zu %016llx\n", kf[e].mBowVec.size(), kf[e].mFeatVec.size(), n_idx, bits(voc.score(kf[e].mBowVec, kf[e].mBowVec)));
        } else if (code == 1) db.add(&kf[e]);
        else if (code == 2) db.erase(&kf[e]);
        else if (code == 3) db.clear();
        else if (code == 4) { int32_t nb[10]; rd(nb, sizeof(nb)); kf[e].best.clear(); for (int j : nb) if (j >= 0) kf[e].best.push_back(&kf[j]); db.UpdateConnections(&kf[e]); }
        else if (code == 5) {
            const int kind = e; int32_t q, nc; uint64_t id; float ms; rd(&q, 4); rd(&id, 8); rd(&ms, 4); rd(&nc, 4);
            std::vector<int32_t> c((size_t)nc); rd(c.data(), c.size() * 4);
            kf[q].mnId = (unsigned long)id; kf[q].conn.clear(); for (int j : c) kf[q].conn.insert(&kf[j]);
            std::vector<mock::KeyFrame*> out;
            if (kind == 0) out = db.DetectLoopCandidates(&kf[q], ms);
            else if (kind == 2) out = db.DetectMapFusionCandidatesFromDB(&kf[q]);
            else { mock::Frame F; F.mnId = (unsigned long)id; F.mBowVec = kf[q].mBowVec; out = db.DetectRelocalizationCandidates(&F); }
            printf("Q %zu", out.size()); for (auto* p : out) printf(" %d", (int)(p - kf.data())); printf("\n");
            for (auto& k : kf) { const CorbKfDbState s = db.State(&k); printf("st %llu %d %08x %llu %d %08x\n", (unsigned long long)s.loop_query, s.loop_words, bits(s.loop_score), (unsigned long long)s.reloc_query, s.reloc_words, bits(s.reloc_score)); }
        }
    }
    fclose(f);
    return 0;
}
